"""The project's own model of MaxMatch-Dropout (include/swt.h, swt_wp_encode_naive_dropout) in plain Python, and
the builders of its test cases.  The reference has no dropout: this file holds the semantics, and the kernel equals it element by
element because a draw is Philox4x32-10 of (the code points a candidate takes, the byte offset of the state in its sentence, the
sentence, epoch) under the seed and of nothing else.

The walk is NaiveWP.encode_word's (wordpiece.py:131-158) with the state "#" * L + word[p:] kept as (p, L).  Non-termination is
decided as MaxMatch of tests/test_naive_wp_encode.py decides it -- a state seen twice, or L beyond the longest run of '#' any
token begins with plus the two put back -- and not by the kernel's count of steps."""
import random

import numpy as np

from tests.dropout_cases import drop_below, fill, words_of  # noqa: F401  (drop_below, fill: for the tests that import this module)
from tests.mlm_cases import philox_scalar

ONE = 1 << 32
M32 = 0xFFFFFFFF


def dropped(c, a, i, epoch, seed, below):
    """the draw of a candidate that takes c >= 2 code points from byte a of sentence i: word c & 3 of the Philox call at the
    counter (c >> 2, a, i, epoch) under the key (seed low word, seed high word), below the threshold"""
    x = philox_scalar(((c >> 2) & M32, a & M32, i & M32, epoch & M32), (seed & M32, (seed >> 32) & M32))
    return x[c & 3] < below


class Model:
    def __init__(self, vocab):
        self.vocab = set(vocab)
        self.ids = {t: k for k, t in enumerate(sorted(self.vocab))}
        self.unk = len(self.ids) + 1
        self.sharp_bound = max([2] + [len(t) - len(t.lstrip("#")) for t in self.vocab]) + 2
        self.longest = max([1] + [len(t) for t in self.vocab])

    def encode_word(self, word, below, seed, epoch, i, a0, stats=None):
        """the rule of include/swt.h on one word whose first byte is byte a0 of sentence i -> its tokens, ["[UNK]"], or None where
        the walk never returns.  stats, a dict, counts the candidates with c >= 2 "looked" at (every one of every step, as a walk
        that draws as it meets them does) and those "dropped"."""
        at = [0]
        for ch in word:
            at.append(at[-1] + len(ch.encode("utf-8", "surrogatepass")))
        pieces, seen, p, L = [], set(), 0, 0
        while True:
            state = "#" * L + word[p:]
            take = 0
            for n in range(min(len(state), self.longest), 0, -1):
                if state[:n] not in self.vocab:
                    continue
                c = max(n - L, 0)
                if c >= 2:
                    gone = dropped(c, a0 + at[p], i, epoch, seed, below)
                    if stats is not None:
                        stats["looked"] += 1
                        stats["dropped"] += gone
                    if gone:
                        continue
                take = max(take, n)
                if stats is None:
                    break  # (with stats every candidate of the step is drawn for, as the kernel does: the answer is the same)
            if take == 0:
                return ["[UNK]"]  # wordpiece.py:148-149: whatever was stored is discarded
            pieces.append(state[:take])
            if take == len(state):
                return pieces
            if take > L:
                p, L = p + take - L, 2
            else:
                L = L - take + 2
            if (p, L) in seen or L > self.sharp_bound:
                return None
            seen.add((p, L))

    def tokenize(self, split, texts, below, seed=0, epoch=0, first=0, stats=None):
        """-> per text its tokens, or None where a word of it never returns.  The sentence index of texts[j] is first + j."""
        res = []
        for j, text in enumerate(texts):
            toks = []
            for word, a0 in words_of(split, text.lower()):
                got = self.encode_word(word, below, seed, epoch, first + j, a0, stats)
                if got is None:
                    toks = None
                    break
                toks += got
            res.append(toks)
        return res

    def ids_of(self, tokens):
        return [self.unk if t == "[UNK]" else self.ids[t] for t in tokens]

    def batch(self, split, texts, below, seed=0, epoch=0, first=0):
        """(ids, offsets, status) as the device must give them"""
        ids, off, st = [], [0], []
        for toks in self.tokenize(split, texts, below, seed, epoch, first):
            st.append(0 if toks is not None else 1)
            if toks is not None:
                ids += self.ids_of(toks)
            off.append(len(ids))
        return np.array(ids, dtype=np.uint32), np.array(off, dtype=np.uint64), np.array(st, dtype=np.uint8)


def characters(split, texts):
    """every word as its code points: what drop_below = 2^32 gives where each is a token in its position"""
    return [[c if k == 0 else "##" + c for word, _ in split(t.lower()) for k, c in enumerate(word)] for t in texts]


def spelled(tokens):
    """the characters a row of tokens without "[UNK]" stands for"""
    return "".join(t[2:] if t.startswith("##") and len(t) > 2 else t for t in tokens)


# ---- vocabularies and texts -------------------------------------------------------------------------------------------
# the status depends on the draw: "abc" is a ##bc while "##bc" lives; once it is dropped the step at "##bc" takes "##" for ever
MICRO_LOOP = ["a", "##", "##bc"]
# and without "##" nothing is left there: one "[UNK]", the stored "a" discarded
MICRO_UNK = ["a", "##bc"]

# words of tests/test_gpu_wp_seams.py::handmade_vocab that NaiveWP returns from (no euro sign, no emoji: "##" is a token there)
WORDS = ["ab", "abc", "abcd", "cd", "xy", "aaaa", "a", "b", "dab", "xyxy", "abab", "żół", "żółżół", "óż", "łłł", "qa", "aaaaab",
         "abcdabcdabcd", "q" * 20, "q" * 41, ",", "-", ".", "x,y", "ab-cd", "a.b", "d.", "aaaaaaaa", "xyab", "żółab", "abżół"]


def short_sentences(n_sent, n_bytes, seed, words=WORDS, empty=37):
    """about n_bytes in n_sent short sentences of `words`, every empty-th of them empty"""
    rng = random.Random(seed)
    return ["" if s % empty == 5 else fill(rng.randrange(n_bytes // n_sent // 2, 3 * n_bytes // n_sent // 2), rng, words)
            for s in range(n_sent)]
