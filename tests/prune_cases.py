"""The project's own model of UnigramWP's removal losses (include/swt.h, swt_wp_removal_losses) in plain Python: the forward pass of
tests/viterbi_cases.py with a barred piece, numpy float32 adds and subtraction, the fixed point in Python ints."""
import math

import numpy as np

from tests.viterbi_cases import HANDMADE, WORDS, Model, dyadic, words_of  # noqa: F401  (and for the tests)

UNIT, CLAMP = 1 << 20, 1 << 40


def fix(b):  # B * 2^20 toward zero, within +-2^40
    return int(max(-float(CLAMP), min(float(CLAMP), float(b) * UNIT)))


def ufix(b, a):
    with np.errstate(all="ignore"):
        d = float(np.float32(b) - np.float32(a))  # (a NaN for two equal infinities, which compare equal)
    return 0 if b == a else CLAMP if math.isinf(d) else min(math.floor(d * UNIT), CLAMP)


class Prune(Model):
    def forward(self, word, barred=None):  # -> (best[n] or None, the path); with a barred piece only the total counts
        n = len(word)
        best, back = [np.float32(0.0)] + [None] * n, [None] * (n + 1)
        for j in range(1, n + 1):
            for i in range(j):
                piece = word[i:j] if i == 0 else "##" + word[i:j]
                if best[i] is None or piece not in self.vocab or piece == barred:
                    continue
                with np.errstate(over="ignore"):
                    cand = best[i] + self.score[piece]
                if best[j] is None or cand > best[j]:
                    best[j], back[j] = cand, (i, piece)
        path, j = [], n
        while j and best[n] is not None:
            j, piece = back[j]
            path.append(piece)
        return best[n], path[::-1]

    def word(self, word):  # -> None for an UNK word, or (fix(B), the path, {t: ufix(B, A_t), or None where t's removal orphans the word})
        b, path = self.forward(word) if len(word) <= self.max_word_chars else (None, [])
        if b is None:
            return None
        loss = {}
        for t in dict.fromkeys(path):
            a = self.forward(word, t)[0]
            assert a is None or a <= b, (word, t)  # rounding to nearest is monotone
            loss[t] = None if a is None else ufix(b, a)
        return fix(b), path, loss

    def batch(self, split, texts):  # (table uint64[3, n_vocab], stats int64[3]) as the device must give them
        table, stats, seen = np.zeros((3, len(self.ids)), dtype=np.uint64), [0, 0, 0], {}
        for text in texts:
            for word, _ in words_of(split, text.lower()):
                got = seen[word] if word in seen else seen.setdefault(word, self.word(word))
                if got is None:
                    stats[1] += 1
                    continue
                stats[0], stats[2] = stats[0] + 1, stats[2] + got[0]
                for t in got[1]:
                    table[0, self.ids[t]] += np.uint64(1)
                for t, u in got[2].items():
                    table[2 if u is None else 1, self.ids[t]] += np.uint64(1 if u is None else u)
        return table, np.array(stats, dtype=np.int64)
