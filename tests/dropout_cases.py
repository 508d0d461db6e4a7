"""The project's own model of BPE-dropout (include/swt.h, swt_bpe_encode_dropout) in plain Python, and the
builders of its test cases.  The reference has no dropout: this file holds the semantics, and the kernel equals it element by
element because a draw is Philox4x32-10 of (round, pair index, the word's byte offset, its sentence, epoch) under the seed and
of nothing else.

A word is a list of symbols (strings; one code point each at the start).  `Table` gives a pair's rank and what it merges to:
from a merges list as FastBPE reads it (a later duplicate of a pair overrides, bpe.py:257; the merged symbol is left + right)."""
import random

import numpy as np

from tests.mlm_cases import philox

ONE = 1 << 32
CONT = 0x80000000  # SWT_BPE_CONT


def drop_below(p):
    """what the Python layer makes of a probability"""
    return int(round(float(p) * 4294967296.0))


class Table:
    def __init__(self, merges):
        self.merges = [tuple(m) for m in merges]
        self.rank = {pair: i for i, pair in enumerate(self.merges)}


def draws(t, n_pairs, b, i, epoch, seed):
    """x[k] for the pairs k = 0 .. n_pairs - 1 of round t of the word with the key (i, b): word k & 3 of the Philox call at the
    counter (((t << 16) + (k >> 2)) mod 2^32, b, i, epoch) under the key (seed low word, seed high word)"""
    groups = np.arange((n_pairs + 3) // 4, dtype=np.uint64)
    c0 = (np.uint64((t << 16) & 0xFFFFFFFF) + groups) & np.uint64(0xFFFFFFFF)
    x = philox(c0, b & 0xFFFFFFFF, i & 0xFFFFFFFF, epoch, seed & 0xFFFFFFFF, seed >> 32)
    return np.stack(x, axis=1).reshape(-1)[:n_pairs]


def encode_word(table, word, below, seed, epoch, i, b, stats=None):
    """the rule of include/swt.h on one word (a str) -> its symbols.  stats, a dict, counts "ranked" pair occurrences looked at
    and those "dropped"."""
    s = list(word)
    t = 0
    while len(s) >= 2:
        n = len(s)
        x = draws(t, n - 1, b, i, epoch, seed)
        ranked = [k for k in range(n - 1) if (s[k], s[k + 1]) in table.rank]
        live = [k for k in ranked if not int(x[k]) < below]
        if stats is not None:
            stats["ranked"] += len(ranked)
            stats["dropped"] += len(ranked) - len(live)
        if not live:
            break
        m = min(table.rank[(s[k], s[k + 1])] for k in live)
        alive = set(live)
        out, k = [], 0
        while k < n:
            if k in alive and table.rank[(s[k], s[k + 1])] == m:
                out.append(s[k] + s[k + 1])
                k += 2
            else:
                out.append(s[k])
                k += 1
        s = out
        t += 1
    return s


def words_of(split, lowered):
    """[(word, byte offset of its first byte in lowered's UTF-8)] by the pre-tokenizer `split` (SubwordTokenizer._split)"""
    out, at, seen = [], 0, 0
    for word, (start, _end) in split(lowered):
        at += len(lowered[seen:start].encode("utf-8", "surrogatepass"))
        seen = start
        out.append((word, at))
    return out


def tokenize(table, split, texts, below, seed=0, epoch=0, first=0, stats=None):
    """-> one list of tokens per text, '##' before every token that does not open its word.  The sentence index of texts[j] is
    first + j."""
    res = []
    for j, text in enumerate(texts):
        toks = []
        for word, b in words_of(split, text.lower()):
            syms = encode_word(table, word, below, seed, epoch, first + j, b, stats)
            toks += [syms[0]] + ["##" + x for x in syms[1:]]
        res.append(toks)
    return res


def ids_of(tokens, intern):
    """the model's tokens as the device's ids and sentence offsets; intern: symbol string -> id (one code point: its ordinal)"""
    ids, off = [], [0]
    for toks in tokens:
        for tok in toks:
            cont = tok.startswith("##") and len(tok) > 2
            sym = tok[2:] if cont else tok
            ids.append((ord(sym) if len(sym) == 1 else intern(sym)) | (CONT if cont else 0))
        off.append(len(ids))
    return np.array(ids, dtype=np.uint32), np.array(off, dtype=np.uint64)


def characters(split, texts):
    """every word as its code points: what drop_below = 2^32 gives"""
    return [[c if k == 0 else "##" + c for word, _ in split(t.lower()) for k, c in enumerate(word)] for t in texts]


# ---- tables ----------------------------------------------------------------------------------------------------------
# proper: every pair ranks above the merges that make its symbols (what training gives)
PROPER = [("a", "b"), ("c", "d"), ("ab", "cd"), ("x", "y"), ("ż", "ó"), ("żó", "ł"), ("q", "q"), ("abcd", "abcd"), ("qq", "qq"),
          ("abcdabcd", "abcd"), ("xy", "xy"), ("ó", "ł"), ("\U0001F600", "\U0001F600"), ("€", "a"), ("b", "a"), ("ab", "ab")]
# improper: ("ab", "c") ranks BELOW ("a", "b"), which makes its left symbol, ("a", "a") is listed twice and ("aa", "a") sits
# between its two positions -- the device takes the literal rounds (literal_rounds) for such a table, and so must the dropout form
IMPROPER = [("ab", "c"), ("a", "a"), ("a", "b"), ("aa", "a"), ("c", "d"), ("abc", "d"), ("a", "a"), ("x", "y"), ("xy", "x"),
            ("q", "q"), ("qq", "q"), ("b", "a")]

WORDS = ["ab", "abc", "abcd", "cd", "xy", "xyxy", "dab", "abab", "żół", "żółżół", "óż", "łłł", "qa", "aaaa", "bdbdbd", "abcdabcdabcd",
         "a", "b", "ż", "słowo", "nie", "wiem", "zażółć", ",", "x,y", "d.", "—", "¿co?", "aaaaaaa", "qqqqq", "abcabc", "xyx", "ba",
         "\U0001F600\U0001F600", "€a€a", "baba"]


def fill(n, rng, words=WORDS):
    """words separated by single spaces, n bytes of UTF-8 exactly (ends with a space; 'q' runs make up the remainder)"""
    out, left = [], n
    while left > 0:
        w = rng.choice(words)
        need = len(w.encode("utf-8")) + 1
        if need > left:
            w, need = "q" * (left - 1), left
        out.append(w)
        left -= need
    return " ".join(out) + " " if out else ""


def short_sentences(n_sent, n_bytes, seed):
    """about n_bytes in n_sent short sentences of handmade words, a few of them empty"""
    rng = random.Random(seed)
    out = []
    for s in range(n_sent):
        out.append("" if s % 37 == 5 else fill(rng.randrange(n_bytes // n_sent // 2, 3 * n_bytes // n_sent // 2), rng))
    return out
