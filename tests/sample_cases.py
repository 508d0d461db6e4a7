"""The project's own model of sampled UnigramWP (include/swt.h, swt_wp_encode_sample) in plain Python: wide float32 on integers.
A value is (m, e) = m * 2^e with m in [2^23, 2^24), or ZERO; every operation is exact, then rounded to nearest-even to 24 bits."""
import math

import numpy as np

from tests.dropout_cases import words_of  # noqa: F401  (and for the tests)
from tests.mlm_cases import philox_scalar
from tests.viterbi_cases import HANDMADE, WORDS  # noqa: F401  (for the tests that import this module)

ZERO, ONE, M32 = (0, 0), (1 << 23, -23), 0xFFFFFFFF


def rne(m, e):  # the integer m >= 0 times 2^e, rounded to 24 significant bits, ties to even
    if m == 0:
        return ZERO
    s = m.bit_length() - 24
    if s <= 0:
        return m << -s, e + s
    rest, m = m & ((1 << s) - 1), m >> s
    m += rest > 1 << (s - 1) or (rest == 1 << (s - 1) and m & 1)
    return (m >> 1, e + s + 1) if m == 1 << 24 else (m, e + s)


def mul(a, b):
    return rne(a[0] * b[0], a[1] + b[1])


def add(a, b):
    e = min(a[1], b[1]) if a[0] and b[0] else 0
    return b if not a[0] else a if not b[0] else rne((a[0] << (a[1] - e)) + (b[0] << (b[1] - e)), e)


def gt(a, b):
    return bool(a[0]) and (not b[0] or (a[1], a[0]) > (b[1], b[0]))


def wide(x):  # a float32 as a wide value
    m, e = math.frexp(float(x))
    return rne(int(m * (1 << 24)), e - 24)


def uniform(seed, epoch, s, a):  # u of the rule: the top 24 bits of word 0 of Philox at the counter (0, a, s, epoch), times 2^-24
    return rne(philox_scalar((0, a & M32, s & M32, epoch & M32), (seed & M32, (seed >> 32) & M32))[0] >> 8, -24)


def weights(scores, alpha):  # token -> float32(exp(alpha * score)), clamped into [2^-64, 2^64] before it is rounded
    return {t: np.float32(min(max(math.exp(alpha * float(np.float32(s))), 2.0 ** -64), 2.0 ** 64)) for t, s in scores.items()}


class Model:
    def __init__(self, vocab, weights, max_word_chars=100):
        self.vocab, self.max_word_chars = set(vocab), max_word_chars
        self.ids, self.unk = {t: k for k, t in enumerate(sorted(self.vocab))}, len(self.vocab) + 1
        self.w = {t: wide(np.float32(weights[t])) for t in self.vocab}

    def pieces(self, word, i):  # [(j, piece(i, j))] in rising j
        found = [(j, word[i:j] if i == 0 else "##" + word[i:j]) for j in range(i + 1, len(word) + 1)]
        return [(j, t) for j, t in found if t in self.vocab]

    def backward(self, word):
        b = [ZERO] * len(word) + [ONE]
        for i in reversed(range(len(word))):
            for j, t in self.pieces(word, i):
                b[i] = add(b[i], mul(self.w[t], b[j]))
        return b

    def take(self, word, b, i, u):  # the piece drawn at start i by the wide value u -> (j, piece)
        t, cum = mul(u, b[i]), ZERO
        for j, piece in self.pieces(word, i):
            cum = add(cum, mul(self.w[piece], b[j]))
            if gt(cum, t):
                return j, piece  # (always reached: the last cum is b[i], and t < b[i])

    def encode_word(self, word, seed, epoch, s, a0, u=None):  # a0: its first byte in sentence s; u: a wide value in place of every draw
        b = self.backward(word) if len(word) <= self.max_word_chars else [ZERO]
        if b[0] == ZERO:
            return ["[UNK]"]
        out, i, at = [], 0, np.cumsum([0] + [len(c.encode("utf-8", "surrogatepass")) for c in word]).tolist()
        while i < len(word):
            i, piece = self.take(word, b, i, uniform(seed, epoch, s, a0 + at[i]) if u is None else u)
            out.append(piece)
        return out

    def tokenize(self, split, texts, seed=0, epoch=0, first=0):  # the sentence index of texts[j] is first + j
        return [[t for word, a0 in words_of(split, text.lower()) for t in self.encode_word(word, seed, epoch, first + j, a0)]
                for j, text in enumerate(texts)]

    def batch(self, split, texts, seed=0, epoch=0, first=0):  # (ids, offsets, status) as the device must give them
        rows = [[self.ids.get(t, self.unk) for t in row] for row in self.tokenize(split, texts, seed, epoch, first)]
        off = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint64)
        return np.array([i for r in rows for i in r], dtype=np.uint32), off, np.zeros(len(texts), dtype=np.uint8)
