"""The project's own model of UnigramWP's expected counts (include/swt.h, swt_wp_expected_counts) in plain Python integers: the wide
float32 of tests/sample_cases.py with its division, the fixed-point count and the bitwise logarithm."""
import numpy as np

from tests.sample_cases import HANDMADE, ONE, WORDS, ZERO, Model, add, mul, rne, weights, wide, words_of  # noqa: F401  (and for the tests)


def div(a, b):  # of non-zero values; the remainder travels as a sticky bit below the quotient, so rne rounds the exact quotient
    q, r = divmod(a[0] << 26, b[0])
    return rne(q << 1 | (r != 0), a[1] - b[1] - 27)


def frac24(m):  # the 24 bits behind the point of log2(m * 2^-23), 2^23 <= m < 2^24, rounded down bit by bit
    m, bits = m << 7, 0
    for _ in range(24):
        m = (m * m) >> 30
        bits, m = (bits << 1) | (m >> 31), m >> (m >> 31)
    return bits


def fixed(p):  # q of the rule: floor(p * 2^32), at most 2^32
    return min(p[0] << (p[1] + 32) if p[1] >= -32 else p[0] >> -(p[1] + 32), 1 << 32)


class Marginal(Model):
    def lattice(self, word):  # -> ([(i, j, piece, q)] in the order of the visits, L), or None for an UNK word
        n = len(word)
        b = self.backward(word) if n <= self.max_word_chars else [ZERO]
        if b[0] == ZERO:
            return None
        a, out = [ONE] + [ZERO] * n, []
        for i in range(n):
            for j, piece in self.pieces(word, i) if a[i] != ZERO else []:  # (an unreached start is skipped)
                term = mul(a[i], self.w[piece])
                a[j] = add(a[j], term)
                if b[j] != ZERO:
                    out.append((i, j, piece, fixed(div(mul(term, b[j]), b[0]))))
        return out, ((b[0][1] + 23) << 24) + frac24(b[0][0])

    def expected(self, word):  # -> ([(id, q)], L) or None
        got = self.lattice(word)
        return got and ([(self.ids[piece], q) for _, _, piece, q in got[0]], got[1])

    def batch(self, split, texts):  # (counts uint64[n_vocab], stats int64[3]) as the device must give them
        counts, stats, seen = [0] * len(self.ids), [0, 0, 0], {}
        for text in texts:
            for word, _ in words_of(split, text.lower()):
                got = seen[word] if word in seen else seen.setdefault(word, self.expected(word))
                if got is None:
                    stats[1] += 1
                    continue
                for k, q in got[0]:
                    counts[k] += q
                stats[0], stats[2] = stats[0] + 1, stats[2] + got[1]
        return np.array(counts, dtype=np.uint64), np.array(stats, dtype=np.int64)
