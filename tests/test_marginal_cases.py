"""The model of tests/marginal_cases.py against exact arithmetic: every fixed-point count lies within its roundings of the exact
posterior, the bitwise logarithm within its stated interval of log2."""
import math
from fractions import Fraction

import numpy as np

from tests import marginal_cases as M
from tests.test_sample_cases import WEIGHTS, exact_sums

SHORT = [w for w in M.WORDS if len(w) <= 8]
U, FLOOR = Fraction(1, 1 << 24), Fraction(1, 1 << 32)


def bound(n):
    """Roundings on the longest chain behind a count of a word of n code points, one relative 2^-24 each.  a[j] is a sum of at most
    j products of an a[i], i < j: a product and at most j - 1 additions (the first lands on 0, exactly) on top of the chain of
    a[j - 1], so at most j(j+1)/2; b[i] the same with n - i for j.  p chains a[i], b[j] and b[0] -- i + (n - j) < n, so the first
    two hold n(n+1)/2 together and b[0] as many -- with the two products and the quotient; the floor costs one unit of 2^-32."""
    return (n * (n + 1) + 3) * U


def exact_forward(model, word, weight):
    a = [Fraction(1)] + [Fraction(0)] * len(word)
    for i in range(len(word)):
        for j, t in model.pieces(word, i):
            a[j] += a[i] * weight[t]
    return a


def test_counts_lie_within_their_roundings_of_the_exact_posterior():
    model, weight = M.Marginal(M.HANDMADE, WEIGHTS), {t: Fraction(float(w)) for t, w in WEIGHTS.items()}
    seen = 0
    for word in SHORT:
        got, n = model.lattice(word), len(word)
        b, a = exact_sums(model, word, weight), exact_forward(model, word, weight)
        assert (got is None) == (b[0] == 0), word
        if got is None:
            continue
        want = {(i, j): a[i] * weight[t] * b[j] / b[0] for i in range(n) for j, t in model.pieces(word, i) if a[i] and b[j]}
        assert [(i, j) for i, j, _, _ in got[0]] == sorted(want), word
        for i, j, _, q in got[0]:
            assert abs(q * FLOOR - want[i, j]) <= bound(n) * want[i, j] + FLOOR, (word, i, j)
        assert abs(sum(q for _, j, _, q in got[0] if j == n) * FLOOR - 1) <= bound(n) + FLOOR, word
        seen += len(got[0])
    assert seen >= 40


def test_the_bitwise_logarithm():
    rng = np.random.RandomState(7)
    for m in [1 << 23, (1 << 23) + 1, (1 << 24) - 1] + rng.randint(1 << 23, 1 << 24, 4000).tolist():
        assert -1.02 * 2.0 ** -24 <= M.frac24(m) * 2.0 ** -24 - math.log2(m * 2.0 ** -23) <= 0, m
    assert M.frac24(1 << 23) == 0 and M.div(M.rne(3, 5), M.rne(3, -7)) == M.ONE[:1] + (12 - 23,)


def test_an_unreached_start_and_a_dead_end():
    model = M.Marginal(["ab", "##b", "##c"], {t: 0.5 for t in ["ab", "##b", "##c"]})
    assert model.backward("abc")[1] != M.ZERO  # "##b ##c" leads to the end from 1, but nothing leads to 1: "##b" counts nothing
    assert model.expected("abc")[0] == [(model.ids["ab"], 1 << 32), (model.ids["##c"], 1 << 32)]
    model, word = M.Marginal(M.HANDMADE, WEIGHTS), "\U0001F600\U0001F600a"
    assert model.backward(word)[2] == M.ZERO  # "##\U0001F600" ends at 2, where nothing goes on: it is visited and counts nothing
    assert [(piece, q) for _, _, piece, q in model.lattice(word)[0]] == [("\U0001F600", 1 << 32), ("##\U0001F600a", 1 << 32)]
    assert model.expected("xq") is None and M.Marginal(M.HANDMADE, WEIGHTS, 4).expected("abcde") is None
