"""The model of tests/sample_cases.py against exact arithmetic: the piece it takes is the one whose exact interval holds u."""
from fractions import Fraction
from itertools import accumulate

import numpy as np
import pytest

from tests import sample_cases as S

WEIGHTS = dict(zip(sorted(S.HANDMADE), np.random.RandomState(6).dirichlet(np.ones(len(S.HANDMADE))).astype(np.float32)))
GRID = [(k * (1 << 18) + 77777) | 1 for k in range(64)]  # (non-dyadic weights; odd multiples of 2^-24 spread over (0, 1))
# each of the at most 2n = 16 roundings behind a b is off by at most 2^-24 of it, and two such values are compared: 2^-19, and
# 2^-18 leaves a factor of two for the roundings of t and of the running sum
MARGIN = Fraction(1, 1 << 18)


def exact_sums(model, word, weight):
    b = [Fraction(0)] * len(word) + [Fraction(1)]
    for i in reversed(range(len(word))):
        b[i] = sum((weight[t] * b[j] for j, t in model.pieces(word, i)), Fraction(0))
    return b


def test_the_piece_taken_is_the_one_whose_exact_interval_holds_u():
    model, weight = S.Model(S.HANDMADE, WEIGHTS), {t: Fraction(float(w)) for t, w in WEIGHTS.items()}
    seen = skipped = 0
    for word in [w for w in S.WORDS if len(w) <= 8]:
        b, exact = model.backward(word), exact_sums(model, word, weight)
        assert [x == S.ZERO for x in b] == [x == 0 for x in exact]
        for i in [i for i in range(len(word)) if exact[i]]:
            pieces = model.pieces(word, i)
            ends = list(accumulate(weight[t] * exact[j] / exact[i] for j, t in pieces))
            for g in GRID:
                u = Fraction(g, 1 << 24)
                seen += 1
                if any(abs(u - end) < MARGIN for end in ends[:-1]):
                    skipped += 1
                    continue
                assert model.take(word, b, i, S.rne(g, -24)) == pieces[sum(u >= end for end in ends[:-1])], (word, i, g)
    assert seen >= 64 * 30 and skipped * 100 <= seen, (seen, skipped)


def test_the_exponent_has_no_bound():
    model = S.Model(S.HANDMADE, {t: 2.0 ** -64 for t in S.HANDMADE})
    exact = exact_sums(model, "x" * 100, {t: Fraction(2) ** -64 for t in S.HANDMADE})
    m, e = model.backward("x" * 100)[0]
    assert m * Fraction(2) ** e == exact[0] == Fraction(2) ** -6400


@pytest.mark.parametrize("g", [0, 1, 1 << 23, (1 << 24) - 1])
def test_one_segmentation_and_none(g):
    model, u = S.Model(S.HANDMADE, WEIGHTS), S.rne(g, -24)
    assert model.encode_word("xxxx", 0, 0, 0, 0, u) == ["x", "##x", "##x", "##x"]
    assert model.encode_word("€€ż", 0, 0, 0, 0, u) == ["€", "##€ż"]
    assert model.encode_word("xq", 0, 0, 0, 0, u) == model.encode_word("abcdx" * 21, 0, 0, 0, 0, u) == ["[UNK]"]
