"""The model of tests/prune_cases.py on words worked by hand, the exports, and what prune and train_unigram refuse (no GPU)."""
import numpy as np
import pytest

from tests import prune_cases as P

SCORES, ONE = dict({t: -1.0 for t in P.HANDMADE}, **{"##bcd": -4.0}), P.UNIT


@pytest.mark.parametrize("word,max_word_chars,want", [
    ("abx", 100, (-2 * ONE, ["ab", "##x"], {"ab": ONE, "##x": None})),  # a ##b ##x is a piece longer; nothing else ends the word
    ("xxxx", 100, (-4 * ONE, ["x", "##x", "##x", "##x"], {"x": None, "##x": None})),  # three times on the path, barred once
    # "##b" stands on the path at (2, 3) and off it at (1, 2): barred at both, ab ##bcd is left (a ##b ##bcd is not)
    ("abbcd", 100, (-3 * ONE, ["ab", "##b", "##cd"], {"ab": ONE, "##b": 2 * ONE, "##cd": ONE})),
    # ab ##cd and abc ##d tie and the longer last piece stays: each of its pieces goes at no loss
    ("abcd", 100, (-2 * ONE, ["ab", "##cd"], {"ab": 0, "##cd": 0})),
    ("abcd", 4, (-2 * ONE, ["ab", "##cd"], {"ab": 0, "##cd": 0})),
    ("abcde", 4, None), ("xq", 100, None),
])
def test_words_worked_by_hand(word, max_word_chars, want):
    assert P.Prune(P.HANDMADE, SCORES, max_word_chars).word(word) == want


def test_the_fixed_point():
    inf, f = np.float32("inf"), np.float32
    assert (P.ufix(inf, inf), P.ufix(-inf, -inf), P.ufix(f(1), -inf), P.ufix(f(2.0 ** 30), f(0))) == (0, 0, P.CLAMP, P.CLAMP)
    assert (P.ufix(f(1.5), f(1.5 - 2.0 ** -21)), P.ufix(f(0.0), f(-0.0)), P.ufix(f(3.0), f(-0.75))) == (0, 0, 3 * ONE + 3 * ONE // 4)
    assert (P.fix(f(-1.5 - 2.0 ** -21)), P.fix(f(2.0 ** -21)), P.fix(inf), P.fix(f(-3e38))) == (-ONE - ONE // 2, 0, P.CLAMP, -P.CLAMP)


def test_the_exports_and_what_is_refused(swt, native):
    assert {"swt_wp_removal_losses", "swt_wp_removal_losses_dev"} <= set(native.SIGNATURES) and hasattr(native.WpTrie, "removal_losses_dev")
    for name in ("removal_losses", "prune", "train_unigram"):
        assert hasattr(swt.UnigramWP, name) and not hasattr(swt.NaiveWP, name) and not hasattr(swt.FastWP, name)
    tok = swt.UnigramWP()
    tok.vocab = set(P.HANDMADE) | {"[UNK]"}
    tokens, size = sorted(tok.vocab), len(tok.vocab)
    losses = {"loss": np.array([{"ab": 3.0, "abc": 1.0, "##cd": 1.0}.get(t, 0.0) for t in tokens]),
              "counts": np.array([int(t == "##cd") for t in tokens]), "orphaned": np.array([int(t == "##cde") for t in tokens])}
    with pytest.raises(ValueError):
        tok.prune([], 10, losses)  # (no scores yet)
    tok.set_scores(dict(SCORES, **{"[UNK]": -1.0}))
    for bad in (0, 2.5, True, 10):  # (10: with the figures of another vocabulary)
        with pytest.raises(ValueError):
            tok.prune([], bad, losses if bad != 10 else {k: v[1:] for k, v in losses.items()})
    many = {t for t in tokens if len(t) > 1 and not (len(t) == 3 and t[:2] == "##") and t != "[UNK]"}
    # the 14 of one code point, [UNK] and the orphaning "##cde" stay whatever the target; then by loss, count, token
    assert len(many) == 10 and tok.prune([], size - 10 + 3, losses) == sorted(many - {"##cde", "ab", "##cd"})
    assert len(tok.vocab) == size - 7 == len(tok.scores()) and {"ab", "##cd", "##cde"} <= tok.vocab and tok._naive_trie is None
    keep = [k for k, t in enumerate(tokens) if t in tok.vocab]
    assert tok.prune([], 1, {k: v[keep] for k, v in losses.items()}) == ["##cd", "ab"]  # below the mandatory set: exactly it stays
    for kwargs in ({"max_vocab": 0}, {"seed_factor": 0}, {"shrink": 1.0}, {"shrink": 0.0}, {"iterations": 0}, {"alpha": 0.0}, {"method": "medium"},
                   {"corpus": "ab"}, {"seed_vocab": "ab"}):
        with pytest.raises(TypeError if set(kwargs) & {"corpus", "seed_vocab"} else ValueError):
            tok.train_unigram(**dict({"corpus": ["ab"], "max_vocab": 10}, **kwargs))
