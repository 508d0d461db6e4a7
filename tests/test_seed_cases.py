"""The model of tests/seed_cases.py against a recount by hand, the exports, and what seed_substrings and train_unigram refuse (no GPU)."""
import inspect

import pytest

from tests import seed_cases as S

WORDS = [("aaaa", 3), ("abab", 2), ("xab", 5)]


def test_the_model_against_a_recount():
    got = S.census(WORDS, 3)
    for flag, piece in {(flag, w[i:i + n]) for w, _ in WORDS for i in range(len(w)) for n in (2, 3) if i + n <= len(w) for flag in (False, True)}:
        recount = sum(f * sum(w.startswith(piece, i) for i in range(len(w)) if (i > 0) == flag) for w, f in WORDS)
        assert got.get((flag, tuple(map(ord, piece))), 0) == recount, (flag, piece)
    assert got[(True, (97, 97))] == 6 and got[(False, (97, 97))] == 3 and got[(True, (97, 98))] == 7 and (False, (97,)) not in got
    assert S.census(WORDS, 3, 7) == {(True, (97, 98)): 7} and S.census(WORDS, 3, 1, 3) == S.census(WORDS[2:], 3)
    ranked = sorted({(False, (97, 98)): 4, (True, (97, 98)): 4, (False, (97, 98, 99)): 3, (False, (120, 121)): 5}.items(), key=S.seed_order)
    assert [S.token(key) for key, _ in ranked] == ["xy", "abc", "##ab", "ab"]


def outcome(call):
    try:
        call()
        return None
    except Exception as e:  # noqa: BLE001  (the kind of failure is what is compared)
        return type(e)


def test_the_exports_and_what_is_refused(swt, native):
    names = {"swt_substring_counts", "swt_substring_counts_dev", "swt_substring_counts_text_dev", "swt_substring_counts_capacity"}
    assert names <= set(native.SIGNATURES) and native.substring_counts_capacity() == (1024, 31, 32)
    assert hasattr(swt.UnigramWP, "seed_substrings") and not hasattr(swt.NaiveWP, "seed_substrings") and not hasattr(swt.FastWP, "seed_substrings")
    assert list(inspect.signature(swt.UnigramWP.train_unigram).parameters)[-1] == "seed"
    tok = swt.UnigramWP()
    for kwargs in ({"size": 0}, {"size": 2.5}, {"size": True}, {"max_piece_chars": 1}, {"max_piece_chars": 33}, {"min_count": 0}, {"corpus": "ab"},
                   {"corpus": [b"ab"]}):
        with pytest.raises(TypeError if "corpus" in kwargs else ValueError):
            tok.seed_substrings(**dict({"corpus": ["ab"], "size": 10}, **kwargs))
    for kwargs in ({"seed": "suffixes"}, {"seed": None}, {"seed": "substrings", "seed_vocab": ["a"]}, {"seed": "substrings", "max_vocab": 0}):
        with pytest.raises(ValueError):
            tok.train_unigram(**dict({"corpus": ["ab"], "max_vocab": 10}, **kwargs))
    # seed="merges" is the call without the keyword: the same end with and without a device
    assert outcome(lambda: tok.train_unigram(["ab ab"], 10, seed="merges")) == outcome(lambda: tok.train_unigram(["ab ab"], 10))
    if not native.device_count():  # no device: a loud failure, not a host-side count
        assert outcome(lambda: tok.seed_substrings(["ab ab"], 10)) is not None
