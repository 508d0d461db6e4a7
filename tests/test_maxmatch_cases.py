"""The plain-Python model of MaxMatch-Dropout (tests/maxmatch_cases.py; the rule: include/swt.h, swt_wp_encode_naive_dropout)
held, without a GPU, to its two end points, to its nominal drop rate, to its own recorded answers
(tests/golden/maxmatch_dropout.json), to what makes it usable per epoch and to the outcomes that depend on the draw; and what the
Python layer refuses before any device call."""
import json
import math

import pytest

from tests import maxmatch_cases as M
from tests.test_dropout_cases import BAD, make
from tests.test_gpu_wp_seams import handmade_vocab
from tests.test_naive_wp_encode import MaxMatch, naivewp_cases


@pytest.fixture(scope="module")
def split(swt):
    return swt.SubwordTokenizer._split


@pytest.fixture(scope="module")
def fixture_cases():
    return {name: (vocab, texts, tokens) for name, vocab, texts, tokens in naivewp_cases()}


@pytest.fixture(scope="module")
def pan(fixture_cases):
    vocab, texts, tokens = fixture_cases["pan_tadeusz_pretrained"]
    return M.Model(vocab), texts, tokens


def test_no_drop_is_the_recorded_naive_wp(pan, split):
    model, texts, tokens = pan
    assert len(texts) == len(tokens) == 989
    got = model.tokenize(split, texts, 0, seed=5, epoch=9)
    assert got == tokens and sum(map(len, got)) == 29164


def test_no_drop_is_max_match_on_every_fixture_vocabulary(fixture_cases, split):
    """drop_below = 0 is the plain walk on any vocabulary, where it never returns included"""
    for name, (vocab, texts, tokens) in fixture_cases.items():
        got = M.Model(vocab).tokenize(split, texts, 0, seed=3)
        assert [g if g is not None else "TIMEOUT" for g in got] == tokens, name
    hand = handmade_vocab()
    texts = M.short_sentences(40, 3000, seed=3)
    plain = MaxMatch(hand)
    assert M.Model(hand).tokenize(split, texts, 0) == [plain.tokenize(t, lambda s: [w for w, _ in split(s.lower())]) for t in texts]


def test_all_dropped_is_the_characters(pan, split):
    model, texts, _ = pan
    got = model.tokenize(split, texts, M.ONE, seed=1)
    assert got == M.characters(split, texts) and sum(map(len, got)) == 36499
    assert [M.spelled(row) for row in got] == ["".join(w for w, _ in split(t.lower())) for t in texts]


def test_drop_rate(pan, split):
    """the share of the candidates with c >= 2 dropped at p = 0.1, within four binomial standard deviations"""
    model, texts, _ = pan
    stats = {"looked": 0, "dropped": 0}
    got = model.tokenize(split, texts, M.drop_below(0.1), seed=2024, epoch=1, stats=stats)
    n, p = stats["looked"], M.drop_below(0.1) / M.ONE
    bound = 4.0 * math.sqrt(p * (1.0 - p) / n)
    share = stats["dropped"] / n
    print("candidates with c >= 2 looked at %d, dropped %d, share %.5f, bound +- %.5f, tokens %d" % (
        n, stats["dropped"], share, bound, sum(map(len, got))))
    assert n > 5000
    assert abs(share - p) <= bound
    assert not any(row is None or "[UNK]" in row for row in got)
    # with and without the count the walk is the same one
    assert got == model.tokenize(split, texts, M.drop_below(0.1), seed=2024, epoch=1)


def test_epochs_differ_and_a_draw_repeats(pan, split):
    model, texts, tokens = pan
    texts, plain, below = texts[:60], tokens[:60], M.drop_below(0.1)
    a = model.tokenize(split, texts, below, seed=7, epoch=0)
    assert a == model.tokenize(split, texts, below, seed=7, epoch=0)
    b = model.tokenize(split, texts, below, seed=7, epoch=1)
    c = model.tokenize(split, texts, below, seed=8, epoch=0)
    assert a != b and a != c and b != c and a != plain
    # the sentence index is part of the key: the same text at another place in the batch draws anew, and by `first` the same
    assert model.tokenize(split, texts[10:20], below, seed=7, first=10) == a[10:20]
    assert model.tokenize(split, texts[10:20], below, seed=7) != a[10:20]
    # every segmentation spells its text
    for row, ref in zip(a, plain):
        assert "[UNK]" not in row and M.spelled(row) == M.spelled(ref)


def test_fuzz_keeps_its_non_terminating_sentences(fixture_cases, split):
    vocab, texts, tokens = fixture_cases["fuzz_pretrained"]
    got = M.Model(vocab).tokenize(split, texts, M.drop_below(0.3), seed=1, epoch=1)
    assert [g is None for g in got] == [t == "TIMEOUT" for t in tokens] and sum(g is None for g in got) == 30


def test_the_status_can_depend_on_the_draw(split):
    texts, below = ["abc"] * 40, M.drop_below(0.5)
    loop = M.Model(M.MICRO_LOOP).tokenize(split, texts, below)
    unk = M.Model(M.MICRO_UNK).tokenize(split, texts, below)
    for i in range(40):
        gone = M.dropped(2, 1, i, 0, 0, below)  # "##bc" takes two code points from byte 1 of sentence i
        assert loop[i] == (None if gone else ["a", "##bc"])
        assert unk[i] == (["[UNK]"] if gone else ["a", "##bc"])
    kinds = {json.dumps(x) for x in loop + unk}
    assert kinds == {"null", '["[UNK]"]', '["a", "##bc"]'}


def test_unk_discards_stored_pieces(fixture_cases, split):
    vocab, texts, tokens = fixture_cases["unk_after_first_piece"]
    model = M.Model(vocab)
    assert model.tokenize(split, ["unaffab"] * 8, M.drop_below(0.5)) == [["[UNK]"]] * 8  # nothing matches "##ab": any draw
    # "unaffable" is un ##aff ##able; with "##able" dropped and the two before it alive, two stored pieces go for one "[UNK]"
    below = M.drop_below(0.5)
    got = model.tokenize(split, ["unaffable"] * 40, below, seed=11)
    late = [i for i in range(40) if not M.dropped(2, 0, i, 0, 11, below) and not M.dropped(3, 2, i, 0, 11, below)
            and M.dropped(4, 5, i, 0, 11, below)]
    assert late and all(got[i] == ["[UNK]"] for i in late)
    assert ["un", "##aff", "##able"] in got


def test_recorded_answers(pan, split, golden):
    model, texts, _ = pan
    rec = golden("maxmatch_dropout.json")
    rows = [texts[r] for r in rec["rows"]]
    assert len(rows) == 20 and len(rec["cases"]) == 3
    for case in rec["cases"]:
        assert case["drop_below"] == M.drop_below(case["probability"])
        assert model.tokenize(split, rows, case["drop_below"], case["seed"], case["epoch"]) == case["tokens"]
    assert len({json.dumps(c["tokens"]) for c in rec["cases"]}) == 3


# ---- what the Python layer refuses (no device call is reached)
@pytest.mark.parametrize("bad", BAD, ids=[json.dumps(b) for b in BAD])
def test_naive_wp_refuses_a_bad_maxmatch_dropout(swt, bad):
    tok = make(swt, "NaiveWP")
    for call in (lambda: tok.encode_ids_batch(["ab"], maxmatch_dropout=bad), lambda: tok.tokenize_batch(["ab"], maxmatch_dropout=bad),
                 lambda: tok.tokenize("ab", maxmatch_dropout=bad), lambda: tok.encode_batch(["ab"], maxmatch_dropout=bad)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(TypeError):
        tok.encode_ids_batch(["ab"], maxmatch_dropout=0.1)
    with pytest.raises(TypeError):
        tok.encode_batch(["ab"], maxmatch_dropout=0.1)


@pytest.mark.parametrize("cls", ["NaiveBPE", "FastBPE", "FastWP"])
def test_the_other_classes_refuse_maxmatch_dropout(swt, cls):
    tok = make(swt, cls)
    spec = {"probability": 0.1}
    for call in (lambda: tok.encode_ids_batch(["ab"], maxmatch_dropout=spec), lambda: tok.tokenize_batch(["ab"], maxmatch_dropout=spec),
                 lambda: tok.encode_batch(["ab"], maxmatch_dropout=spec)):
        with pytest.raises(ValueError, match="NaiveWP"):
            call()


def test_dropout_stays_fast_bpes_on_naive_wp(swt):
    tok = make(swt, "NaiveWP")
    with pytest.raises(ValueError, match="FastBPE"):
        tok.encode_ids_batch(["ab"], dropout={"probability": 0.1}, maxmatch_dropout={"probability": 0.1})


def test_abi_exports(native):
    lib = native.lib()
    assert callable(lib.swt_wp_encode_naive_dropout) and callable(lib.swt_wp_encode_naive_dropout_dev)
