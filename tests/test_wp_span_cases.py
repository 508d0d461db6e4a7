"""The Python model of the FastWP walk with positions (tests/wp_span_cases.py) against the reference's own answers
(tests/golden/fastwp_spans.json, made by tests/golden/make_golden_fastwp_spans.py from the imported reference) and against the C
oracle's FastWP ids.  No GPU: tests/test_gpu_fastwp_spans.py then holds the device to this model."""
import functools

import numpy as np
import pytest

from tests.test_gpu_wp_seams import CAP, DIRECT_BYTES, DIRECT_SENTS, TILE, handmade_vocab
from tests.wp_span_cases import WP_OK, WpSpanModel, seam_batches


@functools.lru_cache(maxsize=None)
def pretrained_model():
    from subword_tokenizers_amd import synth

    return WpSpanModel(synth.pretrained_vocab())


def fixture_parts(golden, corpora):
    """[(part, model, [(text, row)])]"""
    fx = golden("fastwp_spans.json")
    pan = corpora["pan"][:fx["pan"]["n"]]
    assert len(fx["pan"]["rows"]) == len(pan)
    return [("pan", pretrained_model(), list(zip(pan, fx["pan"]["rows"]))),
            ("fuzz", WpSpanModel(fx["fuzz"]["vocab"]), [(r["text"], r) for r in fx["fuzz"]["rows"]])]


def test_fixture_holds_what_it_is_for(golden):
    fz = golden("fastwp_spans.json")["fuzz"]
    assert len(fz["rows"]) >= 400 and fz["dropped"] * 10 <= len(fz["rows"]) + fz["dropped"]
    for need in ("unk", "short_cover", "corner", "empty_leading", "unk_behind_boundary"):
        assert fz["counts"][need] > 0, need
    row = {r["text"]: r for r in fz["rows"]}
    assert row["x-yq"]["tokens"] == ["['UNK']"] and row["x-yq"]["spans"] == [0, 4]
    assert row["a. "]["tokens"] == ["a"] and row["a. "]["spans"] == [0, 1]  # nothing covers the '.'
    assert row["ab##ing"]["tokens"][-1] == "##ing" and row["ab##ing"]["spans"][-2:] == [2, 7]  # the literal text covers five
    assert row[" a"]["word"] == [0]  # the empty leading segment is not counted


def test_model_reproduces_every_fixture_row(golden, corpora):
    for part, model, rows in fixture_parts(golden, corpora):
        for text, row in rows:
            ids, spans, word, status = model.sentence(text.lower())
            assert status == WP_OK, (part, text)
            toks, sp, wd = model.rows(ids, spans, word)
            assert toks == row["tokens"], (part, text)
            assert sp == row["spans"], (part, text)
            assert wd == row["word"], (part, text)


def test_model_ids_are_the_oracles_on_the_fixture(golden, corpora, oracle):
    for part, model, rows in fixture_parts(golden, corpora):
        orc = oracle.OracleWP(model.tokens)
        texts = [t for t, _ in rows]
        want = orc.tokenize_batch_ids(texts)
        got = model.batch([t.lower() for t in texts])
        assert len(model.corner or [0]) == 1  # no multi-token corner here: ids compare one to one
        assert np.array_equal(got[2], want[2]) and np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0]), part


def test_model_ids_are_the_oracles_on_the_seams(oracle):
    model = WpSpanModel(handmade_vocab())
    orc = oracle.OracleWP(model.tokens)
    total = 0
    for name, sents in seam_batches(CAP, TILE, DIRECT_BYTES, DIRECT_SENTS):
        want = orc.tokenize_batch_ids(sents)
        got = model.batch(sents)
        assert np.array_equal(got[2], want[2]) and np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0]), name
        total += sum(len(s.encode("utf-8")) for s in sents)
        # byte spans and code-point spans tell the same story
        assert np.all(got[3][:, 0] <= got[3][:, 1]) and np.all(got[4][:, 0] <= got[4][:, 1])
    assert total < 1 << 20, total


def test_model_refuses_what_the_reference_does_not_return_from():
    """the statuses, which no fixture row can hold: a character the root has no edge for behind punctuation never moves on, and
    the '##' corner of a vocabulary with '#' but no '##' never ends"""
    model = WpSpanModel(["a", "##a", ".", "#"])  # sorted: '#', '##a', '.', 'a'
    assert model.corner is None
    assert model.sentence("a .z")[3] != WP_OK
    assert model.sentence("a ##")[3] != WP_OK
    assert model.sentence("aa a.")[:3] == ([3, 1, 3, 2], [(0, 1), (1, 2), (3, 4), (4, 5)], [0, 0, 1, 2])
