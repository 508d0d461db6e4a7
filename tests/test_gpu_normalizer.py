"""The BERT normalizer on the device (csrc/swt_normalize.hip) against the plain-Python rule of tests/normalizer_cases.py: every code
point, the seams of lanes, tiles and texts, encode_batch of the four classes on both paths, and the label calls."""
import os
import unicodedata

import numpy as np
import pytest

from tests import normalizer_cases as M

pytestmark = pytest.mark.gpu

CLASSES = ["FastBPE", "FastWP", "NaiveBPE", "NaiveWP"]


@pytest.fixture(scope="module")
def dev(native):
    if native.device_count() < 1:
        pytest.fail("no HIP device")
    native.init(0)
    return native


_tokenizers = {}


def _tokenizer(swt, ref_dir, cls):
    if cls not in _tokenizers:
        tok = getattr(swt, cls)()
        tok.load_resources(os.path.join(ref_dir, "resources", "pretrained/FastBPE" if "BPE" in cls else "pretrained/FastWordPiece"))
        _tokenizers[cls] = tok
    _tokenizers[cls].clear_added_tokens()
    _tokenizers[cls].set_normalizer(None)
    return _tokenizers[cls]


def _same(tok, texts, flags, what):
    tok.set_normalizer(flags)
    got, align = tok.normalize_batch(texts, return_alignment=True)
    for i, t in enumerate(texts):
        want, want_align = M.normalize(t, flags)
        assert got[i] == want, (what, i)
        assert np.array_equal(align[i], np.asarray(want_align, dtype=np.int64)), (what, i)


@pytest.mark.parametrize("flags", sorted(M.FLAG_SETS))
def test_every_code_point(swt, dev, ref_dir, flags):
    """U+0001 .. U+10FFFF without the surrogates, 4,096 per text, each between two 'a's: text and alignment are the model's"""
    if dev.lib().swt_unidata_version().decode() != unicodedata.unidata_version:  # the one test that walks the interpreter's tables
        pytest.skip("the tables follow Unicode %s, this interpreter's model %s" % (dev.lib().swt_unidata_version().decode(),
                                                                                  unicodedata.unidata_version))
    texts = ["".join("a" + chr(c) for c in range(max(b, 1), b + 4096) if not 0xD800 <= c <= 0xDFFF) + "a" for b in range(0, 0x110000, 4096)]
    _same(_tokenizer(swt, ref_dir, "FastWP"), texts, M.FLAG_SETS[flags], flags)


@pytest.mark.parametrize("probe", M.PROBES)
def test_seams(swt, dev, ref_dir, probe):
    """a code point that changes length at the sixteen byte positions around a lane's and a tile's boundary, two tiles and a
    remainder behind it; as the last and the first character of neighbouring texts; an empty text, a text that normalises to
    nothing, a text of dropped characters that ends exactly on a tile"""
    tok = _tokenizer(swt, ref_dir, "FastWP")
    tile, lane = dev.normalize_capacity()[:2]
    for flags in ("all", "no_strip"):
        for k in list(range(lane - 8, lane + 8)) + list(range(tile - 8, tile + 8)):
            _same(tok, ["x" * k + probe + "y" * (2100 - k)], M.FLAG_SETS[flags], (flags, k))
        texts = ["z" * (tile - len(probe.encode("utf-8"))) + probe, probe + "tail", "", "\u200b\u00ad", probe]
        room = 2 * tile - sum(len(t.encode("utf-8")) for t in texts) % tile  # dropped characters alone up to a tile's end: U+00AD
        soft = next(m for m in range(3) if (room - 2 * m) % 3 == 0)          # takes two bytes, U+200B three
        texts += ["\u00ad" * soft + "\u200b" * ((room - 2 * soft) // 3), "q\u00ad", "\u200b" * (tile // 3) + "\u0007", "end" + probe]
        assert sum(len(t.encode("utf-8")) for t in texts[:6]) % tile == 0
        _same(tok, texts, M.FLAG_SETS[flags], (flags, "texts"))


def test_ill_formed_bytes_pass_through(dev):
    """an overlong form, a lead without its continuation bytes, 0xF8, a stray continuation byte: copied, and 'É' behind them is 'e'"""
    raw = b"a\xc1\x81b\xe0\x80\x80c\xe2\x82d\xf8e\x80f\xf4\x90\x80\x80g"
    text = np.frombuffer(raw + "É".encode("utf-8") + b"\xe2\x82", dtype=np.uint8)
    out, off, cp_off, src_off, align = dev.normalize(text, np.array([0, 3, text.size], dtype=np.uint64), 15, True)
    assert out.tobytes() == raw + b"e\xe2\x82" and off.tolist() == [0, 3, out.size]
    assert cp_off.tolist() == [0, 2, 14] and src_off.tolist() == [0, 2, 14] and align.tolist() == list(range(14))  # 0x80 is none


@pytest.mark.parametrize("setting", ["all", "no_strip", "no_lower"])
def test_fastwp_gives_the_wheels_ids_and_offsets(swt, dev, ref_dir, golden, setting):
    """FastWP over the vocabulary the golden file was made with, under each recorded setting: ids and offsets are the wheel's (the
    maker says which cases it leaves out: those FastWP refuses with or without a normalizer, as the reference never returns)"""
    g = golden("bert_normalizer.json")
    rec, tok = g["settings"][setting], _tokenizer(swt, ref_dir, "FastWP")
    tok.set_normalizer(rec["flags"])
    for device in (False, True):
        got = _numpy(tok.encode_batch(rec["texts"], return_offsets=True, add_special_tokens=False, device=device))
        for i, (ids, offsets) in enumerate(zip(rec["ids"], rec["offsets"])):
            assert got["attention_mask"][i].sum() == len(ids) and got["input_ids"][i, :len(ids)].tolist() == ids, (setting, device, i)
            assert got["offset_mapping"][i, :len(ids)].tolist() == offsets, (setting, device, i)


def _numpy(res):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in res.items()}


def _texts(golden):
    texts = golden("ref/data/pan_tadeusz.json")[:64] + ["x" * k + p + " yz" for p in M.PROBES for k in (14, 15, 1022)] + ["", "\u200b"]
    models = [M.normalize(t, M.ALL) for t in texts]
    assert all(m[0].lower() == m[0] and "Σ" not in t for m, t in zip(models, texts))  # else the plain call would lowercase further
    return texts, models


def _mapped(want, models, lengths, text_of_row, side_of_row=None):
    """offset_mapping of the plain call over the normalised texts, through the model's alignment"""
    out = want["offset_mapping"].copy()
    for r, c in zip(*np.nonzero(want["word_ids"] >= 0)):
        i = text_of_row(r) + (0 if side_of_row is None else side_of_row(r, c))
        out[r, c] = M.map_span(int(out[r, c, 0]), int(out[r, c, 1]), models[i][1], lengths[i])
    return out


EXTRAS = {"plain": {}, "pairs": {"stride": 3, "max_length": 64, "truncation": "only_second", "return_overflowing": True},
          "packing": {"packing": "whole", "max_length": 48}, "added": {}}


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("cls,extra", [(c, "plain") for c in CLASSES] + [("FastWP", e) for e in ("pairs", "packing", "added")])
def test_encode_batch(swt, dev, ref_dir, golden, cls, extra, device):
    """ids, mask and word ids are those of the plain call over the model-normalised texts, the offsets that call's through the
    model's alignment"""
    tok = _tokenizer(swt, ref_dir, cls)
    texts, models = _texts(golden)
    kw = dict(EXTRAS[extra], return_offsets=extra != "packing")
    if extra == "added":
        tok.add_special_tokens(["[MASK]"])
        texts = ["Zażółć [MASK] gęślą", "jaźń[MASK]", "[mask] Élan 中[MASK]"]
        models = [M.normalize(t, M.ALL) for t in texts]
    if cls == "NaiveWP":  # the reference's loop never ends on a character its vocabulary lacks, with or without a normalizer:
        keep = [i for i, t in enumerate(texts) if not set(t) & set("한中𝐀")]  # those three stay with the classes that return
        texts, models = [texts[i] for i in keep], [models[i] for i in keep]
    n = len(texts)
    if extra == "pairs":  # fewer and shorter texts: the first side is spared and has to leave the second room
        keep = list(range(12)) + [i for i in range(64, len(texts)) if len(texts[i]) < 100]
        texts, models = [texts[i] for i in keep], [models[i] for i in keep]
        n = len(texts)
        kw["text_pairs"] = texts[::-1]
        models = models + models[::-1]
    normalised = [m[0] for m in models]
    want = tok.encode_batch(normalised[:n], **dict(kw, **({"text_pairs": normalised[n:]} if extra == "pairs" else {})))
    assert "offset_unit" not in want  # without a normalizer the result's keys are what they were
    tok.set_normalizer("bert")
    got = _numpy(tok.encode_batch(texts, device=device, **kw))
    for k in ("input_ids", "attention_mask") + (("word_ids",) if extra != "packing" else ("sample_ids", "position_ids")):
        assert np.array_equal(got[k], want[k]), (cls, extra, k)
    if extra != "packing":
        assert got["offset_unit"] == "original"
        lengths = [len(t) for t in texts] + [len(t) for t in texts[::-1]]
        sample = want.get("overflow_to_sample_mapping", np.arange(len(want["input_ids"])))
        side = (lambda r, c: n * int(want["sequence_ids"][r, c])) if extra == "pairs" else None
        assert np.array_equal(got["offset_mapping"], _mapped(want, models, lengths, lambda r: int(sample[r]), side)), (cls, extra)


def test_labels_in_the_original_string(swt, dev, ref_dir):
    """answer_positions takes and best_answers returns character spans of the text as given; "text" is texts[i][a:b]"""
    tok = _tokenizer(swt, ref_dir, "FastWP")
    context = "Gęślą jaźń \u200b\u200bİ中 Zażółć koniec"
    a = context.index("Zażółć")
    e = a + len("Zażółć")
    tok.set_normalizer("bert")  # before the answer the ideograph gains two spaces and two code points vanish... and one more
    context = "\u00ad" + context
    a, e = a + 1, e + 1
    assert len(M.normalize(context, M.ALL)[0]) != len(context) and M.normalize(context, M.ALL)[1][a - 1] != a - 1
    batch = tok.encode_batch([context], return_offsets=True)
    pos = tok.answer_positions(batch, [(a, e)], texts=[context])
    start, end = int(pos["start_positions"][0]), int(pos["end_positions"][0])
    assert pos["n_with"] == 1 and batch["offset_mapping"][0, start, 0] == a and batch["offset_mapping"][0, end, 1] == e
    logits = np.zeros((2,) + batch["input_ids"].shape, dtype=np.float32)
    logits[0, 0, start] = logits[1, 0, end] = 9.0
    best = tok.best_answers(batch, logits[0], logits[1], texts=[context])
    assert (int(best["char_start"][0]), int(best["char_end"][0])) == (a, e) and best["text"] == [context[a:e]]
