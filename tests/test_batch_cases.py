"""Model-ready batches without a GPU: the Python model of tests/batch_cases.py against what the `tokenizers` wheel recorded
(tests/golden/model_batches.json), the dense vocabularies of the four classes, and the argument checks the host forms of
swt_batch_plan / swt_batch_rows make before anything touches a device."""
import ctypes as C
import os

import numpy as np
import pytest

from . import batch_cases as B


@pytest.fixture(scope="module")
def recorded(golden):
    return golden("model_batches.json")


def _spec_of(g, width, stride, cls, sep, left, windows):
    i = g["ids"]
    return B.spec(width, stride, windows, bool(left), False, i["pad"], i["unk"], i["cls"] if cls else None, i["sep"] if sep else None)


def _slots(text, width):
    """the fixture's one character per slot -> (ids int32[rows, width], mask uint8[rows, width])"""
    code = np.frombuffer(text.encode("ascii"), dtype=np.uint8).astype(np.int32).reshape(-1, width)
    mask = code < 80
    return np.where(mask, code - 40, code - 80).astype(np.int32), mask.astype(np.uint8)


def test_model_equals_the_recorded_cases(recorded):
    """every recorded case, windowed (the encoding and its overflowing encodings) and truncating (the encoding alone)"""
    first = recorded["ids"]["first"]
    seen = set()
    for key, by_n in recorded["cases"].items():
        width, stride, cls, sep, left = (int(x) for x in key.split(","))
        assert len(by_n) == 21
        for n, text in enumerate(by_n):
            seen.add((width, stride, cls, sep, left, n))
            rows = [[first + i for i in range(n)]]
            want_ids, want_mask = _slots(text, width)
            got = B.expected_batch(rows, _spec_of(recorded, width, stride, cls, sep, left, True))
            assert np.array_equal(got["input_ids"], want_ids), (key, n)
            assert np.array_equal(got["attention_mask"], want_mask), (key, n)
            assert np.array_equal(got["length"], want_mask.sum(axis=1))
            assert got["row_base"].tolist() == [0, want_ids.shape[0]] and got["lost"] == 0
            cut = B.expected_batch(rows, _spec_of(recorded, width, stride, cls, sep, left, False))
            assert np.array_equal(cut["input_ids"], want_ids[:1]) and np.array_equal(cut["attention_mask"], want_mask[:1])
            assert cut["lost"] == (want_ids.shape[0] > 1)
    # the grid the fixture promises
    want = {(w, s, c, p, l, n) for w in (3, 4, 5, 8) for c in (0, 1) for p in (0, 1) for s in range(w - c - p) for l in (0, 1) for n in range(21)}
    assert seen == want and len(want) == 2688


def test_model_equals_the_recorded_batch(recorded):
    b, first = recorded["batch"], recorded["ids"]["first"]
    rows = [[first + i for i in range(n)] for n in b["lengths"]]
    got = B.expected_batch(rows, _spec_of(recorded, b["width"], b["stride"], b["cls"], b["sep"], b["left"], True))
    want_ids, want_mask = _slots(b["slots"], b["width"])
    assert np.array_equal(got["input_ids"], want_ids) and np.array_equal(got["attention_mask"], want_mask)
    assert got["sample"].tolist() == b["sample"]
    assert [int(got["row_base"][i]) for i in range(len(rows))] == [b["sample"].index(i) for i in range(len(rows))]


def test_model_dense_ids_and_payloads():
    cmap = np.array([5, 6, B.NONE, 7, 15, 16, 17, B.NONE], dtype=np.uint32)  # n_map 4, flagged
    rows = [[0, 1 | B.CONT, 2, 3 | B.CONT, 4, 0 | B.CONT]]
    pay = ([[(i, i + 1) for i in range(6)]], [[i // 2 for i in range(6)]])
    got = B.expected_batch(rows, B.spec(8, cls_id=2, pad_id=9, unk_id=1), (cmap, 4, True), pay)
    assert got["input_ids"].tolist() == [[2, 5, 16, 1, 1, 1, 15, 9]]
    assert got["n_unknown"] == 3 and got["word_ids"].tolist() == [[-1, 0, 0, 1, 1, 2, 2, -1]]
    assert got["offset_mapping"][0, 1].tolist() == [0, 1] and got["offset_mapping"][0, 7].tolist() == [0, 0]
    ident = B.expected_batch([[3, 4, 5]], B.spec(3), (None, 4, False))
    assert ident["input_ids"].tolist() == [[3, 1, 1]] and ident["n_unknown"] == 2


# ---- the dense vocabularies

def _loaded(swt, ref_dir, cls):
    tok = getattr(swt, cls)()
    tok.load_resources(os.path.join(ref_dir, "resources/pretrained", "FastBPE" if "BPE" in cls else "FastWordPiece"))
    return tok


@pytest.mark.parametrize("cls", ["NaiveBPE", "FastBPE", "NaiveWP", "FastWP"])
def test_vocab_list_is_a_bijection_and_survives_a_save(swt, ref_dir, corpora, tmp_path, cls):
    tok = _loaded(swt, ref_dir, cls)
    names = tok.vocab_list()
    assert len(set(names)) == len(names)
    assert [tok.token_to_id(t) for t in names] == list(range(len(names)))
    sp = tok.special_ids()
    assert [names[sp[k]] for k in ("pad", "unk", "cls", "sep")] == ["[PAD]", "[UNK]", "[CLS]", "[SEP]"]
    assert tok.token_to_id("no such token ☃") == sp["unk"]
    tok.save_resources(str(tmp_path / cls))
    again = getattr(swt, cls)()
    again.load_resources(str(tmp_path / cls))
    assert again.vocab_list() == names
    # every token string the reference produced on pan_tadeusz has an id of its own
    ref = corpora["pan_tokens"]["FastBPE" if "BPE" in cls else "FastWordPiece"]
    assert len(ref) == 989
    strings = {t for row in ref for t in row}
    got = {t: tok.token_to_id(t) for t in strings}
    assert sp["unk"] not in got.values() and len(set(got.values())) == len(strings)
    if "WP" in cls:
        assert tok.token_to_id("['UNK']") == sp["unk"] == tok.token_to_id("[UNK]")
        assert names[:len(tok.vocab)] == sorted(tok.vocab)  # the identity on the encoder's ids


def test_bpe_vocab_list_layout(swt, ref_dir):
    tok = _loaded(swt, ref_dir, "FastBPE")
    names = tok.vocab_list()
    assert names[:4] == ["[PAD]", "[UNK]", "[CLS]", "[SEP]"]
    n = (len(names) - 4) // 2
    bare = names[4:4 + n]
    assert bare == sorted(bare) and names[4 + n:] == ["##" + s for s in bare]
    assert {l + r for l, r in tok.merges_list} <= set(bare) and "," in bare
    assert tok.token_to_id("中") == tok.special_ids()["unk"]  # a code point of no merge and outside the base alphabet


# ---- the host forms refuse bad arguments before they look for a device

def _rows_call(native, spec, ids, off, cmap=None, n_map=100, flagged=0, row_base=None, rows_cap=8, out_ids=True, out_mask=True):
    u32p, u64p, u8p = native.u32p, native.u64p, native.u8p
    out = np.zeros(rows_cap * max(spec.width, 1), dtype=np.int32)
    mask = np.zeros(rows_cap * max(spec.width, 1), dtype=np.uint8)
    info = np.zeros(3, dtype=np.uint64)
    rc = native.lib().swt_batch_rows(native.ptr(ids, u32p), native.ptr(off, u64p), int(off.size) - 1,
                                     native.ptr(cmap, u32p) if cmap is not None else None, n_map, flagged, None, None, C.byref(spec),
                                     native.ptr(row_base, u64p) if row_base is not None else None, rows_cap,
                                     out.ctypes.data_as(C.c_void_p) if out_ids else None, native.ptr(mask, u8p) if out_mask else None,
                                     None, None, None, None, native.ptr(info, u64p))
    return rc, info


def test_host_forms_refuse_bad_arguments_without_a_device(native):
    ids = np.arange(10, dtype=np.uint32)
    off = np.array([0, 4, 10], dtype=np.uint64)
    good = native.batch_spec(8, cls_id=2, sep_id=3)
    INV = native.ERR_INVALID
    bad_specs = {
        "cap < 1": native.batch_spec(2, cls_id=2, sep_id=3),
        "cap < 1 without specials": native.batch_spec(0),
        "stride >= cap": native.batch_spec(8, stride=6, cls_id=2, sep_id=3),
        "pad_id none": native.batch_spec(8, pad_id=native.BATCH_NONE),
        "unk_id none": native.batch_spec(8, unk_id=native.BATCH_NONE),
    }
    unknown = native.batch_spec(8)
    unknown.flags = 8
    bad_specs["unknown flag"] = unknown
    for name, s in bad_specs.items():
        assert _rows_call(native, s, ids, off)[0] == INV, name
    assert _rows_call(native, good, ids, off, out_ids=False)[0] == INV
    assert _rows_call(native, good, ids, off, out_mask=False)[0] == INV
    assert _rows_call(native, good, ids, np.array([0, 6, 4], dtype=np.uint64))[0] == INV  # decreasing offsets
    assert _rows_call(native, good, ids, off, cmap=None, flagged=1)[0] == INV  # flagged with a NULL map
    windows = native.batch_spec(8, stride=1, windows=True, cls_id=2, sep_id=3)
    assert _rows_call(native, windows, ids, off)[0] == INV  # windows without row_base
    assert _rows_call(native, windows, ids, off, row_base=np.array([0, 1, 3], dtype=np.uint64))[0] == INV  # not the plan: 10 tokens need 2 rows
    assert "row_base" in native.lib().swt_last_error().decode()
    # the capacity answer needs no device either: cap 3 and step 2 make 2 + 3 rows of 4 and 6 tokens
    rc, info = _rows_call(native, native.batch_spec(5, stride=1, windows=True, cls_id=2, sep_id=3), ids, off,
                          row_base=np.array([0, 2, 5], dtype=np.uint64), rows_cap=4)
    assert rc == native.ERR_CAPACITY and int(info[0]) == 5
    # the plan calls
    row_base, info2 = np.zeros(3, dtype=np.uint64), np.zeros(2, dtype=np.uint64)
    plan = lambda s, o, rb=row_base: native.lib().swt_batch_plan(native.ptr(o, native.u64p), int(o.size) - 1, C.byref(s),
                                                                  native.ptr(rb, native.u64p) if rb is not None else None,
                                                                  native.ptr(info2, native.u64p))
    assert plan(native.batch_spec(2, windows=True, cls_id=2, sep_id=3), off) == INV
    assert plan(native.batch_spec(8, stride=6, windows=True, cls_id=2, sep_id=3), off) == INV
    assert plan(unknown, off) == INV
    assert plan(good, np.array([0, 6, 4], dtype=np.uint64)) == INV
    assert plan(good, off, None) == INV
    with pytest.raises(native.SwtError):
        native.check(plan(unknown, off))


def test_batch_capacity_and_struct(native):
    cols, group = native.batch_capacity()
    assert cols >= 64 and cols % 64 == 0 and group >= 64
    assert C.sizeof(native.BatchSpec) == 28
    s = native.batch_spec(16, 2, windows=True, pad_left=True, ids64=True, cls_id=5)
    assert (s.width, s.stride, s.flags, s.cls_id, s.sep_id) == (16, 2, 7, 5, native.BATCH_NONE)
