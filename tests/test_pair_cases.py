"""Sentence-pair batches without a GPU: the Python model of tests/pair_cases.py against what the `tokenizers` wheel recorded
(tests/golden/pair_batches.json), and the argument checks the host forms of swt_batch_pair_plan / swt_batch_pair_rows make before
anything touches a device."""
import ctypes as C

import numpy as np
import pytest

from . import batch_cases as B
from . import pair_cases as P


@pytest.fixture(scope="module")
def recorded(golden):
    return golden("pair_batches.json")


def _spec_of(g, width, stride, left, specials, windows):
    i = g["ids"]
    return P.spec(width, stride, windows, bool(left), False, i["pad"], i["unk"], i["cls"] if specials else None,
                  i["sep"] if specials else None)


def _slots(text, width):
    """the fixture's two characters per slot -> ids, mask, type, special, seq, each [rows, width]"""
    code = np.frombuffer(text.encode("ascii"), dtype=np.uint8).astype(np.int32).reshape(-1, width, 2)
    mask = code[:, :, 0] < 80
    extra = code[:, :, 1] - 48
    return {"input_ids": np.where(mask, code[:, :, 0] - 40, code[:, :, 0] - 80).astype(np.int32), "attention_mask": mask.astype(np.uint8),
            "token_type_ids": (extra & 1).astype(np.int32), "special_tokens_mask": ((extra >> 1) & 1).astype(np.uint8),
            "sequence_ids": ((extra >> 2) - 1).astype(np.int8)}


def _pair(g, na, nb):
    return [[g["ids"]["first_a"] + i for i in range(na)]], [[g["ids"]["first_b"] + i for i in range(nb)]]


def _same(got, want, rows, what, specials=True):
    """Without a template the wheel's OVERFLOWING encodings lose their sequence ranges -- sequence_ids are 0 on both sides with
    only_first and None on B with only_second, the first encoding being right in both -- which is no behaviour to follow: there
    the sequence ids are held to the first row, and to include/swt.h (0 on A, 1 on B) by the type ids, which the wheel keeps."""
    for k, v in want.items():
        n = 1 if k == "sequence_ids" and not specials else rows
        assert np.array_equal(got[k][:n], v[:n]), (k, what)
    if not specials:
        live = got["special_tokens_mask"] == 0
        assert np.array_equal(got["sequence_ids"][live], got["token_type_ids"][live]) and (got["sequence_ids"][~live] == -1).all()
    assert np.array_equal(got["length"], want["attention_mask"][:rows].sum(axis=1)), what


def test_model_equals_the_recorded_cases(recorded):
    """every recorded case: windowed (the encoding and its overflowing encodings; refused exactly where the wheel raises) and
    truncating (the encoding alone; refused exactly where the wheel raises whatever the stride, that is with stride 0)"""
    n_max = recorded["n_max"]
    seen, n_refused = set(), 0
    for key, entries in recorded["cases"].items():
        width, stride, strategy, left, specials = (int(x) for x in key.split(","))
        assert len(entries) == (n_max + 1) ** 2
        at_zero = recorded["cases"]["%d,0,%d,%d,%d" % (width, strategy, left, specials)]
        for i, text in enumerate(entries):
            na, nb = divmod(i, n_max + 1)
            seen.add((width, stride, strategy, left, specials, na, nb))
            a, b = _pair(recorded, na, nb)
            if strategy != P.LONGEST_FIRST:
                got = P.expected_pair_batch(a, b, _spec_of(recorded, width, stride, left, specials, True), strategy)
                assert (got["status"][0] == P.REFUSED) == (text == "E") == bool(got["refused"]), (key, na, nb)
                if text == "E":
                    n_refused += 1
                    assert got["input_ids"].shape == (1, width) and (got["input_ids"] == recorded["ids"]["pad"]).all()
                    assert not got["attention_mask"].any() and got["length"].tolist() == [0] and (got["sequence_ids"] == -1).all()
                    assert got["special_tokens_mask"].all() and not got["token_type_ids"].any()
                else:
                    want = _slots(text, width)
                    rows = want["input_ids"].shape[0]
                    assert got["row_base"].tolist() == [0, rows] and got["lost"] == 0
                    _same(got, want, rows, (key, na, nb), specials)
            assert text != "E" or strategy != P.LONGEST_FIRST
            cut = P.expected_pair_batch(a, b, _spec_of(recorded, width, stride, left, specials, False), strategy)
            assert (cut["status"][0] == P.REFUSED) == (at_zero[i] == "E"), (key, na, nb)
            if text != "E":
                want = _slots(text, width)
                _same(cut, want, 1, (key, na, nb, "cut"))
                assert cut["lost"] == (na + nb > width - 3 * specials) and cut["longest"] == na + nb
    # the grid the fixture promises
    want = set()
    for w, l, sp in [(6, 0, 1), (7, 0, 1), (8, 0, 1), (9, 0, 1), (8, 1, 1), (5, 0, 0)]:
        for strategy in range(3):
            for s in range(1 if strategy == 0 else w - 3 * sp):
                want |= {(w, s, strategy, l, sp, na, nb) for na in range(9) for nb in range(9)}
    assert seen == want and len(want) == 5022 and n_refused > 1000


def test_the_issue_examples_of_longest_first():
    for (na, nb, cap), keep in {(4, 6, 6): (3, 3), (5, 2, 5): (3, 2), (6, 1, 5): (4, 1), (7, 7, 6): (3, 3)}.items():
        assert P.pair_cut(na, nb, cap, 0, False, P.LONGEST_FIRST)[1:3] == keep
    # a row that fits is never refused, whatever the stride: na = 2, nb = 3, width 8, stride 3
    assert P.pair_cut(2, 3, 5, 3, True, P.ONLY_SECOND) == (False, 2, 3, 0, 0, 1)


def test_model_equals_the_recorded_batch(recorded):
    b = recorded["batch"]
    pairs = [_pair(recorded, na, nb) for na, nb in b["lengths"]]
    got = P.expected_pair_batch([p[0][0] for p in pairs], [p[1][0] for p in pairs], _spec_of(recorded, b["width"], b["stride"], 0, 1, True),
                                b["strategy"])
    want = _slots(b["slots"], b["width"])
    _same(got, want, want["input_ids"].shape[0], "batch")
    assert got["sample"].tolist() == b["sample"] and not got["refused"]
    assert [int(x) for x in got["row_base"][:-1]] == [b["sample"].index(i) for i in range(len(pairs))]


def test_model_dense_ids_and_payloads():
    cmap = np.array([5, 6, P.NONE, 7, 15, 16, 17, P.NONE], dtype=np.uint32)  # n_map 4, flagged
    a, b = [[0, 1 | 0x80000000, 2]], [[3 | 0x80000000, 4, 0 | 0x80000000, 1]]
    pay = (([[(i, i + 1) for i in range(3)]], [[0, 0, 1]]), ([[(10 + i, 11 + i) for i in range(4)]], [[0, 1, 1, 2]]))
    got = P.expected_pair_batch(a, b, P.spec(9, cls_id=2, sep_id=3, pad_id=9, unk_id=1), P.ONLY_SECOND, (cmap, 4, True), pay)
    assert got["input_ids"].tolist() == [[2, 5, 16, 1, 3, 1, 1, 15, 3]]  # B cut to 3 tokens: 3|CONT -> NONE, 4 >= n_map
    assert got["token_type_ids"].tolist() == [[0, 0, 0, 0, 0, 1, 1, 1, 1]]
    assert got["sequence_ids"].tolist() == [[-1, 0, 0, 0, -1, 1, 1, 1, -1]]
    assert got["special_tokens_mask"].tolist() == [[1, 0, 0, 0, 1, 0, 0, 0, 1]]
    assert got["word_ids"].tolist() == [[-1, 0, 0, 1, -1, 0, 1, 1, -1]]  # B's word indices start again at 0
    assert got["offset_mapping"][0, 5].tolist() == [10, 11] and got["offset_mapping"][0, 4].tolist() == [0, 0]
    assert got["n_unknown"] == 3 and got["lost"] == 1 and got["longest"] == 7


ONE_SIDED = ((P.ONLY_FIRST, True), (P.ONLY_SECOND, True), (P.ONLY_FIRST, False), (P.ONLY_SECOND, False), (P.LONGEST_FIRST, False))
SINGLE_KEYS = ("input_ids", "attention_mask", "length", "sample", "row_base", "offset_mapping", "word_ids")


def test_a_pair_with_an_empty_side_is_the_single_batch_of_the_other_side():
    """Without specials the two models meet: only_first with (n, 0) and only_second with (0, n), windowed and truncating, and
    longest_first with (n, 0) truncating, give the single-sequence batch of the side that holds the tokens, and refuse no pair.
    Widths of one token up to one past a full lane group, the strides 0, cap // 3 and cap - 1, both padding sides, the lengths
    at the window seams and one of several windows."""
    n_cases = 0
    for width in (1, 4, 6, 9, 63, 64, 65):
        for stride in sorted({0, width // 3, width - 1}):
            lengths = B.seam_lengths(width, width - stride) + [3 * width + 1]
            for left in (False, True):
                for strategy, windows in ONE_SIDED:
                    n_cases += 1
                    side = int(strategy == P.ONLY_SECOND)
                    rows_a, rows_b, _, _, _, pay = P.pair_stream([(0, n) if side else (n, 0) for n in lengths], seed=width)
                    s = P.spec(width, stride, windows, pad_left=left)
                    pair = P.expected_pair_batch(rows_a, rows_b, s, strategy, None, pay)
                    single = B.expected_batch(rows_b if side else rows_a, s, None, pay[side])
                    assert pair["refused"] == 0 and not pair["status"].any()
                    for k in SINGLE_KEYS:
                        assert np.array_equal(pair[k], single[k]), (k, width, stride, left, strategy, windows)
    assert n_cases == 190


# ---- the host forms refuse bad arguments before they look for a device

def _calls(native):
    lib, p = native.lib(), native.ptr
    u32p, u64p, u8p = native.u32p, native.u64p, native.u8p

    def plan(spec, off_a, off_b, strategy, row_base=True, status=True, info=True):
        n = int(off_a.size) - 1
        rb, st, inf = np.zeros(n + 1, dtype=np.uint64), np.zeros(n + 1, dtype=np.uint8), np.zeros(5, dtype=np.uint64)
        return lib.swt_batch_pair_plan(p(off_a, u64p), p(off_b, u64p), n, C.byref(spec) if spec is not None else None, strategy,
                                       p(rb, u64p) if row_base else None, p(st, u8p) if status else None, p(inf, u64p) if info else None)

    def rows(spec, ids, off_a, off_b, strategy, cmap=None, n_map=100, flagged=0, row_base=None, status=None, rows_cap=8, out_ids=True,
             out_mask=True, spans=None, out_spans=False):
        n = int(off_a.size) - 1
        slots = rows_cap * max(spec.width, 1)
        out, mask = np.zeros(slots, dtype=np.int32), np.zeros(slots, dtype=np.uint8)
        osp = np.zeros(2 * slots, dtype=np.uint32)
        info = np.zeros(5, dtype=np.uint64)
        rc = lib.swt_batch_pair_rows(p(ids, u32p), p(off_a, u64p), p(off_b, u64p), n, p(cmap, u32p) if cmap is not None else None, n_map,
                                     flagged, p(spans, u32p) if spans is not None else None, None, C.byref(spec), strategy,
                                     p(row_base, u64p) if row_base is not None else None, p(status, u8p) if status is not None else None,
                                     rows_cap, out.ctypes.data_as(C.c_void_p) if out_ids else None, p(mask, u8p) if out_mask else None,
                                     None, None, None, p(osp, u32p) if out_spans else None, None, None, None, p(info, u64p))
        return rc, info

    return plan, rows


def test_host_forms_refuse_bad_arguments_without_a_device(native):
    plan, rows = _calls(native)
    ids = np.arange(20, dtype=np.uint32)
    off_a = np.array([0, 2, 6], dtype=np.uint64)    # A: 2 and 4 tokens
    off_b = np.array([6, 9, 19], dtype=np.uint64)   # B: 3 and 10 tokens
    down = np.array([0, 6, 4], dtype=np.uint64)
    good = native.batch_spec(8, cls_id=2, sep_id=3)
    windows = native.batch_spec(8, stride=1, windows=True, cls_id=2, sep_id=3)
    INV, SECOND = native.ERR_INVALID, native.PAIR_ONLY_SECOND
    unknown = native.batch_spec(8, cls_id=2, sep_id=3)
    unknown.flags = 8
    bad_specs = {
        "cap < 1": native.batch_spec(3, cls_id=2, sep_id=3),
        "cap < 1 without specials": native.batch_spec(0),
        "stride >= cap": native.batch_spec(8, stride=5, cls_id=2, sep_id=3),
        "pad_id none": native.batch_spec(8, pad_id=native.BATCH_NONE, cls_id=2, sep_id=3),
        "unk_id none": native.batch_spec(8, unk_id=native.BATCH_NONE, cls_id=2, sep_id=3),
        "cls without sep": native.batch_spec(8, cls_id=2),
        "sep without cls": native.batch_spec(8, sep_id=3),
        "unknown flag": unknown,
    }
    for name, s in bad_specs.items():
        assert rows(s, ids, off_a, off_b, SECOND)[0] == INV, name
    for name in ("cls without sep", "sep without cls", "unknown flag"):
        assert plan(bad_specs[name], off_a, off_b, SECOND) == INV, name
    for strategy in (3, 0xFFFFFFFF):
        assert rows(good, ids, off_a, off_b, strategy)[0] == INV and plan(good, off_a, off_b, strategy) == INV
    assert rows(windows, ids, off_a, off_b, native.PAIR_LONGEST_FIRST, row_base=np.array([0, 1, 2], dtype=np.uint64))[0] == INV
    assert plan(windows, off_a, off_b, native.PAIR_LONGEST_FIRST) == INV  # windows of both sides: out of scope
    assert "longest_first" in native.lib().swt_last_error().decode()
    assert rows(good, ids, off_a, off_b, SECOND, out_ids=False)[0] == INV
    assert rows(good, ids, off_a, off_b, SECOND, out_mask=False)[0] == INV
    assert rows(good, ids, down, off_b, SECOND)[0] == INV and rows(good, ids, off_a, down, SECOND)[0] == INV  # decreasing offsets
    assert rows(good, ids, off_a, off_b, SECOND, cmap=None, flagged=1)[0] == INV  # flagged with a NULL map
    assert rows(good, ids, off_a, off_b, SECOND, out_spans=True)[0] == INV  # an output without its payload
    assert rows(windows, ids, off_a, off_b, SECOND)[0] == INV  # windows without row_base
    # width 8, stride 1, only_second: (2, 3) fits; (4, 10) has a budget of 1 and is refused: 1 + 1 rows
    ok_base, ok_status = np.array([0, 1, 2], dtype=np.uint64), np.array([0, 1], dtype=np.uint8)
    assert rows(windows, ids, off_a, off_b, SECOND, row_base=np.array([0, 1, 3], dtype=np.uint64), status=ok_status)[0] == INV
    assert "row_base" in native.lib().swt_last_error().decode()
    assert rows(windows, ids, off_a, off_b, SECOND, row_base=ok_base, status=np.array([0, 0], dtype=np.uint8))[0] == INV
    assert "status" in native.lib().swt_last_error().decode()
    # the capacity answer needs no device either: stride 0 gives (4, 10) ten windows of one token
    s0 = native.batch_spec(8, stride=0, windows=True, cls_id=2, sep_id=3)
    rc, info = rows(s0, ids, off_a, off_b, SECOND, row_base=np.array([0, 1, 11], dtype=np.uint64), status=np.array([0, 0], dtype=np.uint8),
                    rows_cap=10)
    assert rc == native.ERR_CAPACITY and int(info[0]) == 11
    # the plan calls
    assert plan(native.batch_spec(3, windows=True, cls_id=2, sep_id=3), off_a, off_b, SECOND) == INV
    assert plan(native.batch_spec(8, stride=5, windows=True, cls_id=2, sep_id=3), off_a, off_b, SECOND) == INV
    assert plan(good, down, off_b, SECOND) == INV and plan(good, off_a, down, SECOND) == INV
    assert plan(None, off_a, off_b, SECOND) == INV
    for missing in ("row_base", "status", "info"):
        assert plan(good, off_a, off_b, SECOND, **{missing: False}) == INV, missing


def test_encode_batch_refuses_pair_keywords_without_pairs_and_bad_pairs(swt):
    """decided from the arguments alone, before a vocabulary or a device is looked for"""
    tok = swt.FastWP()
    for bad in ({"truncation": "only_first"}, {"truncation": "only_second"}, {"return_token_type_ids": True}, {"return_special_tokens_mask": True},
                {"truncation": "shortest"}, {"text_pairs": ["b", "c"]}, {"text_pairs": ["b"], "truncation": "shortest"},
                {"text_pairs": ["b"], "max_length": 8, "return_overflowing": True},
                {"text_pairs": ["b"], "max_length": 8, "return_overflowing": True, "truncation": "longest_first"}):
        with pytest.raises(ValueError):
            tok.encode_batch(["a"], **bad)
    with pytest.raises(TypeError):
        tok.encode_batch(["a"], text_pairs="b")
    with pytest.raises(TypeError):
        tok.encode_batch(["a"], text_pairs=[None])


def test_pair_capacity_and_constants(native):
    cols, group = native.batch_pair_capacity()
    assert cols >= 64 and cols % 64 == 0 and group >= 64
    assert (native.PAIR_LONGEST_FIRST, native.PAIR_ONLY_FIRST, native.PAIR_ONLY_SECOND) == (0, 1, 2)
    assert (native.PAIR_OK, native.PAIR_REFUSED) == (0, 1)
