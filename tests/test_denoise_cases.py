"""Span corruption without a GPU: the exports and the spec's size, what corrupt_spans and the host forms refuse from their
arguments alone, the host's length tables, and the model (tests/denoise_cases.py) on three rows worked out by hand."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from tests import denoise_cases as D

W, CT, SEP, PAD, MK, IGN = D.WORD, D.CONT, D.SEP, D.PAD, D.MASK_ID, -100


def test_symbols_and_constants(native):
    lib = C.CDLL(native._build.LIB_PATH)
    for name in ("swt_denoise_plan", "swt_denoise_plan_dev", "swt_denoise_rows", "swt_denoise_rows_dev", "swt_denoise_capacity"):
        assert hasattr(lib, name) and name in native.SIGNATURES
    assert C.sizeof(native.DenoiseSpec) == 304 and native.DenoiseSpec.len_below.offset == 16 and native.DenoiseSpec.n_len.offset == 264
    assert native.denoise_capacity() == (native.mlm_capacity()[0], 2 * native.mlm_capacity()[0], 31)
    assert (native.DENOISE_WHOLE_WORD, native.DENOISE_IDS64) == (native.MLM_WHOLE_WORD, native.BATCH_IDS64)


def test_host_forms_refuse_bad_arguments_without_a_device(native):
    a = np.arange(4, 16, dtype=np.int32).reshape(3, 4) % 12
    o, lab, cls, sent, info = np.zeros_like(a), np.zeros_like(a), D.CLS_TAB, D.SENTINELS, np.full(7, 9, dtype=np.uint64)
    lib, p = native.lib(), lambda x, typ=C.c_void_p: None if x is None else C.cast(C.c_void_p(x.ctypes.data), typ)

    def rows(mode=D.SENTINEL, ids=a, out=o, labels=lab, sentinels=sent, n_rows=3, width=4, info=None, table=(), **fields):
        s = native.denoise_spec(mode, 12, D.MASK_ID, D.PAD, 1 << 30, table, len(D.SENTINELS), 4)
        for k, v in fields.items():
            setattr(s, k, v)
        rc = lib.swt_denoise_rows(p(ids), n_rows, width, p(cls, native.u8p), p(sentinels, native.u32p), C.byref(s), p(out), None, None, p(labels),
                                  None, p(info, native.u64p))
        msg = lib.swt_last_error().decode()
        plan =lib.swt_denoise_plan(p(ids), n_rows, width, p(cls, native.u8p), C.byref(s), p(np.zeros(7, dtype=np.uint64), native.u64p))
        return rc, msg, plan

    for kw, word, both in (({"ids": None}, "ids", True), ({"out": None}, "out_ids", False), ({"labels": None}, "out_labels", False),
                           ({"sentinels": None}, "sentinel_ids", False), ({"width": 0}, "width", True), ({"n_rows": 1 << 32}, "rows", True),
                           ({"flags": 2}, "flag", True), ({"mode": 3}, "mode", True), ({"start_below": (1 << 32) + 1}, "start_below", True),
                           ({"n_len": 32}, "n_len", True), ({"table": (5, 4)}, "len_below", True), ({"table": (4, (1 << 32) + 1)}, "len_below", True),
                           ({"n_class": 0}, "n_class", True), ({"n_sentinel": 1}, "n_sentinel", True), ({"out": a}, "out_ids", False),
                           ({"labels": a[1:]}, "out_labels", False), ({"mode": D.INFILL}, "out_labels", False)):
        rc, msg, plan = rows(**kw)
        assert rc == native.ERR_INVALID and word in msg, (kw, msg)
        assert (plan == native.ERR_INVALID) == both, kw
    rc, _, plan = rows(n_rows=0, info=info)  # no row: success without a device, info zeroed
    assert rc == 0 and plan == 0 and info.tolist() == [0] * 7
    assert rows(mode=D.MASK, n_sentinel=0, sentinels=None, n_rows=0)[0] == 0 and rows(mode=D.INFILL, labels=None, n_rows=0)[0] == 0
    if native.device_count() == 0:  # everything in order: only now is a device looked for
        assert rows()[0] == native.ERR_NO_DEVICE


def test_corrupt_spans_refuses_bad_arguments(swt, ref_dir):
    tok = swt.FastWP()  # decided before a vocabulary is looked for
    ids = np.zeros((2, 3), dtype=np.int32)
    for bad in ({"mode": "t5"}, {"noise_density": -0.1}, {"noise_density": 1.5}, {"mean_span_length": 0.5}, {"mean_span_length": 40},
                {"lengths": "uniform"}, {"lengths": "fixed", "mean_span_length": 2.5}, {"max_span_length": 0}, {"max_span_length": 33},
                {"lengths": [0.5, 0.6]}, {"lengths": [1.5, -0.5]}, {"lengths": []}, {"lengths": [1 / 33.0] * 33}, {"seed": -1},
                {"seed": 1 << 64}, {"epoch": 1 << 32}, {"target_length": 0}):
        with pytest.raises(ValueError):
            tok.corrupt_spans(ids, **bad)
    tok.load_resources(os.path.join(ref_dir, "resources/pretrained", "FastWordPiece"))
    tok.add_special_tokens(["<extra_id_0>", "<extra_id_1>"])
    for bad in (["<extra_id_0>", "<extra_id_7>"], ["<extra_id_0>"], [5, -1]):
        with pytest.raises(ValueError):
            tok.corrupt_spans(ids, sentinels=bad)
    for bad in (np.zeros((2, 3), dtype=np.int16), np.zeros(6, dtype=np.int32), np.zeros((3, 4), dtype=np.int32).T, [[1, 2]]):
        with pytest.raises(TypeError):
            tok.corrupt_spans(bad)


@pytest.mark.parametrize("lengths, mean, longest", [("fixed", 1, 10), ("fixed", 4, 10), ("fixed", 32, 10), ("geometric", 3.0, 10),
                                                    ("geometric", 1.0, 32), ("geometric", 5.0, 32), ("poisson", 3.0, 10),
                                                    ("poisson", 3.5, 32), ([0.25, 0.0, 0.75], None, None)])
def test_length_tables(swt, lengths, mean, longest):
    """non-decreasing, 2^32 at most, one entry per length but the last; the table's mean is the distribution's, each entry being
    floored by less than 2^-32"""
    from subword_tokenizers_amd import batching as B
    below, table_mean = B._denoise_lengths(mean or 3.0, lengths, longest or 10)
    if lengths == "fixed":
        p = [0.0] * (mean - 1) + [1.0]
    elif lengths == "geometric":
        p = [(1 - 1 / mean) ** k for k in range(longest)]
    elif lengths == "poisson":
        p = [mean ** k / math.factorial(k) for k in range(1, longest + 1)]
    else:
        p = lengths
    p = [x / sum(p) for x in p]
    assert len(below) == len(p) - 1 <= 31 and all(a <= b for a, b in zip(below, below[1:])) and all(0 <= b <= D.ONE for b in below)
    want = sum((k + 1) * x for k, x in enumerate(p))
    assert want - 1e-9 <= table_mean <= want + len(p) * 2.0 ** -32 + 1e-9
    assert table_mean == 1.0 + sum(1.0 - b / 2.0 ** 32 for b in below)
    _, start, _ = B._denoise_thresholds("mask", 0.15, mean or 3.0, lengths, longest or 10)
    assert start == int(0.15 / table_mean * 2.0 ** 32)


def test_model_on_rows_worked_out_by_hand():
    ids = np.array([[W, CT, SEP, W, W, PAD]], dtype=np.int32)
    # every unit starts a span of one unit: the runs are the words on either side of [SEP]
    got = D.expected(ids, D.CLS_TAB, D.spec(D.SENTINEL, D.ONE, []))
    assert got["input_ids"].tolist() == [[100, SEP, 101, PAD, PAD, PAD]] and got["attention_mask"].tolist() == [[1, 1, 1, 0, 0, 0]]
    assert got["labels"].tolist() == [[100, W, CT, 101, W, W, 102]] and got["length"].tolist() == [4] and got["label_length"].tolist() == [7]
    assert got["info"].tolist() == [4, 4, 2, 0, 0, 4, 7]
    # two sentinels: the second run is given back, and labels of width 2 are cut
    got = D.expected(ids, D.CLS_TAB, D.spec(D.SENTINEL, D.ONE, [], n_sentinel=2, label_width=2))
    assert got["input_ids"].tolist() == [[100, SEP, W, W, PAD, PAD]] and got["labels"].tolist() == [[100, W]]
    assert got["info"].tolist() == [4, 2, 2, 1, 1, 5, 4]
    got = D.expected(ids, D.CLS_TAB, D.spec(D.INFILL, D.ONE, []))
    assert got["input_ids"].tolist() == [[MK, SEP, MK, PAD, PAD, PAD]] and got["labels"] is None and got["length"].tolist() == [4]
    # no unit starts a span
    got = D.expected(ids, D.CLS_TAB, D.spec(D.SENTINEL, 0, [0] * 31))
    assert np.array_equal(got["input_ids"], ids) and got["labels"].tolist() == [[100]] and got["info"].tolist() == [4, 0, 0, 0, 0, 6, 1]
    # seed 0, row 0: x0 of the heads 0, 1, 3, 4, 7 is 2DCE73E5 E9535BE3 9E9DBCB9 1983B60E 7AB96FE8, so units 0 and 3 start below
    # 30000000; their x1 are 1348E23F and E97F4AB4: two units from unit 0, three from unit 3, of which the row has two
    ids = np.array([[W, W, CT, W, W, CT, CT, W]], dtype=np.int64)
    got = D.expected(ids, D.CLS_TAB, D.spec(D.MASK, 0x30000000, [0x10000000, 0x80000000, 0xF0000000]))
    assert got["input_ids"].tolist() == [[MK, MK, MK, W, MK, MK, MK, MK]] and got["labels"].tolist() == [[W, W, CT, IGN, W, CT, CT, W]]
    assert got["info"].tolist() == [8, 7, 2, 0, 0, 8, 0] and got["input_ids"].dtype == np.int64
