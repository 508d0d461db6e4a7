"""The NumPy model of masked-LM inference (tests/fill_cases.py) against plain Python loops and cases worked out by hand, the
tolerance on out_lse under its cap, the library's exports, and what the host forms and the methods refuse from the arguments
alone -- all without a device."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from tests import fill_cases as F

NAMES = ("swt_mlm_positions", "swt_mlm_positions_dev", "swt_mlm_predict", "swt_mlm_predict_dev", "swt_fill_capacity")
METHODS = ("fill_mask", "mlm_scores")


# ---- the model

def _loop_order(x):
    """selection by loops: repeatedly the best entry that is left"""
    left = [i for i in range(len(x)) if not math.isnan(x[i])]
    out = []
    while left:
        best = left[0]
        for i in left[1:]:
            if x[i] > x[best]:
                best = i
        out.append(best)
        left.remove(best)
    return out


def _loop_lse(x):
    if any(math.isnan(v) for v in x):
        return float("nan")
    m = max(x)
    if math.isinf(m):
        return m
    return m + math.log(math.fsum(math.exp(v - m) for v in x))


def test_model_against_loops_on_random_rows():
    rng = np.random.default_rng(5)
    for trial in range(60):
        V = int(rng.integers(1, 40))
        x = F.tie_row(rng, V, 4) if trial % 2 else F.normal_row(rng, V)
        if trial % 5 == 0:
            x[rng.integers(0, V)] = np.nan
        if trial % 7 == 0:
            x[rng.integers(0, V)] = -np.inf
        order = _loop_order([float(v) for v in x])
        assert F.row_order(x).tolist() == order
        want = _loop_lse([float(v) for v in x])
        got = F.row_lse(x)
        assert (math.isnan(want) and math.isnan(got)) or got == pytest.approx(want, rel=1e-14, abs=1e-14)
        for label in range(-1, V + 1):
            rank = order.index(label) if label in order else -1
            assert F.row_rank(x, label) == rank
        k = int(rng.integers(0, 8))
        labels = rng.integers(-1, V + 1, size=(1, 1))
        out = F.expected_predict(x.reshape(1, 1, V), [0], labels, k)
        if k:
            assert out["top_id"][0].tolist() == (order + [-1] * k)[:k]
        assert out["label_rank"][0] == F.row_rank(x, int(labels[0, 0]))


def test_cases_by_hand():
    nan, inf = float("nan"), float("inf")
    x = np.array([[[1.0, 3.0, 3.0, nan, -inf, 2.0], [0.0, 0.0, -inf, -inf, 0.0, 0.0], [nan] * 6, [-inf] * 6, [inf, 1.0, inf, 0.0, 0.0, 0.0]]],
                 dtype=np.float32)
    labels = np.array([[2, 5, 0, 6, 1]], dtype=np.int64)
    pos = np.array([0, 1, 2, 3, 4, 5, F.NO_POS], dtype=np.uint64)
    out = F.expected_predict(x, pos, labels, 3)
    assert out["top_id"].tolist() == [[1, 2, 5], [0, 1, 4], [-1, -1, -1], [0, 1, 2], [0, 2, 1], [-1, -1, -1], [-1, -1, -1]]
    assert out["top_logit"][0].tolist() == [3.0, 3.0, 2.0] and np.isnan(out["top_logit"][2]).all() and np.isnan(out["top_logit"][5]).all()
    assert out["label_id"].tolist() == [2, 5, 0, -1, 1, -1, -1]
    assert out["label_rank"].tolist() == [1, 3, -1, -1, 2, -1, -1]  # tied with a smaller id; the last of four zeros; a NaN logit; V
    assert np.array_equal(out["label_logit"], np.array([3.0, 0.0, nan, nan, 1.0, nan, nan], dtype=np.float32), equal_nan=True)
    assert math.isnan(out["lse"][0]) and out["lse"][1] == pytest.approx(math.log(4.0)) and math.isnan(out["lse"][2])
    assert out["lse"][3] == -inf and out["lse"][4] == inf and math.isnan(out["lse"][5])
    assert out["info"].tolist() == [7, 0, 2, 2, 1]  # positions; rank 0; rank < 3; rows with a NaN; labels out of range
    none = F.expected_predict(x, pos[:2], None, 0)
    assert none["top_id"] is None and none["label_rank"] is None and none["info"].tolist() == [2, 0, 0, 1, 0]
    # the argmax of the smallest index has rank 0, and k == 0 counts rank 0 alone
    assert F.expected_predict(x, [1], np.array([[0, 0, 0, 0, 0]]), 0)["info"].tolist() == [1, 1, 1, 0, 0]
    ids = np.array([[7, -100, 7], [-100, -100, 2]], dtype=np.int32)
    got = F.expected_positions(ids, -100, True)
    assert got["pos"].tolist() == [0, 2, 5] + [int(F.NO_POS)] * 3 and got["info"].tolist() == [3, 6]
    assert F.expected_positions(ids, 7)["pos"].tolist()[:3] == [0, 2, int(F.NO_POS)]


def test_lse_tol_under_its_cap(native):
    """the derived tolerance never exceeds the any-order worst case, and is made of what include/swt.h states"""
    STEP = native.fill_capacity()[0]
    for V in list(range(1, 3000)) + [8192, 30522, 70001, (1 << 31) - 1]:
        for lse in (0.0, 0.5, 1.0, 7.0, -30.0, 88.0):
            assert F.lse_tol(V, STEP, lse) <= F.lse_cap(V, lse), (V, lse)
        assert F.chain(V, STEP) == min(V - 1, (V + STEP - 1) // STEP + 8)
    assert F.lse_tol(1, STEP) < 4 * F.U and F.lse_tol(8192, STEP) < 80 * F.U
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "swt.h"), encoding="utf-8") as f:
        assert "chain(V) = min(V - 1, ceil(V / s) + 8)" in f.read()


# ---- the library

def test_symbols_and_constants(native, swt):
    lib = C.CDLL(native._build.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name) and name in native.SIGNATURES, name
    for name in METHODS:
        assert callable(getattr(swt.FastBPE, name)) and callable(getattr(swt.FastWP, name)), name
    step, per_block, k_max, scan_cells = native.fill_capacity()
    assert step >= 64 and step % 4 == 0 and per_block >= 1 and k_max == 64 and scan_cells >= 1024
    assert (native.FILL_EQUAL, native.FILL_NOT_EQUAL, native.FILL_IDS64) == (0, 1, 4)
    assert [n for n, _, _ in native.FILL_OUT] == ["lse", "top_id", "top_logit", "label_id", "label_logit", "label_rank"]


ROWS, WIDTH, VOCAB, NPOS, K = 3, 4, 5, 4, 2
CELLS = ROWS * WIDTH


def _arrays():
    """an array for every pointer of the two host forms, all apart from each other"""
    i32, f32, u64 = np.int32, np.float32, np.uint64
    return {"ids": np.zeros(CELLS, i32), "out_pos": np.full(CELLS, 9, u64), "info": np.full(6, 9, u64), "logits": np.zeros(CELLS * VOCAB, f32),
            "pos": np.arange(NPOS, dtype=u64), "labels": np.zeros(CELLS, i32), "out_lse": np.full(NPOS, 5, f32),
            "out_top_id": np.full(NPOS * K, 5, i32), "out_top_logit": np.full(NPOS * K, 5, f32), "out_label_id": np.full(NPOS, 5, i32),
            "out_label_logit": np.full(NPOS, 5, f32), "out_label_rank": np.full(NPOS, 5, i32)}


FORMS = {
    "swt_mlm_positions": ["ids", ("rows", ROWS), ("width", WIDTH), ("value", -100), ("mode", 1), ("flags", 0), "out_pos", "info"],
    "swt_mlm_predict": ["logits", ("rows", ROWS), ("width", WIDTH), ("n_vocab", VOCAB), "pos", ("n_pos", NPOS), "labels", ("flags", 0), ("k", K),
                        "out_lse", "out_top_id", "out_top_logit", "out_label_id", "out_label_logit", "out_label_rank", "info"],
}
REQUIRED = {"swt_mlm_positions": ("ids", "out_pos", "info"), "swt_mlm_predict": ("logits", "pos")}
BAD_POS = np.array([0, CELLS, 1, 2], np.uint64)
BAD = {"swt_mlm_positions": [({"width": 0}, "width"), ({"rows": 1 << 32}, "rows"), ({"width": 1 << 31}, "width"), ({"mode": 2}, "mode"),
                             ({"flags": 1}, "flags"), ({"rows": 1 << 20, "width": 1 << 12}, "rows * width")],
       "swt_mlm_predict": [({"width": 0}, "width"), ({"rows": 1 << 32}, "rows"), ({"n_vocab": 0}, "n_vocab"), ({"n_vocab": 1 << 31}, "n_vocab"),
                           ({"n_vocab": 1 << 40}, "n_vocab"), ({"k": 65}, "k"), ({"flags": 2}, "flags"),
                           ({"rows": 1 << 31, "width": 1 << 11, "n_vocab": 1 << 20}, "logits"), ({"n_pos": 1 << 32}, "n_pos"),
                           ({"k": 0}, "k"), ({"labels": None}, "labels"), ({"pos": BAD_POS.ctypes.data}, "pos")]}


def _call(native, form, arrays=None, **over):
    """one call of a host form; over: a pointer's name -> None or an address, a scalar's name -> its value"""
    arrays = arrays or _arrays()
    args = []
    for a in FORMS[form]:
        name, value = a if isinstance(a, tuple) else (a, arrays[a].ctypes.data)
        args.append(over.get(name, value))
    lib = native.lib()
    rc = getattr(lib, form)(*args)
    return rc, lib.swt_last_error().decode(), arrays


@pytest.mark.parametrize("form", sorted(FORMS))
def test_host_forms_refuse_bad_arguments_without_a_device(native, form):
    INV = native.ERR_INVALID
    pointers = [a for a in FORMS[form] if not isinstance(a, tuple)]
    for name in REQUIRED[form]:
        rc, msg, _ = _call(native, form, **{name: None})
        assert rc == INV and name in msg, (name, msg)
    for kw, word in BAD[form]:
        rc, msg, _ = _call(native, form, **kw)
        assert rc == INV and word in msg, (kw, msg)
    # every array off the alignment of its element type
    arrays = _arrays()
    for name in pointers:
        rc, msg, _ = _call(native, form, arrays, **{name: arrays[name].ctypes.data + 1})
        assert rc == INV and name in msg and "aligned" in msg, (name, msg)
    # every output over every input, and over another output: the same address, and one shifted into it
    for out in [n for n in pointers if n.startswith("out_") or n == "info"]:
        for other in pointers:
            if other == out:
                continue
            shift = 0 if arrays[other].nbytes < 16 else 8
            rc, msg, _ = _call(native, form, arrays, **{out: arrays[other].ctypes.data + shift})
            assert rc == INV and out in msg and "overlaps" in msg, (out, other, msg)
    # nothing to do: success without a device, info zeroed and nothing else written
    empty = {"rows": 0} if form == "swt_mlm_positions" else {"n_pos": 0}
    rc, msg, arrays = _call(native, form, **empty)
    assert rc == 0, msg
    if form == "swt_mlm_positions":
        assert arrays["info"].tolist() == [0, 0, 9, 9, 9, 9] and arrays["out_pos"].tolist() == [9] * CELLS
        rc, msg, _ = _call(native, form, rows=0, width=0)
        assert rc == 0, msg
    else:
        assert arrays["info"].tolist() == [0, 0, 0, 0, 0, 9]
        for k in pointers:
            if k.startswith("out_"):
                assert (arrays[k] == 5).all(), k
        rc, msg, _ = _call(native, form, n_pos=0, rows=0, width=0, labels=None, info=None, **{k: None for k in pointers if k.startswith("out_")})
        assert rc == 0, msg
        rc, msg, _ = _call(native, form, k=0, out_top_id=None, out_top_logit=None, n_pos=0)
        assert rc == 0, msg
        rc, msg, _ = _call(native, form, rows=0, n_pos=1)  # no cell: every position is outside
        assert rc == INV and "pos" in msg, msg
    if native.device_count() == 0:  # everything in order: only now is a device looked for
        rc, _, _ = _call(native, form)
        assert rc == native.ERR_NO_DEVICE


# ---- the Python methods, where no device is needed

def test_methods_refuse_bad_arguments(swt):
    tok = swt.FastWP()
    tok.load_resources(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref", "resources", "tests", "FastWordPiece"))
    ids, f32 = np.zeros((2, 5), dtype=np.int32), np.zeros((2, 5, 7), dtype=np.float32)
    calls = (lambda x, i, **kw: tok.fill_mask(i, x, **kw), lambda x, i, **kw: tok.mlm_scores(x, i, **kw))
    for call in calls:
        for bad in (f32.astype(np.float64), f32.astype(np.float16), f32.tolist(), None):
            with pytest.raises(TypeError):
                call(bad, ids)
        for bad in (ids.astype(np.int16), ids.astype(np.float32), ids.tolist(), ids[:, ::2], np.zeros(10, dtype=np.int32)):
            with pytest.raises(TypeError):
                call(f32, bad)
        for bad in (f32[:1], f32[:, :4], f32[0], f32.reshape(2, 5, 7, 1), np.zeros((2, 5, 0), dtype=np.float32)):
            with pytest.raises(ValueError):
                call(bad, ids)
        with pytest.raises(ValueError):
            call(np.zeros((2, 5, 14), dtype=np.float32)[:, :, ::2], ids)  # of the right shape and not contiguous: no silent copy
        for bad in (0, 65, -1, 2.5, True):
            with pytest.raises(ValueError):
                call(f32, ids, top_k=bad)
    try:
        import torch
    except ImportError:
        return
    for call in calls:
        with pytest.raises(TypeError):
            call(torch.zeros((2, 5, 7)), ids)  # not of the ids' kind
        with pytest.raises(TypeError):
            call(f32, torch.zeros((2, 5), dtype=torch.int32))  # a tensor that is not on the GPU
