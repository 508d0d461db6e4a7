"""swt_mlm_predict16 (half and bfloat16 logits) on the GPU, host and `_dev` forms, against the NumPy model (tests/fill_cases.py) on the
exactly widened float32 array: element by element, out_lse alone within lse_tol restated for chain16.  Seams from swt_fill_capacity16."""
import math

import numpy as np
import pytest

from tests import fill_cases as F

pytestmark = pytest.mark.gpu

FORMS = ["host", "dev"]
DTYPES = ["f16", "bf16"]


@pytest.fixture(scope="module")
def dev(native):
    assert native.device_count() >= 1, "no HIP device"
    native.init(0)
    return native


@pytest.fixture(scope="module")
def cap(dev):
    return dev.fill_capacity16()


def bits_of(x, dtype):
    """float32 values -> the uint16 bits of the dtype: half by rounding, bfloat16 by truncation to the upper 16 bits"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    return x.astype(np.float16).view(np.uint16) if dtype == "f16" else (x.view(np.uint32) >> 16).astype(np.uint16)


def widen(bits, dtype):
    return bits.view(np.float16).astype(np.float32) if dtype == "f16" else (bits.astype(np.uint32) << 16).view(np.float32)


def lse_tol16(V, cap, lse=0.0):
    """fill_cases.lse_tol with chain16(V) = min(V - 1, ceil(V / s16) + log2(lane_sums) + 6) for its chain, and never above the cap"""
    chain = min(V - 1, -(-V // cap[0]) + int(math.log2(cap[1])) + 6)
    r = (1.0 + (1.0 + math.log(V)) * F.U) * (1.0 + F.U) ** (chain + 2) - 1.0
    tol = r / (1.0 - r) + 2.0 * F.U * math.log(V) + F.U * abs(lse)
    assert tol <= F.lse_cap(V, lse)
    return tol


def call_dev(dev, form, head, logits, shape, pos, labels, k, shift=0):
    """a `_dev` form over torch tensors, the logits (a NumPy array of any 2- or 4-byte type) `shift` elements into their buffer"""
    import torch
    (rows, width, V), n = shape, len(pos)
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    size = logits.dtype.itemsize
    buf = up(np.concatenate([np.zeros(shift, logits.dtype), logits.reshape(-1)]).view(np.int16 if size == 2 else np.float32))
    d_pos, d_lab, info = up(pos.view(np.int64)), up(labels), torch.empty(5, dtype=torch.int64, device="cuda")
    out = {name: torch.empty((n, k) if per_k else n, dtype=torch.float32 if t == np.float32 else torch.int32, device="cuda")
           for name, t, per_k in dev.FILL_OUT if (labels is not None or not name.startswith("label")) and (k or not per_k)}
    p = lambda a: None if a is None else a.data_ptr()
    dev.check(getattr(dev.lib(), form)(buf.data_ptr() + shift * size, *head, rows, width, V, p(d_pos), n, p(d_lab),
                                       dev.FILL_IDS64 if labels is not None and labels.dtype == np.int64 else 0, k,
                                       *[p(out.get(name)) for name, _, _ in dev.FILL_OUT], p(info), None))
    torch.cuda.synchronize()
    got = {name: a.cpu().numpy() for name, a in out.items()}
    got["info"] = info.cpu().numpy().view(np.uint64)
    return got


def agree(got, want, tol, what):
    """every array of got equals want's element by element; lse lies within tol(lse) of the model's where that is finite"""
    for key, g in got.items():
        w = want[key]
        if g is None:
            continue
        if key != "lse":
            assert g.dtype == w.dtype and np.array_equal(g, w, equal_nan=g.dtype.kind == "f"), (what, key, g, w)
            continue
        finite = np.isfinite(w)
        assert g.dtype == np.float32 and np.array_equal(g[~finite].astype(np.float64), w[~finite], equal_nan=True), (what, key, g, w)
        for a, b in zip(g[finite].astype(np.float64), w[finite].astype(np.float64)):
            assert abs(a - b) <= tol(b), (what, key, a, b, abs(a - b) / F.U, tol(b) / F.U)


def run(dev, cap, form, dtype, bits, pos, labels, k, shift=0, what=""):
    code = dev.FILL_F16 if dtype == "f16" else dev.FILL_BF16
    pos = np.asarray(pos, dtype=np.uint64)
    want = F.expected_predict(widen(bits, dtype), pos, labels, k)
    if form == "host":
        view = np.concatenate([np.zeros(shift, np.uint16), bits.reshape(-1)])[shift:].reshape(bits.shape)
        got = dev.mlm_predict16(view, code, pos, labels, k)
    else:
        got = call_dev(dev, "swt_mlm_predict16_dev", (code,), bits, bits.shape, pos, labels, k, shift)
    agree(got, want, lambda lse: lse_tol16(bits.shape[2], cap, lse), (what, form, dtype, bits.shape, k, shift))
    return got


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", FORMS)
def test_geometry(dev, cap, form, dtype):
    """nine cells a call: more than a workgroup's, and with V odd at every alignment modulo eight; a position past the rows (`_dev`)"""
    rng = np.random.default_rng(16)
    s = cap[0]
    for V in (1, 7, 8, 9, 15, 17, s - 1, s, s + 1, 2 * s + 9):
        bits = bits_of(F.logits_of([F.tie_row(rng, V, 4) if i % 3 == 2 else F.normal_row(rng, V) for i in range(9)], 3, 3), dtype)
        labels = rng.integers(0, V, size=(3, 3)).astype(np.int32)
        pos = list(range(9)) + ([9, int(F.NO_POS), 4] if form == "dev" else [4])
        for shift in (0, 1):
            run(dev, cap, form, dtype, bits, pos, labels, 5, shift)


def order_rows(rng, V, dtype):
    """-> uint16 [14, V]: ties, both zeros, NaNs of both signs in the head, an octet and the tail, infinities, and the extremes: the
    subnormals next to zero, the greatest subnormal, the smallest normal, +-65504 (half) or the largest exponent (bfloat16)"""
    nan, inf, tiny = (0x7E00, 0x7C00, 0x0400) if dtype == "f16" else (0x7FC0, 0x7F80, 0x0080)
    ext = [0x0001, 0x8001, tiny - 1, tiny, inf - 1, (inf - 1) | 0x8000]
    rows = [bits_of(r, dtype) for r in (F.tie_row(rng, V), F.tie_row(rng, V, 7), F.normal_row(rng, V), F.zeros_row(rng, V, 5),
                                        np.full(V, -np.inf), np.full(V, 1.5))]
    rows.append(np.where(rng.integers(0, 2, V) > 0, 0x8000, 0).astype(np.uint16))  # 0.0 and -0.0 tie: the ids decide
    rows.append((rng.integers(0, tiny, V) | (rng.integers(0, 2, V) << 15)).astype(np.uint16))  # subnormals of both signs, and zeros
    for base, at, put in ((2, [0, V // 2, V - 1], [nan, nan | 0x8001, nan]), (0, [V // 2 + 1], [nan]), (1, [1, V - 2], [nan | 0x8000] * 2),
                          (2, [1, V - 2], [inf, inf | 0x8000]), (2, [3, V - 1], [inf, inf]), (2, rng.permutation(V)[:len(ext)], ext)):
        row = rows[base].copy()
        row[at] = put
        rows.append(row)
    return np.stack(rows)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", FORMS)
def test_order_and_special_values(dev, cap, form, dtype):
    """one element off alignment: head, octets and tail; the label in each, out of range and on a NaN, moved round from k to k"""
    rng = np.random.default_rng(17)
    for V in (cap[0] + 9, 17):
        rows = order_rows(rng, V, dtype)
        bits = rows.reshape(2, len(rows) // 2, V)
        places = [0, V // 2, V - 1, V, V // 2 + 1, 1, -1]
        for r, k in enumerate((0, 1, 5, 64) if form == "host" else (1, 5, 64)):
            labels = np.array([places[(i + r) % len(places)] for i in range(len(rows))], dtype=np.int64).reshape(2, -1)
            got = run(dev, cap, form, dtype, bits, np.arange(len(rows)), labels, k, shift=1, what="order")
            assert int(got["info"][3]) == 3  # the three rows with a NaN
            if k:
                assert got["top_id"][5].tolist() == (list(range(min(k, V))) + [-1] * k)[:k]  # all equal: the smallest ids
                assert got["top_id"][6].tolist() == got["top_id"][5].tolist()  # and so for the zeros of either sign
        run(dev, cap, form, dtype, bits, [8, 9, 2], None, 3, shift=1, what="no labels")


@pytest.mark.parametrize("dtype", DTYPES)
def test_against_the_float32_path(dev, cap, dtype):
    """the same values as float32 through swt_mlm_predict_dev: exact outputs and info equal, lse within the sum of the tolerances"""
    rng = np.random.default_rng(18)
    V = 2 * cap[0] + 9
    rows = order_rows(rng, V, dtype)
    bits, pos = rows.reshape(1, len(rows), V), np.arange(len(rows), dtype=np.uint64)
    labels = rng.integers(0, V, size=(1, len(rows))).astype(np.int32)
    code = dev.FILL_F16 if dtype == "f16" else dev.FILL_BF16
    got = call_dev(dev, "swt_mlm_predict16_dev", (code,), bits, bits.shape, pos, labels, 8, shift=1)
    ref = call_dev(dev, "swt_mlm_predict_dev", (), widen(bits, dtype), bits.shape, pos, labels, 8, shift=1)
    ref["lse"] = ref["lse"].astype(np.float64)
    agree(got, ref, lambda lse: lse_tol16(V, cap, lse) + F.lse_tol(V, dev.fill_capacity()[0], lse), ("float32 path", dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_fill_mask_and_mlm_scores_take_half_tensors(swt, dev, cap, ref_dir, dtype):
    """against the same call on .float(): ids, ranks and counts equal, lse, log-probabilities and loss within tolerance"""
    import torch
    tok = swt.FastWP()
    tok.load_resources(ref_dir + "/resources/tests/FastWordPiece")
    rng = np.random.default_rng(19)
    V, shape = cap[0] + 9, (3, 7)
    ids = rng.integers(0, 5, size=shape).astype(np.int64)
    ids[rng.random(shape) < 0.4] = tok.mask_id()
    labels = np.where(ids == tok.mask_id(), rng.integers(0, V, size=shape), -100).astype(np.int64)
    half = torch.from_numpy(F.normal_row(rng, 21 * V).reshape(3, 7, V)).cuda().to(torch.float16 if dtype == "f16" else torch.bfloat16)
    d_ids, d_labels = torch.from_numpy(ids).cuda(), torch.from_numpy(labels).cuda()
    # the two lse, each within its tolerance (|lse| < 16); logit - lse rounds once on each side (|logprob| < 32); exp within 1 ulp
    tol = lse_tol16(V, cap, 16.0) + F.lse_tol(V, dev.fill_capacity()[0], 16.0) + (2 * 32.0 + 4.0) * F.U
    for a, b in ((tok.fill_mask(d_ids, half, top_k=3), tok.fill_mask(d_ids, half.float(), top_k=3)),
                 (tok.mlm_scores(half, d_labels, top_k=2), tok.mlm_scores(half.float(), d_labels, top_k=2))):
        assert sorted(a) == sorted(b) and a["n_positions"] == int((ids == tok.mask_id()).sum()) > 0
        for key in a:
            va, vb = (v.cpu().numpy() if hasattr(v, "cpu") else v for v in (a[key], b[key]))
            if key in ("lse", "logprob", "score", "label_logprob", "loss", "perplexity"):
                assert np.asarray(va).dtype == np.asarray(vb).dtype and np.allclose(va, vb, rtol=tol, atol=tol), key
            else:
                assert np.array_equal(va, vb), key
    for call in (lambda x, i: tok.fill_mask(i, x), lambda x, i: tok.mlm_scores(x, i)):
        with pytest.raises(TypeError):
            call(half.cpu(), d_ids)  # on the host
        with pytest.raises(TypeError):
            call(half, ids)  # not of the ids' kind
