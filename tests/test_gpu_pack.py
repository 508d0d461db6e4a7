"""Packed batches on the device (csrc/swt_pack.hip): swt_pack_plan / swt_pack_rows, host and `_dev` forms, both modes, and
encode_batch(packing=...) of the four classes, against the Python model of tests/pack_cases.py (held to expected_batch and to
the properties of a packing by tests/test_pack_cases.py).  Every output is pre-filled with garbage and fenced by sentinel bytes;
the `_dev` runs use torch tensors on a side stream (Fenced: tests/test_gpu_model_batches.py)."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import batch_cases as B
from tests import pack_cases as K
from tests.test_gpu_model_batches import GARBAGE, Fenced

pytestmark = pytest.mark.gpu

MODES = [K.WHOLE, K.SPLIT, K.SPLIT | K.DROP_LAST]
SPECIALS = [(None, None), (2, None), (None, 3), (2, 3)]
OPTIONAL = ("pos", "seg", "doc", "len", "info")


@pytest.fixture(scope="module")
def dev(native):
    if native.device_count() < 1:
        pytest.fail("no HIP device")
    native.init(0)
    return native


@pytest.fixture(scope="module")
def caps(dev):
    return dev.pack_capacity()


def plan(dev, form, off, s, mode):
    """swt_pack_plan in one form -> (slot, row_first, info[4])"""
    n_rows = int(off.size) - 1
    spec, m = B.native_spec(dev, s), K.native_mode(dev, mode)
    if form == "host":
        return dev.pack_plan(off, spec, m)
    import torch
    stream = torch.cuda.Stream()
    d_off = torch.from_numpy(off.view(np.int64).copy()).cuda()
    d_slot = torch.full((n_rows + 1 + 2,), -1, dtype=torch.int64, device="cuda")
    d_first = torch.full((n_rows + 1 + 2,), -1, dtype=torch.int64, device="cuda")
    d_info = torch.full((4 + 2,), -1, dtype=torch.int64, device="cuda")
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        dev.check(dev.lib().swt_pack_plan_dev(d_off.data_ptr(), n_rows, C.byref(spec), m, d_slot.data_ptr(), d_first.data_ptr(),
                                              d_info.data_ptr(), stream.cuda_stream))
    stream.synchronize()
    hs, hf, hi = d_slot.cpu().numpy(), d_first.cpu().numpy(), d_info.cpu().numpy()
    assert (hs[n_rows + 1:] == -1).all() and (hf[n_rows + 1:] == -1).all() and (hi[4:] == -1).all(), "the plan wrote behind its arrays"
    return hs[:n_rows + 1].view(np.uint64), hf[:n_rows + 1].view(np.uint64), hi[:4].view(np.uint64)


def run(dev, form, ids, off, s, mode, cmap=None, rows_cap=None, front=32, skip=(), want=None):
    """swt_pack_plan + swt_pack_rows in one form -> (rc, dict of the rows written, raw bodies).  cmap = (map or None, n_map,
    flagged).  skip: the optional outputs that are not given.  want: the model's result, to which the plan is held.  The outputs
    have room for rows_cap rows (default: the rows needed); what lies behind the rows written must still be garbage."""
    table, n_map, flagged = (None, 1 << 31, False) if cmap is None else cmap
    n_rows = int(off.size) - 1
    spec, m = B.native_spec(dev, s), K.native_mode(dev, mode)
    width, idb = s["width"], 8 if s["ids64"] else 4
    lib = dev.lib()
    slot, row_first, pinfo = plan(dev, form, off, s, mode)
    if want is not None:
        assert slot.tolist() == want["slot"].tolist()
        assert row_first.tolist() == want["row_first"].tolist()
        assert pinfo.tolist() == [want["rows"], want["longest"], 0, want["total"]]
    need = int(pinfo[0])
    if rows_cap is None:
        rows_cap = need
    slots = rows_cap * width
    outs = {"ids": Fenced(slots * idb, front), "mask": Fenced(slots, front), "pos": Fenced(slots * 4, front), "seg": Fenced(slots * 4, front),
            "doc": Fenced(slots * 4, front), "len": Fenced(rows_cap * 4, front), "info": Fenced(24, 32)}
    use = {k: k not in skip for k in outs}
    if form == "host":
        p = {k: (C.c_void_p(o.host_ptr()) if use[k] else None) for k, o in outs.items()}
        cast = lambda a, t: a.ctypes.data_as(t) if a is not None and a.size else None
        opt = lambda k, t: C.cast(p[k], t) if use[k] else None
        rc = lib.swt_pack_rows(cast(ids, dev.u32p), cast(off, dev.u64p), n_rows, cast(table, dev.u32p), n_map, int(flagged), C.byref(spec), m,
                               cast(slot, dev.u64p), cast(row_first, dev.u64p), rows_cap, p["ids"], C.cast(p["mask"], dev.u8p),
                               opt("pos", dev.u32p), opt("seg", dev.u32p), opt("doc", dev.u32p), opt("len", dev.u32p), opt("info", dev.u64p))
    else:
        import torch
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt).copy()).cuda()
        pad4 = lambda a: np.concatenate([a, np.zeros(4, a.dtype)])
        stream = torch.cuda.Stream()
        d_ids, d_off = up(pad4(ids), np.int32), up(off, np.int64)
        d_map = up(pad4(table), np.int32) if table is not None else None
        d_slot, d_first = up(slot, np.int64), up(row_first, np.int64)
        p = {k: (o.to_device(torch) if use[k] else None) for k, o in outs.items()}
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            rc = lib.swt_pack_rows_dev(d_ids.data_ptr(), d_off.data_ptr(), n_rows, d_map.data_ptr() if d_map is not None else None, n_map,
                                       int(flagged), C.byref(spec), m, d_slot.data_ptr(), d_first.data_ptr(), rows_cap, p["ids"], p["mask"],
                                       p["pos"], p["seg"], p["doc"], p["len"], p["info"], stream.cuda_stream)
        stream.synchronize()
    if rc == dev.ERR_CAPACITY:
        return rc, {"info": outs["info"].body(np.uint64)}, outs
    dev.check(rc)
    done = min(need, rows_cap)
    body = {"ids": outs["ids"].body(np.int64 if s["ids64"] else np.int32), "mask": outs["mask"].body(np.uint8),
            "pos": outs["pos"].body(np.uint32), "seg": outs["seg"].body(np.uint32), "doc": outs["doc"].body(np.uint32),
            "len": outs["len"].body(np.uint32), "info": outs["info"].body(np.uint64)}
    per_row = {"ids": width, "mask": width, "pos": width, "seg": width, "doc": width, "len": 1}
    got = {}
    for k, n in per_row.items():
        garbage = np.frombuffer(bytes([GARBAGE]) * body[k].itemsize, dtype=body[k].dtype)[0]
        if use[k]:
            assert (body[k][done * n:] == garbage).all(), "%s: a row at or beyond the capacity was written" % k
            got[k] = body[k][:done * n]
        else:
            assert (body[k] == garbage).all(), "%s was not given and was written" % k
    res = {"input_ids": got["ids"].reshape(done, width), "attention_mask": got["mask"].reshape(done, width)}
    for k, name in (("pos", "position_ids"), ("seg", "sequence_ids"), ("doc", "sample_ids")):
        if use[k]:
            res[name] = got[k].reshape(done, width)
    if use["len"]:
        res["length"] = got["len"]
    if use["info"]:
        res["info"] = body["info"]
    else:
        assert (body["info"] == np.frombuffer(bytes([GARBAGE]) * 8, dtype=np.uint64)[0]).all()
    return rc, res, outs


def agree(res, want, rows=None, info=True):
    rows = want["rows"] if rows is None else rows
    for k in ("input_ids", "attention_mask", "position_ids", "sequence_ids", "sample_ids", "length"):
        if k not in res:
            continue
        assert res[k].shape[0] == rows, k
        if not np.array_equal(res[k], want[k][:rows]):
            bad = np.argwhere(np.asarray(res[k]) != np.asarray(want[k][:rows]))[0]
            raise AssertionError("%s differs first at %s: %r != %r" % (k, bad.tolist(), res[k][tuple(bad)], want[k][:rows][tuple(bad)]))
    if info and "info" in res:
        assert res["info"].tolist() == [rows, want["lost"], want["n_unknown"]]


def both(dev, form, rows, ids, off, s, mode, cmap=None, **kw):
    want = K.expected_pack(rows, s, mode, cmap)
    _, res, _ = run(dev, form, ids, off, s, mode, cmap, want=want, **kw)
    agree(res, want)
    return want


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("form", ["host", "dev"])
def test_widths_and_specials(dev, form, mode):
    """widths that are no multiple of four, one lane group and several steps of a wavefront (129, 130 in WHOLE: rows over cap);
    every combination of specials; both id types; outputs aligned to 16 bytes and off by 4 (8 for 64-bit ids)"""
    case = 0
    for width in (3, 4, 5, 8, 64, 129, 130):
        for cls_id, sep_id in SPECIALS:
            if width - (cls_id is not None) - (sep_id is not None) < 1:
                continue
            case += 1
            ids64 = bool(case & 1)
            lengths = K.random_lengths(37, width, 100 * width + case)
            rows, ids, off, _ = B.stream(lengths, seed=case)
            s = B.spec(width, ids64=ids64, pad_id=7, unk_id=8, cls_id=cls_id, sep_id=sep_id)
            want = K.expected_pack(rows, s, mode)
            for front in (32, 40 if ids64 else 36):
                _, res, _ = run(dev, form, ids, off, s, mode, front=front, want=want)
                agree(res, want)


@pytest.mark.parametrize("form", ["host", "dev"])
def test_optional_outputs(dev, form):
    """each optional output NULL once, and all of them at once"""
    rows, ids, off, _ = B.stream(K.random_lengths(20, 8, 3), seed=3)
    s = B.spec(8, cls_id=2, sep_id=3)
    for mode in (K.WHOLE, K.SPLIT):
        want = K.expected_pack(rows, s, mode)
        for skip in [(k,) for k in OPTIONAL] + [OPTIONAL]:
            _, res, _ = run(dev, form, ids, off, s, mode, skip=skip, want=want)
            agree(res, want)
            assert not any(name in res for name, k in (("position_ids", "pos"), ("length", "len"), ("info", "info")) if k in skip)


@pytest.mark.parametrize("which", range(6))
@pytest.mark.parametrize("form", ["host", "dev"])
def test_row_count_seams(dev, caps, form, which):
    """n_rows = 0, 1 and around the scan groups and the orbit groups of the plan"""
    for group in sorted(set(g for g in caps[1:] if g)):
        n_rows = [0, 1, group - 1, group, group + 1, 2 * group + 1][which]
        lengths = K.random_lengths(n_rows, 8, n_rows + 5)
        rows, ids, off, _ = B.stream(lengths, seed=n_rows)
        for mode in MODES:
            both(dev, form, rows, ids, off, B.spec(8, cls_id=2, sep_id=3), mode)
        both(dev, form, rows, ids, off, B.spec(5), K.WHOLE)


@pytest.mark.parametrize("form", ["host", "dev"])
def test_full_rows_and_rows_over_cap(dev, form):
    """a segment of exactly the width, rows of cap - 1, cap, cap + 1 and many more tokens, and what follows them"""
    for width, (cls_id, sep_id) in ((8, (2, 3)), (8, (None, None)), (64, (2, None))):
        cap = width - (cls_id is not None) - (sep_id is not None)
        lengths = [cap, 1, cap - 1, 1, cap + 1, 0, 3 * cap + 2, 2, cap, cap]
        rows, ids, off, _ = B.stream(lengths, seed=width)
        s = B.spec(width, cls_id=cls_id, sep_id=sep_id)
        want = both(dev, form, rows, ids, off, s, K.WHOLE)
        assert want["lost"] == 2 and (want["length"] == width).sum() >= 4
        both(dev, form, rows, ids, off, s, K.SPLIT)


@pytest.mark.parametrize("form", ["host", "dev"])
def test_empty_rows_with_specials(dev, caps, form):
    """nothing but empty texts with [CLS] and [SEP]: 256 segments per packed row at width 512, packed rows across the seams of
    the plan's groups"""
    n_rows = 2 * max(caps[1:]) + 300
    rows, ids, off, _ = B.stream([0] * n_rows, seed=1)
    s = B.spec(512, cls_id=2, sep_id=3)
    want = both(dev, form, rows, ids, off, s, K.WHOLE)
    assert want["rows"] == -(-n_rows // 256) and int(want["sequence_ids"][0, -1]) == 255
    both(dev, form, rows, ids, off, s, K.SPLIT)


@pytest.mark.parametrize("form", ["host", "dev"])
def test_empty_rows_without_specials(dev, form):
    """T = 0: one row of padding in WHOLE, no row in SPLIT"""
    for n_rows in (1, 5, 1500):
        rows, ids, off, _ = B.stream([0] * n_rows, seed=1)
        s = B.spec(8)
        want = both(dev, form, rows, ids, off, s, K.WHOLE)
        assert want["rows"] == 1 and not want["attention_mask"].any()
        for mode in (K.SPLIT, K.SPLIT | K.DROP_LAST):
            assert both(dev, form, rows, ids, off, s, mode)["rows"] == 0


@pytest.mark.parametrize("form", ["host", "dev"])
def test_zero_length_rows_between_full_ones(dev, form):
    """5,000 rows of no column between two rows: one packed row spans several groups of the plan"""
    for head in (8, 5):  # the first packed row full, and with room to spare
        rows, ids, off, _ = B.stream([head] + [0] * 5000 + [8, 2], seed=head)
        s = B.spec(8)
        want = both(dev, form, rows, ids, off, s, K.WHOLE)
        assert want["rows"] == 3 and want["row_first"][:4].tolist() == [0, 5001, 5002, 5003]
        both(dev, form, rows, ids, off, s, K.SPLIT)


@pytest.mark.parametrize("form", ["host", "dev"])
def test_split_long_rows_and_drop_last(dev, form):
    """a row longer than three widths (more packed rows than source rows); T a multiple of the width, one more and one less"""
    s = B.spec(8, cls_id=2, sep_id=3)
    for lengths in ([27], [1, 30, 0, 2], [6, 6], [6, 7], [6, 5], [14], [2]):
        rows, ids, off, _ = B.stream(lengths, seed=len(lengths))
        for mode in (K.SPLIT, K.SPLIT | K.DROP_LAST):
            want = both(dev, form, rows, ids, off, s, mode)
            assert want["rows"] == (want["total"] // 8 if mode & K.DROP_LAST else -(-want["total"] // 8))


def test_capacity(dev):
    """rows_cap one short: the host form answers SWT_ERR_CAPACITY with the rows needed and writes nothing; the `_dev` form writes
    the rows below rows_cap and leaves everything behind them alone (run() checks the garbage and the fences)"""
    rows, ids, off, _ = B.stream([3, 20, 0, 7, 13, 1, 1, 6], seed=77)
    s = B.spec(8, cls_id=2, sep_id=3)
    for mode in MODES:
        want = K.expected_pack(rows, s, mode)
        need = want["rows"]
        assert need >= 2
        rc, res, outs = run(dev, "host", ids, off, s, mode, rows_cap=need - 1)
        assert rc == dev.ERR_CAPACITY and res["info"].tolist() == [need, 0, 0]
        assert (outs["ids"].body(np.uint8) == GARBAGE).all() and (outs["mask"].body(np.uint8) == GARBAGE).all()
        rc, res, _ = run(dev, "dev", ids, off, s, mode, rows_cap=need - 1)
        assert rc == 0
        agree(res, want, rows=need - 1, info=False)
        assert int(res["info"][0]) == need - 1
        rc, res, _ = run(dev, "dev", ids, off, s, mode, rows_cap=need + 3)  # room to spare: the rows behind stay as they were
        agree(res, want)


@pytest.mark.parametrize("form", ["host", "dev"])
def test_map_edges(dev, form):
    """ids at n_map - 1 and n_map, an entry of 0xFFFFFFFF, flagged ids through the second half of the map, the identity and its
    bound; info[2] counts every column that went to unk_id"""
    n_map = 50
    rng = np.random.RandomState(5)
    flat = (1000 + rng.permutation(n_map)).astype(np.uint32)
    flat[7] = B.NONE
    two = np.concatenate([flat, (2000 + rng.permutation(n_map)).astype(np.uint32)])
    two[n_map + 9] = B.NONE
    edge = [n_map - 1, n_map, n_map + 1, 7, 9, 0, 0x7FFFFFFF]
    row = edge + [x | B.CONT for x in edge] + [int(x) for x in rng.randint(0, n_map, size=11)]
    rows = [row, [], [n_map - 1], [n_map | B.CONT, 7 | B.CONT]]
    ids = np.array([x for r in rows for x in r], dtype=np.uint32)
    off = np.array(np.cumsum([0] + [len(r) for r in rows]), dtype=np.uint64)
    for cmap in ((two, n_map, True), (flat, n_map, False), (None, n_map, False), None):
        for mode in MODES:
            s = B.spec(8, unk_id=77, pad_id=78, cls_id=2, sep_id=3)
            want = both(dev, form, rows, ids, off, s, mode, cmap)
            assert cmap is None or want["n_unknown"] > 0


def test_refused(dev):
    """what the header says is SWT_ERR_INVALID, in the plan and the row calls, and what the host forms check before the device"""
    lib = dev.lib()
    rows, ids, off, _ = B.stream([3, 2, 4], seed=1)
    good = B.spec(8, cls_id=2, sep_id=3)
    slot, row_first, _ = dev.pack_plan(off, B.native_spec(dev, good), dev.PACK_WHOLE)

    def calls(s, mode, slot=slot, row_first=row_first, off=off):
        spec = B.native_spec(dev, s)
        out = np.zeros(64 * s["width"] + 64, dtype=np.int64)
        u64 = lambda a: a.ctypes.data_as(dev.u64p)
        yield lib.swt_pack_plan(u64(off), 3, C.byref(spec), mode, u64(np.zeros(4, np.uint64)), u64(np.zeros(4, np.uint64)),
                                u64(np.zeros(4, np.uint64)))
        yield lib.swt_pack_rows(ids.ctypes.data_as(dev.u32p), u64(off), 3, None, 1 << 31, 0, C.byref(spec), mode, u64(slot), u64(row_first), 64,
                                out.ctypes.data_as(C.c_void_p), np.zeros(out.size, np.uint8).ctypes.data_as(dev.u8p), None, None, None, None, None)

    assert list(calls(good, dev.PACK_WHOLE)) == [0, 0]
    bad = [(dict(good, stride=1), dev.PACK_WHOLE), (dict(good, windows=True), dev.PACK_WHOLE), (dict(good, pad_left=True), dev.PACK_SPLIT),
           (dict(good, width=2), dev.PACK_WHOLE), (dict(good, width=2), dev.PACK_SPLIT), (dict(good, pad_id=B.NONE), dev.PACK_WHOLE),
           (dict(good, unk_id=B.NONE), dev.PACK_SPLIT), (good, 0), (good, dev.PACK_WHOLE | dev.PACK_SPLIT),
           (good, dev.PACK_WHOLE | dev.PACK_DROP_LAST), (good, dev.PACK_DROP_LAST), (good, 8 | dev.PACK_SPLIT)]
    for s, mode in bad:
        assert list(calls(s, mode)) == [dev.ERR_INVALID] * 2, (s, mode)
    spec = B.native_spec(dev, good)
    spec.flags |= 64
    u64 = lambda a: a.ctypes.data_as(dev.u64p)
    assert lib.swt_pack_plan(u64(off), 3, C.byref(spec), dev.PACK_WHOLE, u64(np.zeros(4, np.uint64)), u64(np.zeros(4, np.uint64)),
                             u64(np.zeros(4, np.uint64))) == dev.ERR_INVALID
    # the host forms: offsets that decrease; a slot or a row_first that is not the plan; 2^32 rows
    down = np.array([0, 3, 2, 6], dtype=np.uint64)
    assert list(calls(good, dev.PACK_WHOLE, off=down)) == [dev.ERR_INVALID] * 2
    for k in range(4):
        wrong = slot.copy()
        wrong[k] += 1
        assert list(calls(good, dev.PACK_WHOLE, slot=wrong))[1] == dev.ERR_INVALID
        wrong = row_first.copy()
        wrong[k] += 1
        assert list(calls(good, dev.PACK_WHOLE, row_first=wrong))[1] == dev.ERR_INVALID
    assert list(calls(good, dev.PACK_SPLIT))[1] == dev.ERR_INVALID  # the WHOLE plan is not the SPLIT plan of these offsets
    spec = B.native_spec(dev, good)
    assert lib.swt_pack_plan_dev(1, 1 << 32, C.byref(spec), dev.PACK_WHOLE, 1, 1, 1, None) == dev.ERR_INVALID
    with pytest.raises(dev.SwtError):
        dev.check(lib.swt_pack_plan(None, 0, C.byref(spec), dev.PACK_WHOLE, None, None, None))


# ---- through the classes

def _tokenizer(swt, ref_dir, cls):
    tok = getattr(swt, cls)()
    tok.load_resources(os.path.join(ref_dir, "resources/pretrained", "FastBPE" if "BPE" in cls else "FastWordPiece"))
    return tok


_model_cache = {}


def _model(swt, ref_dir, corpora, cls):
    """-> (tokenizer, texts, per text its raw ids from encode_ids_batch)"""
    if cls not in _model_cache:
        tok = _tokenizer(swt, ref_dir, cls)
        texts = list(corpora["pan"])
        if not cls.startswith("Fast"):
            texts = texts[:300]
        got = tok.encode_ids_batch(texts)
        raw, off = got[0], got[1]
        _model_cache[cls] = (tok, texts, [[int(x) for x in raw[int(off[i]):int(off[i + 1])]] for i in range(len(texts))])
    return _model_cache[cls]


ROWS_OF_THE_ISSUE = {("FastBPE", 64): 227, ("FastWP", 64): 664, ("FastWP", 128): 278}


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("cls", ["FastBPE", "FastWP", "NaiveBPE", "NaiveWP"])
def test_encode_batch_packing(swt, dev, ref_dir, corpora, cls, device):
    """encode_batch(packing=...) on pan_tadeusz at widths 64 and 128 against the model applied to encode_ids_batch; the row
    counts of next-fit packing computed from the reference's token lists"""
    tok, texts, rows = _model(swt, ref_dir, corpora, cls)
    voc, sp = tok._batch_vocabulary(), tok.special_ids()
    for width in (64, 128):
        for packing, drop_last, mode in (("whole", False, K.WHOLE), ("split", False, K.SPLIT), ("split", True, K.SPLIT | K.DROP_LAST)):
            s = B.spec(width, pad_id=sp["pad"], unk_id=sp["unk"], cls_id=sp["cls"], sep_id=sp["sep"])
            want = K.expected_pack(rows, s, mode, (voc.cmap, voc.n_map, voc.flagged))
            got = tok.encode_batch(texts, max_length=width, packing=packing, drop_last=drop_last, device=device)
            got = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in got.items()}
            assert got["input_ids"].shape == (want["rows"], width)
            for k in ("input_ids", "attention_mask", "position_ids", "length"):
                assert np.array_equal(got[k], want[k]), (k, width, packing)
            for k in ("sequence_ids", "sample_ids"):
                assert np.array_equal(got[k], want[k].view(np.int32)), (k, width, packing)
            assert got["n_unknown"] == want["n_unknown"] and got["n_truncated"] == want["lost"]
            n = len(texts)
            assert np.array_equal(got["segment_row"], want["slot"][:n] // width) and np.array_equal(got["segment_col"], want["slot"][:n] % width)
            assert np.array_equal(got["segment_length"], want["seg"])
            shown = min(want["total"], want["rows"] * width)
            assert got["density"] == pytest.approx(shown / (want["rows"] * width), abs=1e-12)
            if mode == K.WHOLE and (cls, width) in ROWS_OF_THE_ISSUE:
                assert want["rows"] == ROWS_OF_THE_ISSUE[(cls, width)]
    with pytest.raises(ValueError):
        tok.encode_batch(texts[:4], packing="whole")  # no max_length
    for bad in ({"text_pairs": texts[:4]}, {"return_overflowing": True}, {"stride": 2}, {"return_offsets": True}, {"padding_side": "left"},
                {"drop_last": True}, {"packing": "best"}):
        with pytest.raises(ValueError):
            tok.encode_batch(texts[:4], **dict({"max_length": 16, "packing": "whole", "device": device}, **bad))
    got = tok.encode_batch(texts[:9], max_length=30, pad_to_multiple_of=8, packing="split", add_special_tokens=False, int64=True, device=device)
    assert tuple(got["input_ids"].shape)[1] == 32 and "int64" in str(got["input_ids"].dtype)
