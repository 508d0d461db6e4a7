"""Model-ready batches on the device (csrc/swt_batch.hip): swt_batch_plan / swt_batch_rows, host and `_dev` forms, and
encode_batch of the four classes, against the Python model of tests/batch_cases.py (itself held to the `tokenizers` wheel's
recorded output by tests/test_batch_cases.py).  Every output is pre-filled with garbage and fenced by sentinel bytes; the `_dev`
runs use torch tensors on a side stream."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import batch_cases as B

pytestmark = pytest.mark.gpu

FENCE, GARBAGE, BACK = 0xEE, 0x5A, 32


@pytest.fixture(scope="module")
def dev(native):
    if native.device_count() < 1:
        pytest.fail("no HIP device")
    native.init(0)
    return native


@pytest.fixture(scope="module")
def caps(dev):
    return dev.batch_capacity()


class Fenced:
    """an output of `nbytes` bytes behind `front` fence bytes and before BACK more, garbage inside"""

    def __init__(self, nbytes, front):
        self.front, self.nbytes = front, nbytes
        self.host = np.full(front + nbytes + BACK, GARBAGE, dtype=np.uint8)
        self.host[:front] = FENCE
        self.host[front + nbytes:] = FENCE
        self.dev = None

    def to_device(self, torch):
        self.dev = torch.from_numpy(self.host.copy()).cuda()
        return self.dev.data_ptr() + self.front

    def host_ptr(self):
        return self.host.ctypes.data + self.front

    def body(self, dtype):
        a = self.dev.cpu().numpy() if self.dev is not None else self.host
        assert (a[:self.front] == FENCE).all() and (a[self.front + self.nbytes:] == FENCE).all(), "a fence was written"
        return a[self.front:self.front + self.nbytes].copy().view(dtype)


def run(dev, form, ids, off, s, cmap=None, pay=None, rows_cap=None, front=32, extras=True, want_rows=None):
    """swt_batch_plan + swt_batch_rows in one form -> (rc, dict of the rows written, raw bodies).  cmap = (map or None, n_map,
    flagged).  extras: out_sample, out_len and info are given.  The outputs have room for rows_cap rows (default: the rows
    needed); what lies behind the rows written must still be garbage."""
    table, n_map, flagged = (None, 1 << 31, False) if cmap is None else cmap
    n_rows = int(off.size) - 1
    spec = B.native_spec(dev, s)
    width, idb = s["width"], 8 if s["ids64"] else 4
    lib = dev.lib()
    # the plan
    if form == "host":
        row_base, longest = dev.batch_plan(off, spec)
    else:
        import torch
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt).copy()).cuda()
        stream = torch.cuda.Stream()
        d_off = up(off, np.int64)
        d_base = torch.full((n_rows + 1 + 2,), -1, dtype=torch.int64, device="cuda")
        d_pinfo = torch.full((2 + 2,), -1, dtype=torch.int64, device="cuda")
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            dev.check(lib.swt_batch_plan_dev(d_off.data_ptr(), n_rows, C.byref(spec), d_base.data_ptr(), d_pinfo.data_ptr(), stream.cuda_stream))
        stream.synchronize()
        hb, hi = d_base.cpu().numpy(), d_pinfo.cpu().numpy()
        assert (hb[n_rows + 1:] == -1).all() and (hi[2:] == -1).all()
        row_base, longest = hb[:n_rows + 1].view(np.uint64), int(hi[1])
        assert int(hi[0]) == int(row_base[-1])
    assert longest == (int(np.diff(off.astype(np.int64)).max()) if n_rows else 0)
    if want_rows is not None:
        assert row_base.tolist() == want_rows.tolist()
    need = int(row_base[-1])
    if rows_cap is None:
        rows_cap = need
    slots = rows_cap * width
    outs = {"ids": Fenced(slots * idb, front), "mask": Fenced(slots, front), "spans": Fenced(slots * 8, front), "word": Fenced(slots * 4, front),
            "sample": Fenced(rows_cap * 4, front), "len": Fenced(rows_cap * 4, front), "info": Fenced(24, 32)}
    use = {"ids": True, "mask": True, "spans": pay is not None, "word": pay is not None, "sample": extras, "len": extras, "info": extras}
    spans = word = None
    if pay is not None:
        spans, word = B.flat_payloads(pay)
    windows = s["windows"]
    if form == "host":
        p = {k: (C.c_void_p(o.host_ptr()) if use[k] else None) for k, o in outs.items()}
        cast = lambda a, t: a.ctypes.data_as(t) if a is not None and a.size else None
        rc = lib.swt_batch_rows(cast(ids, dev.u32p), cast(off, dev.u64p), n_rows, cast(table, dev.u32p), n_map, int(flagged),
                                cast(spans, dev.u32p) if pay is not None else None, cast(word, dev.u32p) if pay is not None else None,
                                C.byref(spec), cast(row_base, dev.u64p) if windows else None, rows_cap, p["ids"],
                                C.cast(p["mask"], dev.u8p), C.cast(p["spans"], dev.u32p) if pay is not None else None,
                                C.cast(p["word"], dev.u32p) if pay is not None else None, C.cast(p["sample"], dev.u32p) if extras else None,
                                C.cast(p["len"], dev.u32p) if extras else None, C.cast(p["info"], dev.u64p) if extras else None)
    else:
        pad4 = lambda a: np.concatenate([a, np.zeros(4, a.dtype)])
        d_ids = up(pad4(ids), np.int32)
        d_map = up(pad4(table), np.int32) if table is not None else None
        d_spans = up(pad4(spans.reshape(-1)), np.int32) if pay is not None else None
        d_word = up(pad4(word), np.int32) if pay is not None else None
        d_rb = up(row_base, np.int64)
        p = {k: (o.to_device(torch) if use[k] else None) for k, o in outs.items()}
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            rc = lib.swt_batch_rows_dev(d_ids.data_ptr(), d_off.data_ptr(), n_rows, d_map.data_ptr() if d_map is not None else None, n_map,
                                        int(flagged), d_spans.data_ptr() if pay is not None else None,
                                        d_word.data_ptr() if pay is not None else None, C.byref(spec), d_rb.data_ptr() if windows else None,
                                        rows_cap, p["ids"], p["mask"], p["spans"], p["word"], p["sample"], p["len"], p["info"],
                                        stream.cuda_stream)
        stream.synchronize()
    if rc == dev.ERR_CAPACITY:
        return rc, {"info": outs["info"].body(np.uint64)}, outs
    dev.check(rc)
    done = min(need, rows_cap)
    got = {}
    body = {"ids": outs["ids"].body(np.int64 if s["ids64"] else np.int32), "mask": outs["mask"].body(np.uint8),
            "spans": outs["spans"].body(np.uint32), "word": outs["word"].body(np.int32), "sample": outs["sample"].body(np.uint32),
            "len": outs["len"].body(np.uint32), "info": outs["info"].body(np.uint64)}
    per_row = {"ids": width, "mask": width, "spans": 2 * width, "word": width, "sample": 1, "len": 1}
    for k, n in per_row.items():
        garbage = np.frombuffer(bytes([GARBAGE]) * body[k].itemsize, dtype=body[k].dtype)[0]
        if use[k]:
            assert (body[k][done * n:] == garbage).all(), "%s: a row at or beyond the capacity was written" % k
            got[k] = body[k][:done * n]
        else:
            assert (body[k] == garbage).all(), "%s was not given and was written" % k
    res = {"input_ids": got["ids"].reshape(done, width), "attention_mask": got["mask"].reshape(done, width)}
    if pay is not None:
        res["offset_mapping"], res["word_ids"] = got["spans"].reshape(done, width, 2), got["word"].reshape(done, width)
    if extras:
        res["sample"], res["length"], res["info"] = got["sample"], got["len"], body["info"]
    else:
        assert (body["info"] == np.frombuffer(bytes([GARBAGE]) * 8, dtype=np.uint64)[0]).all()
    return rc, res, outs


def agree(res, want, rows=None, extras=True, info=True):
    rows = want["input_ids"].shape[0] if rows is None else rows
    keys = ["input_ids", "attention_mask"] + (["offset_mapping", "word_ids"] if "offset_mapping" in res else []) + \
           (["sample", "length"] if extras else [])
    for k in keys:
        assert res[k].shape[0] == rows
        if not np.array_equal(res[k], want[k][:rows]):
            bad = np.argwhere(np.asarray(res[k]) != np.asarray(want[k][:rows]))[0]
            raise AssertionError("%s differs first at %s: %r != %r" % (k, bad.tolist(), res[k][tuple(bad)], want[k][:rows][tuple(bad)]))
    if extras and info:
        assert res["info"].tolist() == [rows, want["lost"], want["n_unknown"]]


SPECIALS = [(None, None), (2, None), (None, 3), (2, 3)]


def seam_widths(cols):
    return [cols - 1, cols, cols + 1, 2 * cols - 1, 2 * cols + 1]


@pytest.mark.parametrize("which", range(5))
@pytest.mark.parametrize("form", ["host", "dev"])
def test_width_seams(dev, caps, form, which):
    """widths around one and two wavefront steps; row lengths around the window seams; cap - 1 and zero strides; every
    combination of specials; both padding sides; both id types; with and without payloads and the optional outputs"""
    width = seam_widths(caps[0])[which]
    case = 0
    for cls_id, sep_id in SPECIALS:
        cap = width - (cls_id is not None) - (sep_id is not None)
        for stride in (0, cap - 1, cap // 3):
            case += 1
            lengths = B.seam_lengths(cap, cap - stride) + [0, 3]
            rows, ids, off, pay = B.stream(lengths, seed=width * 100 + case)
            for windows in (False, True):
                s = B.spec(width, stride, windows, pad_left=bool(case & 1), ids64=bool(case & 2), cls_id=cls_id, sep_id=sep_id)
                use_pay = pay if (case + windows) % 2 else None
                extras = (case + windows) % 3 != 0
                want = B.expected_batch(rows, s, None, use_pay)
                _, res, _ = run(dev, form, ids, off, s, None, use_pay, extras=extras, want_rows=want["row_base"])
                agree(res, want, extras=extras)


@pytest.mark.parametrize("form", ["host", "dev"])
def test_small_widths_and_cap_one(dev, form):
    """cap = 1 (a window per token), widths that are no multiple of four, the widths at which a row's lane group doubles
    (cols_per_step / 2^k and one more), and outputs that are not aligned to the wide stores"""
    case = 0
    for width in (1, 2, 3, 4, 5, 7, 8, 9, 12, 16, 17, 32, 33, 64, 65, 128, 129):
        for cls_id, sep_id in SPECIALS:
            cap = width - (cls_id is not None) - (sep_id is not None)
            if cap < 1:
                continue
            for stride in sorted({0, cap - 1}):
                case += 1
                lengths = B.seam_lengths(cap, cap - stride) + [2, 9]
                rows, ids, off, pay = B.stream(lengths, seed=9000 + case)
                s = B.spec(width, stride, True, pad_left=bool(case & 1), ids64=bool(case & 4), cls_id=cls_id, sep_id=sep_id)
                want = B.expected_batch(rows, s, None, pay)
                for front in (32, 8):  # 8: no output is 16-byte aligned, the kernel takes its element-wise stores
                    _, res, _ = run(dev, form, ids, off, s, None, pay, front=front, want_rows=want["row_base"])
                    agree(res, want)


@pytest.mark.parametrize("which", range(5))
@pytest.mark.parametrize("form", ["host", "dev"])
def test_row_count_seams(dev, caps, form, which):
    """n_rows around the scan groups of the plan; windows and truncation"""
    group = caps[1]
    n_rows = [1, group - 1, group, group + 1, 2 * group + 1][which]
    rng = np.random.RandomState(n_rows)
    lengths = rng.choice([0, 1, 5, 6, 7, 10, 11, 12, 25], size=n_rows).tolist()
    rows, ids, off, pay = B.stream(lengths, seed=n_rows)
    for windows in (True, False):
        s = B.spec(8, 2, windows, cls_id=2, sep_id=3)
        want = B.expected_batch(rows, s, None, pay)
        _, res, _ = run(dev, form, ids, off, s, None, pay, want_rows=want["row_base"])
        agree(res, want)


@pytest.mark.parametrize("form", ["host", "dev"])
def test_map_edges(dev, form):
    """ids at n_map - 1 and n_map, an entry of 0xFFFFFFFF, SWT_BPE_CONT ids through the second half of a flagged map, the identity
    map and its bound; info[2] counts every slot that went to unk_id -- a token in two overlapping windows twice"""
    n_map = 50
    rng = np.random.RandomState(5)
    flat = (1000 + rng.permutation(n_map)).astype(np.uint32)
    flat[7] = B.NONE
    both = np.concatenate([flat, (2000 + rng.permutation(n_map)).astype(np.uint32)])
    both[n_map + 9] = B.NONE
    edge = [n_map - 1, n_map, n_map + 1, 7, 9, 0, 0x7FFFFFFF]
    row = edge + [x | B.CONT for x in edge] + [int(x) for x in rng.randint(0, n_map, size=11)]
    rows = [row, [], [n_map - 1], [n_map | B.CONT, 7 | B.CONT]]
    ids = np.array([x for r in rows for x in r], dtype=np.uint32)
    off = np.array(np.cumsum([0] + [len(r) for r in rows]), dtype=np.uint64)
    for cmap in ((both, n_map, True), (flat, n_map, False), (None, n_map, False), None):
        for windows, stride in ((False, 0), (True, 0), (True, 3)):
            s = B.spec(8, stride, windows, unk_id=77, pad_id=78, cls_id=2, sep_id=3)
            want = B.expected_batch(rows, s, cmap)
            assert cmap is None or want["n_unknown"] > 0
            _, res, _ = run(dev, form, ids, off, s, cmap)
            agree(res, want)


def test_capacity(dev):
    """rows_cap one short: the host form answers SWT_ERR_CAPACITY with the rows needed and writes nothing; the `_dev` form writes
    the rows below rows_cap and leaves everything behind them alone (run() checks the garbage and the fences)"""
    lengths = [3, 20, 0, 7, 13]
    rows, ids, off, pay = B.stream(lengths, seed=77)
    for windows in (True, False):
        s = B.spec(8, 1, windows, cls_id=2, sep_id=3)
        want = B.expected_batch(rows, s, None, pay)
        need = want["input_ids"].shape[0]
        rc, res, outs = run(dev, "host", ids, off, s, None, pay, rows_cap=need - 1)
        assert rc == dev.ERR_CAPACITY and res["info"].tolist() == [need, 0, 0]
        assert (outs["ids"].body(np.uint8) == GARBAGE).all() and (outs["mask"].body(np.uint8) == GARBAGE).all()
        rc, res, _ = run(dev, "dev", ids, off, s, None, pay, rows_cap=need - 1)
        assert rc == 0
        agree(res, want, rows=need - 1, info=False)
        assert int(res["info"][0]) == need - 1
        # room to spare: the rows behind the last one stay as they were
        rc, res, _ = run(dev, "dev", ids, off, s, None, pay, rows_cap=need + 3)
        agree(res, want)


# ---- through the classes

def _tokenizer(swt, ref_dir, cls):
    tok = getattr(swt, cls)()
    tok.load_resources(os.path.join(ref_dir, "resources/pretrained", "FastBPE" if "BPE" in cls else "FastWordPiece"))
    return tok


def _to_numpy(res):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in res.items()}


_anchor_cache = {}


def _anchor(swt, ref_dir, corpora, cls):
    """-> (tokenizer, texts, per text the dense ids of the expected token strings)"""
    if cls not in _anchor_cache:
        tok = _tokenizer(swt, ref_dir, cls)
        texts = list(corpora["pan"])
        if cls.startswith("Fast"):
            strings = corpora["pan_tokens"]["FastBPE" if "BPE" in cls else "FastWordPiece"]
        else:
            # the reference recorded the Fast classes only: the Naive classes are held to their own token strings, which the
            # encode and span tests hold to the reference; a text NaiveWP does not return from is an empty row
            texts = texts[:300]
            status = tok.encode_ids_batch(texts)[2] if "WP" in cls else np.zeros(len(texts), dtype=np.uint8)
            good = [t for t, st in zip(texts, status) if not st]
            it = iter(tok.tokenize_batch(good))
            strings = [next(it) if not st else [] for st in status]
        assert len(strings) == len(texts)
        _anchor_cache[cls] = (tok, texts, [[tok.token_to_id(t) for t in row] for row in strings])
    return _anchor_cache[cls]


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("cls", ["FastBPE", "FastWP", "NaiveBPE", "NaiveWP"])
def test_encode_batch_anchored_on_the_reference(swt, dev, ref_dir, corpora, cls, device):
    """the rows of pan_tadeusz encoded by the product against the model over the REFERENCE's token strings (the Fast classes;
    989 rows) mapped through token_to_id: width 16 for BPE (cap 14: about a tenth of the rows window), 32 for WordPiece (cap 30:
    the median); truncating, and windowed with stride 0 and 4"""
    tok, texts, dense = _anchor(swt, ref_dir, corpora, cls)
    if cls.startswith("Fast"):
        assert len(texts) == 989
    sp = tok.special_ids()
    assert sp["unk"] not in {d for row in dense for d in row} or not cls.startswith("Fast")
    width = 16 if "BPE" in cls else 32
    for windows, stride in ((False, 0), (True, 0), (True, 4)):
        s = B.spec(width, stride, windows, pad_id=sp["pad"], unk_id=sp["unk"], cls_id=sp["cls"], sep_id=sp["sep"])
        want = B.expected_batch(dense, s)
        got = _to_numpy(tok.encode_batch(texts, max_length=width, stride=stride, padding="max_length", return_overflowing=windows, device=device))
        assert np.array_equal(got["input_ids"], want["input_ids"])
        assert np.array_equal(got["attention_mask"], want["attention_mask"])
        assert np.array_equal(got["length"], want["length"])
        assert got["n_unknown"] == 0 or not cls.startswith("Fast")
        if windows:
            assert np.array_equal(got["overflow_to_sample_mapping"], want["sample"])
            assert want["input_ids"].shape[0] > len(texts)  # some rows did window
        else:
            assert "overflow_to_sample_mapping" not in got


@pytest.mark.parametrize("cls", ["FastBPE", "NaiveBPE", "NaiveWP", "FastWP"])
def test_encode_batch_options(swt, dev, ref_dir, corpora, cls):
    """padding="longest" with pad_to_multiple_of, left padding, no specials, int64; return_offsets on train-5K's first 200
    sentences against the class's span call rearranged by the model; device on and off give equal arrays"""
    tok = _tokenizer(swt, ref_dir, cls)
    texts = list(corpora["t5k"])[:200]
    if "WP" in cls:  # a text the reference does not return from has no spans: the span calls raise on it
        status = (tok.encode_ids_batch(texts))[2]
        texts = [t for t, st in zip(texts, status) if not st]
        assert len(texts) > 150
    got = tok._batch_encode_spans(texts)
    raw, off, spans, word = got[0], got[1], got[-2], got[-1]
    rows = [[int(x) for x in raw[int(off[i]):int(off[i + 1])]] for i in range(len(texts))]
    pay = ([spans[int(off[i]):int(off[i + 1])].tolist() for i in range(len(texts))],
           [word[int(off[i]):int(off[i + 1])].tolist() for i in range(len(texts))])
    voc = tok._batch_vocabulary()
    sp = tok.special_ids()
    longest = max(len(r) for r in rows)
    # longest, rounded up to a multiple of 8
    s = B.spec(-(-(longest + 2) // 8) * 8, pad_id=sp["pad"], unk_id=sp["unk"], cls_id=sp["cls"], sep_id=sp["sep"])
    want = B.expected_batch(rows, s, (voc.cmap, voc.n_map, voc.flagged), pay)
    for device in (False, True):
        got = _to_numpy(tok.encode_batch(texts, pad_to_multiple_of=8, return_offsets=True, device=device))
        assert got["input_ids"].shape == (len(texts), s["width"]) and s["width"] % 8 == 0
        for k in ("input_ids", "attention_mask", "length", "offset_mapping", "word_ids"):
            assert np.array_equal(got[k], want[k]), (k, device)
        assert got["n_unknown"] == want["n_unknown"]
    # windows, left padding, no specials, 64-bit ids, a width cut by max_length
    s = B.spec(12, 5, True, pad_left=True, ids64=True, pad_id=sp["pad"], unk_id=sp["unk"])
    want = B.expected_batch(rows, s, (voc.cmap, voc.n_map, voc.flagged), pay)
    for device in (False, True):
        got = _to_numpy(tok.encode_batch(texts, max_length=12, stride=5, add_special_tokens=False, padding_side="left",
                                         return_overflowing=True, return_offsets=True, int64=True, device=device))
        assert got["input_ids"].dtype == np.int64
        for k in ("input_ids", "attention_mask", "length", "offset_mapping", "word_ids"):
            assert np.array_equal(got[k], want[k]), (k, device)
        assert np.array_equal(got["overflow_to_sample_mapping"], want["sample"])
    with pytest.raises(ValueError):
        tok.encode_batch(texts[:2], return_overflowing=True)
    with pytest.raises(TypeError):
        tok.encode_batch("not a list")
