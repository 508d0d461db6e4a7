"""swt_mlm_mask / swt_mlm_mask_dev on the GPU against the NumPy model (tests/mlm_cases.py), element by element and `info`
included, at the smallest shapes that reach each seam of the kernel: the scalar and the wide path, one, two and three steps a
row, rows that share a wavefront and a last wavefront that is partly dead, words laid across every quad, lane and step seam.
Every `_dev` call runs with fences before and after each output."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import mlm_cases as M

pytestmark = pytest.mark.gpu

FENCE, GARBAGE, FRONT, BACK = 0xEE, 0x5A, 64, 64


@pytest.fixture(scope="module")
def dev(native):
    if native.device_count() < 1:
        pytest.fail("no HIP device")
    native.init(0)
    return native


@pytest.fixture(scope="module")
def cols(dev):
    return dev.mlm_capacity()[0]


def native_spec(dev, s, ids64):
    return dev.mlm_spec(s["n_class"], s["mask_id"], s["select_below"], s["mask_below"], s["random_below"], s["seed"], s["epoch"],
                        s["whole_word"], ids64)


def run(dev, form, ids, cls_tab, rand_ids, s, selected=True, info=True, shift=0):
    """one call in one form -> dict as mlm_cases.expected_mlm gives it ("selected" / "info" None when not given).  The `_dev`
    form: every output lies behind FRONT fence bytes and before BACK more; shift moves the ids pointer off 16-byte alignment by
    that many elements."""
    spec = native_spec(dev, s, ids.dtype == np.int64)
    if form == "host":
        assert not shift
        return dev.mlm_mask(ids, cls_tab, rand_ids, spec, selected=selected, info=info)
    import torch
    cells, size = ids.size, ids.dtype.itemsize
    d_in = torch.from_numpy(np.concatenate([np.zeros(shift, dtype=ids.dtype), ids.reshape(-1), np.zeros(4, dtype=ids.dtype)])).cuda()
    d_cls = torch.from_numpy(np.ascontiguousarray(cls_tab, dtype=np.uint8)).cuda()
    d_rand = torch.from_numpy(np.ascontiguousarray(rand_ids, dtype=np.uint32).view(np.int32)).cuda() if rand_ids is not None else None
    bodies = {"input_ids": cells * size, "labels": cells * size, "selected": cells, "info": 40}
    given = {"input_ids": True, "labels": True, "selected": selected, "info": info}
    bufs = {}
    for k, n in bodies.items():
        h = np.full(FRONT + n + BACK, GARBAGE, dtype=np.uint8)
        h[:FRONT] = FENCE
        h[FRONT + n:] = FENCE
        bufs[k] = torch.from_numpy(h).cuda()
    p = {k: (bufs[k].data_ptr() + FRONT if given[k] else None) for k in bodies}
    rc = dev.lib().swt_mlm_mask_dev(d_in.data_ptr() + shift * size, ids.shape[0], ids.shape[1], d_cls.data_ptr(),
                                    d_rand.data_ptr() if d_rand is not None else None, 0 if rand_ids is None else len(rand_ids), C.byref(spec),
                                    p["input_ids"], p["labels"], p["selected"], p["info"], None)
    dev.check(rc)
    torch.cuda.synchronize()
    out = {}
    for k, n in bodies.items():
        h = bufs[k].cpu().numpy()
        assert (h[:FRONT] == FENCE).all() and (h[FRONT + n:] == FENCE).all(), "%s: a byte outside rows * width was written" % k
        body = h[FRONT:FRONT + n].copy()
        if not given[k]:
            assert (body == GARBAGE).all(), "%s was not given and was written" % k
            out[k] = None
        else:
            out[k] = body.view({"selected": np.uint8, "info": np.uint64}.get(k, ids.dtype))
            if k != "info":
                out[k] = out[k].reshape(ids.shape)
    return out


def agree(got, want, what):
    for k in ("input_ids", "labels", "selected", "info"):
        if got[k] is None:
            continue
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        if not np.array_equal(got[k], want[k]):
            bad = np.argwhere(got[k] != want[k])
            raise AssertionError("%s: %s differs at %d places, first %s: got %s, want %s"
                                 % (what, k, len(bad), bad[0].tolist(), got[k][tuple(bad[0])], want[k][tuple(bad[0])]))


def check(dev, form, ids, s, what, tables=None, **kw):
    cls_tab, rand_ids = tables or M.toy_tables()
    want = M.expected_mlm(ids, cls_tab, rand_ids, s)
    got = run(dev, form, ids, cls_tab, rand_ids, s, **kw)
    agree(got, want, (what, form, str(ids.dtype)))
    return got, want


FORMS = ["host", "dev"]
DTYPES = [np.int32, np.int64]


@pytest.mark.parametrize("whole_word", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", FORMS)
def test_widths(dev, cols, form, dtype, whole_word):
    """the scalar and the wide path; one, two and three steps a row; 11 rows, so that groups of every size leave a wavefront
    partly dead"""
    for width in (1, 3, 4, 5, cols - 1, cols, cols + 1, 2 * cols + 1, 512, 513):
        ids = M.random_rows(11, width, seed=width, dtype=dtype)
        s = M.spec(M.N_CLASS, M.MASK_ID, 0.4, whole_word, seed=width * 7 + 1, epoch=3)
        got, want = check(dev, form, ids, s, ("width", width))
        assert width < 16 or 0 < want["n_selected"] < want["n_eligible"]


@pytest.mark.parametrize("form", FORMS)
def test_row_counts(dev, form):
    """the narrowest groups (widths 3 and 4: one lane a row, widths 5 and 8: two): 1 row, one wavefront's rows - 1, + 0 and + 1, a
    workgroup's rows + 1 with one set and with the four sets narrow groups walk"""
    per_wave = dev.mlm_capacity()[1]
    for width in (3, 4, 5, 8):
        for rows in (1, per_wave - 1, per_wave, per_wave + 1, 4 * per_wave + 1, 16 * per_wave + 1):
            ids = M.random_rows(rows, width, seed=rows + width, pad_tail=False)
            check(dev, form, ids, M.spec(M.N_CLASS, M.MASK_ID, 0.5, True, seed=rows), ("rows", rows, width))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", FORMS)
def test_words_across_the_seams(dev, cols, form, dtype):
    """a word of cols_per_step + 5 continuation tokens across every quad, lane and step seam, from four starting columns; a row
    that is one word; a row that starts with continuations; a class-2 id between two runs of continuations; padding only"""
    for width in (cols + 9, 2 * cols + 4, 2 * cols + 7):
        ids = M.long_word_rows(width, cols + 5, dtype)
        for seed in range(6):  # a word is selected with 1/2: some of the six draws select it, some do not
            got, want = check(dev, form, ids, M.spec(M.N_CLASS, M.MASK_ID, 0.5, True, seed=seed), ("long word", width, seed))
            for r in range(4):
                word = want["selected"][r, r:r + cols + 6]
                assert word.all() or not word.any()
    width = 2 * cols + 3
    ids = np.full((7, width), M.CONT + 3, dtype=dtype)  # row 1: continuations from column 0 on, one group
    ids[0, 0] = M.WORD                      # one word from end to end
    ids[2, cols + 1] = M.UNK                # [UNK] between two runs of continuations: the second run is a group of its own
    ids[3, :] = M.PAD                       # padding only
    ids[4, cols] = M.SEP                    # a run that ends on the last column of a step
    ids[5, 4 * 17] = M.WORD                 # a head on a quad's first column
    ids[6, cols - 1] = M.SEP                # a run that starts on the first column of a step: its left neighbour is the carry
    seen = set()
    for seed in range(8):
        got, want = check(dev, form, ids, M.spec(M.N_CLASS, M.MASK_ID, 0.5, True, seed=seed), ("runs", seed))
        sel = want["selected"]
        assert sel[0].all() or not sel[0].any()
        assert sel[1].all() or not sel[1].any()
        for part in (sel[2, :cols + 1], sel[2, cols + 2:]):
            assert part.all() or not part.any()
        assert not sel[3].any() and not sel[2, cols + 1]
        for r, cut in ((4, cols), (6, cols - 1)):
            assert all(part.all() or not part.any() for part in (sel[r, :cut], sel[r, cut + 1:])) and not sel[r, cut]
        seen.add((bool(sel[2, 0]), bool(sel[2, -1])))
    assert len(seen) > 1  # the two runs of row 2 are drawn apart
    # without whole words every column draws for itself
    check(dev, form, ids, M.spec(M.N_CLASS, M.MASK_ID, 0.5, False, seed=1), "runs, per token")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", FORMS)
def test_thresholds_and_ids_outside_the_table(dev, cols, form, dtype):
    cls_tab, rand_ids = M.toy_tables()
    ids = M.random_rows(9, cols + 6, seed=4, dtype=dtype)
    ids[1, 5], ids[1, 6], ids[2, 0] = M.N_CLASS, 2 ** 31 - 1, M.N_CLASS + 1000  # >= n_class: class 2, and a neighbour's left
    if dtype == np.int64:
        ids[3, 2], ids[3, 3], ids[4, 7], ids[5, 1] = -1, -(2 ** 40), 2 ** 40 + 7, 2 ** 32 + 6  # the low word alone would be an id
    else:
        ids[3, 2], ids[3, 3] = -1, -(2 ** 31)
    for name, kw in (("p 0", {"probability": 0.0}), ("p 1", {"probability": 1.0}), ("mask 1", {"probability": 0.5, "mask_share": 1.0, "random_share": 0.0}),
                     ("default", {}), ("keep all", {"probability": 0.5, "mask_share": 0.0, "random_share": 0.0})):
        got, want = check(dev, form, ids, M.spec(M.N_CLASS, M.MASK_ID, seed=11, **kw), name)
        if name == "p 0":
            assert want["n_selected"] == 0 and np.array_equal(got["input_ids"], ids)
        if name == "p 1":
            assert want["n_selected"] == want["n_eligible"] > 0
        if name == "mask 1":
            assert want["n_masked"] == want["n_selected"] > 0
    # every selected column becomes one of two ids
    two = np.array([7, 33], dtype=np.uint32)
    s = M.spec(M.N_CLASS, M.MASK_ID, 0.6, True, seed=5, mask_share=0.0, random_share=1.0)
    got, want = check(dev, form, ids, s, "random 1", tables=(cls_tab, two))
    assert want["n_random"] == want["n_selected"] > 0 and set(got["input_ids"][got["selected"] == 1].tolist()) == {7, 33}
    # no random share: rand_ids may be NULL
    s = M.spec(M.N_CLASS, M.MASK_ID, 0.6, True, seed=5, mask_share=0.7, random_share=0.0)
    check(dev, form, ids, s, "no rand_ids", tables=(cls_tab, None))
    # out_selected and info NULL
    for selected, info in ((False, True), (True, False), (False, False)):
        check(dev, form, ids, M.spec(M.N_CLASS, M.MASK_ID, 0.3, seed=8), ("optional", selected, info), selected=selected, info=info)


@pytest.mark.parametrize("dtype", DTYPES)
def test_unaligned_ids_take_the_scalar_path(dev, cols, dtype):
    """an ids pointer one element off: the width is a multiple of four and the wide path still must not be taken"""
    for width in (8, cols + 4):
        ids = M.random_rows(5, width, seed=width, dtype=dtype)
        check(dev, "dev", ids, M.spec(M.N_CLASS, M.MASK_ID, 0.4, seed=2), ("shifted", width), shift=1)


@pytest.mark.parametrize("form", FORMS)
def test_epochs_and_repeats(dev, cols, form):
    ids = M.random_rows(13, cols + 8, seed=21)
    a, _ = check(dev, form, ids, M.spec(M.N_CLASS, M.MASK_ID, 0.3, seed=99, epoch=0), "epoch 0")
    b, _ = check(dev, form, ids, M.spec(M.N_CLASS, M.MASK_ID, 0.3, seed=99, epoch=1), "epoch 1")
    again, _ = check(dev, form, ids, M.spec(M.N_CLASS, M.MASK_ID, 0.3, seed=99, epoch=0), "epoch 0 again")
    assert not np.array_equal(a["selected"], b["selected"])
    for k in ("input_ids", "labels", "selected", "info"):
        assert np.array_equal(a[k], again[k])
    # a row's masks do not depend on the rows around it, nor on the integer width
    part, _ = check(dev, form, np.ascontiguousarray(ids[:3]), M.spec(M.N_CLASS, M.MASK_ID, 0.3, seed=99, epoch=0), "three rows")
    assert np.array_equal(part["input_ids"], a["input_ids"][:3])
    wide, _ = check(dev, form, ids.astype(np.int64), M.spec(M.N_CLASS, M.MASK_ID, 0.3, seed=99, epoch=0), "int64")
    assert np.array_equal(wide["input_ids"], a["input_ids"]) and np.array_equal(wide["labels"], a["labels"])
    big, _ = check(dev, form, ids, M.spec(M.N_CLASS, M.MASK_ID, 0.3, seed=(1 << 64) - 3, epoch=(1 << 32) - 1), "the largest seed and epoch")
    assert not np.array_equal(big["selected"], a["selected"])


def test_dev_form_refuses_and_takes_no_row(dev):
    import torch
    d = torch.zeros(64, dtype=torch.int32, device="cuda")
    p = d.data_ptr()
    spec = dev.mlm_spec(40, 4, 1 << 30, 1 << 31, 1 << 31)
    lib = dev.lib()
    assert lib.swt_mlm_mask_dev(p, 2, 4, p + 128, None, 0, C.byref(spec), p, p + 64, None, None, None) == dev.ERR_INVALID
    assert "out_ids" in lib.swt_last_error().decode()
    assert lib.swt_mlm_mask_dev(p, 2, 4, p + 128, None, 0, C.byref(spec), p + 64, p + 96, None, None, None) == 0
    assert lib.swt_mlm_mask_dev(p + 2, 2, 4, p + 128, None, 0, C.byref(spec), p + 64, p + 96, None, None, None) == dev.ERR_INVALID  # alignment
    info = torch.full((5,), 7, dtype=torch.int64, device="cuda")
    assert lib.swt_mlm_mask_dev(p, 0, 4, p + 128, None, 0, C.byref(spec), p + 64, p + 96, None, info.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert info.tolist() == [0] * 5


# ---- through the classes

def _tokenizer(swt, ref_dir, cls):
    tok = getattr(swt, cls)()
    tok.load_resources(os.path.join(ref_dir, "resources/pretrained", "FastBPE" if "BPE" in cls else "FastWordPiece"))
    return tok


def _np(res):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in res.items()}


@pytest.mark.parametrize("cls", ["FastBPE", "FastWP", "NaiveBPE", "NaiveWP"])
def test_encode_batch_mlm(swt, dev, ref_dir, corpora, cls):
    """encode_batch(mlm=...) on 200 sentences of train-5K -- padded rows of 32, pairs, rows packed whole at 128 -- against the
    model applied to the same call's ids without mlm; NumPy and torch results are equal"""
    tok = _tokenizer(swt, ref_dir, cls)
    texts = list(corpora["t5k"])[:200]
    voc = tok._batch_vocabulary()
    mlm = {"probability": 0.2, "seed": 31, "epoch": 2, "return_selected": True}
    forms = ({"max_length": 32, "padding": "max_length"}, {"text_pairs": texts[100:] + texts[:100], "max_length": 48},
             {"max_length": 128, "packing": "whole"}, {"max_length": 32, "padding": "max_length", "int64": True})
    for kw in forms:
        results = []
        for device in (False, True):
            base = _np(tok.encode_batch(texts, device=device, **kw))
            got = tok.encode_batch(texts, device=device, mlm=mlm, **kw)
            assert ("torch" in str(type(got["input_ids"]))) == device and got["labels"].dtype == got["input_ids"].dtype
            got = _np(got)
            ids = base["input_ids"]
            s = M.spec(voc.cls_tab.size, tok.mask_id(), 0.2, True, seed=31, epoch=2)
            want = M.expected_mlm(ids, voc.cls_tab, voc.rand_ids, s)
            assert np.array_equal(got["input_ids"], want["input_ids"]) and np.array_equal(got["labels"], want["labels"])
            assert np.array_equal(got["selected"], want["selected"])
            on = got["labels"] != -100
            assert on.any() and np.array_equal(got["labels"][on], ids[on])
            for name in M.COUNTS:
                assert got[name] == want[name], name
            assert 0 < got["n_masked"] and got["n_eligible"] < ids.size
            sp = tok.special_ids()
            assert not on[np.isin(ids, list(sp.values()))].any()
            for k in base:  # everything else is the call's without mlm
                if k != "input_ids":
                    assert np.array_equal(got[k], base[k]), k
            results.append(got)
        for k in results[0]:
            assert np.array_equal(results[0][k], results[1][k]), k
    # mask_tokens on finished rows: the defaults, and {} through encode_batch
    base = tok.encode_batch(texts[:50], max_length=32)
    a = tok.encode_batch(texts[:50], max_length=32, mlm={})
    b = tok.mask_tokens(base["input_ids"])
    assert np.array_equal(a["input_ids"], b["input_ids"]) and np.array_equal(a["labels"], b["labels"]) and "selected" not in b
    assert (b["input_ids"] == tok.mask_id()).any()
    import torch
    with pytest.raises(TypeError):
        tok.mask_tokens(torch.zeros((2, 3), dtype=torch.int32))  # a tensor that is not on the GPU
    with pytest.raises(TypeError):
        tok.mask_tokens(torch.zeros((2, 3), dtype=torch.float32, device="cuda"))
    with pytest.raises(TypeError):
        tok.mask_tokens(torch.zeros((3, 4), dtype=torch.int64, device="cuda").t())
