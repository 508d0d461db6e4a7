"""swt_denoise_plan / swt_denoise_rows and their `_dev` forms on the GPU against the plain-Python model (tests/denoise_cases.py):
every output array and `info`, exactly, at the shapes where the kernel can go wrong (denoise_cases.cases).  Every `_dev` call
runs with fences before and after each output."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from tests import denoise_cases as D

pytestmark = pytest.mark.gpu

FENCE, GARBAGE, BAND = 0xEE, 0x5A, 64
OUTPUTS = ("input_ids", "attention_mask", "length", "labels", "label_length", "info")


@pytest.fixture(scope="module")
def dev(native):
    if native.device_count() < 1:
        pytest.fail("no HIP device")
    native.init(0)
    return native


@functools.lru_cache(maxsize=None)
def wanted(dtype, mode, whole_word):
    """the model of every case, computed once; its label width is the one the calls are given"""
    out = []
    for name, ids, kw in D.cases(dtype):
        s = D.spec(mode, whole_word=whole_word, seed=len(name), epoch=5, **kw)
        want = D.expected(ids, D.CLS_TAB, s)
        out.append((name, ids, dict(s, label_width=want["labels"].shape[1] if mode == D.SENTINEL else 0), want))
    return out


def run(dev, form, ids, s, want):
    """the plan, then the rows, in one form -> (plan's info, dict as denoise_cases.expected gives it)"""
    spec = dev.denoise_spec(s["mode"], s["n_class"], s["mask_id"], s["pad_id"], s["start_below"], s["len_below"], s["n_sentinel"],
                            s["label_width"], s["seed"], s["epoch"], s["whole_word"], ids.dtype == np.int64)
    if form == "host":
        return dev.denoise_plan(ids, D.CLS_TAB, spec), dev.denoise_rows(ids, D.CLS_TAB, D.SENTINELS, spec)
    import torch
    d_in, d_cls = torch.from_numpy(ids).cuda(), torch.from_numpy(D.CLS_TAB).cuda()
    d_sent, d_plan = torch.from_numpy(D.SENTINELS.view(np.int32)).cuda(), torch.zeros(7, dtype=torch.int64, device="cuda")
    bufs = {}
    for k in OUTPUTS:
        if want[k] is not None:
            h = np.full(want[k].nbytes + 2 * BAND, FENCE, dtype=np.uint8)
            h[BAND:BAND + want[k].nbytes] = GARBAGE
            bufs[k] = torch.from_numpy(h).cuda()
    p = {k: bufs[k].data_ptr() + BAND if k in bufs else None for k in OUTPUTS}
    lib = dev.lib()
    dev.check(lib.swt_denoise_plan_dev(d_in.data_ptr(), ids.shape[0], ids.shape[1], d_cls.data_ptr(), C.byref(spec), d_plan.data_ptr(), None))
    dev.check(lib.swt_denoise_rows_dev(d_in.data_ptr(), ids.shape[0], ids.shape[1], d_cls.data_ptr(), d_sent.data_ptr(), C.byref(spec),
                                       p["input_ids"], p["attention_mask"], p["length"], p["labels"], p["label_length"], p["info"], None))
    torch.cuda.synchronize()
    out = dict.fromkeys(OUTPUTS)
    for k, b in bufs.items():
        h = b.cpu().numpy()
        assert (h[:BAND] == FENCE).all() and (h[-BAND:] == FENCE).all(), "%s: a byte outside the output was written" % k
        out[k] = h[BAND:-BAND].copy().view(want[k].dtype).reshape(want[k].shape)
    return d_plan.cpu().numpy().astype(np.uint64), out


def agree(got, want, what):
    for k in OUTPUTS:
        assert (got[k] is None) == (want[k] is None), (what, k)
        if want[k] is not None:
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
            bad = np.argwhere(got[k] != want[k])
            assert not len(bad), "%s: %s differs at %d places, first %s" % (what, k, len(bad), bad[0].tolist())


@pytest.mark.parametrize("whole_word", [True, False])
@pytest.mark.parametrize("dtype", [np.int32, np.int64])
@pytest.mark.parametrize("form", ["host", "dev"])
@pytest.mark.parametrize("mode", [D.MASK, D.SENTINEL, D.INFILL])
def test_cases_equal_the_model(dev, mode, form, dtype, whole_word):
    seen = np.zeros(7, dtype=np.uint64)
    for name, ids, s, want in wanted(dtype, mode, whole_word):
        plan, got = run(dev, form, ids, s, want)
        agree(got, want, (name, form))
        assert np.array_equal(plan, want["info"]), (name, plan, want["info"])
        seen = np.maximum(seen, want["info"])
        if name.startswith("seams 1"):  # the first row alone is the first row of the batch
            alone = run(dev, form, np.ascontiguousarray(ids[:1]), s, {k: None if v is None or k == "info" else v[:1] for k, v in want.items()})[1]
            for k in OUTPUTS[:-1]:
                assert want[k] is None or np.array_equal(alone[k], want[k][:1]), (name, k)
    # the cases reach what they are there for: noise, runs, and in SENTINEL mode runs given back and rows cut
    assert seen[1] > 0 and seen[2] > 1 and (mode != D.SENTINEL or (seen[3] > 0 and seen[4] > 0)) and seen[5] == 516


def test_corrupt_spans_through_a_class(swt, dev, ref_dir, corpora):
    """corrupt_spans over padded rows of 200 sentences, NumPy and torch, against the model over the vocabulary's own tables"""
    tok = swt.FastWP()
    tok.load_resources(os.path.join(ref_dir, "resources/pretrained", "FastWordPiece"))
    names = ["<extra_id_%d>" % k for k in range(8)]
    tok.add_special_tokens(names)
    voc = tok._batch_vocabulary()
    sent = np.array([voc.index[n] for n in names], dtype=np.uint32)
    from subword_tokenizers_amd import batching as B
    for mode, m in (("mask", D.MASK), ("sentinel", D.SENTINEL), ("infill", D.INFILL)):
        for device in (False, True):
            ids = tok.encode_batch(list(corpora["t5k"])[:200], max_length=48, padding="max_length", device=device)["input_ids"]
            got = tok.corrupt_spans(ids, mode, noise_density=0.3, seed=7, epoch=1, target_length=20 if device else None)
            got = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in got.items()}
            _, start, below = B._denoise_thresholds(mode, 0.3)
            s = dict(D.spec(m, start, below, seed=7, epoch=1, n_sentinel=8, label_width=20 if device else None), n_class=voc.cls_tab.size,
                     mask_id=tok.mask_id(), pad_id=voc.special["pad"])
            host = ids.cpu().numpy() if device else ids
            want = D.expected(host, voc.cls_tab, s, sent)
            want["labels"] = host if m == D.INFILL else want["labels"]
            for k in OUTPUTS[:-1]:
                assert (want[k] is None and k not in got) or np.array_equal(got[k], want[k]), (mode, device, k)
            assert [got[k] for k in D.COUNTS] == want["info"].tolist() and 0 < got["n_noise"] < got["n_eligible"]
