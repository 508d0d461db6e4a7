"""The NumPy model of masked-LM batches (tests/mlm_cases.py) held, without a GPU, to the known answers of Philox4x32-10, to a
plain per-column loop, to the properties that make a masking one and to its nominal shares; what the host form refuses before it
looks for a device; and the class tables of the shipped vocabularies."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from tests import mlm_cases as M

KNOWN = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


def test_philox_known_answers():
    for counter, key, want in KNOWN:
        assert tuple(M.philox_scalar(counter, key)) == want
        assert tuple(int(x) for x in M.philox(*counter, *key)) == want
    c = np.array([k[0] for k in KNOWN], dtype=np.uint64).T  # the vector form, one key at a time
    for i, (_, key, want) in enumerate(KNOWN):
        got = M.philox(c[0], c[1], c[2], c[3], *key)
        assert tuple(int(x[i]) for x in got) == want


@pytest.mark.parametrize("whole_word", [True, False])
@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_model_equals_the_loop(whole_word, dtype):
    cls_tab, rand_ids = M.toy_tables()
    ids = M.random_rows(7, 37, seed=5, dtype=dtype)
    ids[2, 3], ids[4, 0] = 1000, -7  # outside the table
    ids[5, :4] = M.CONT  # a row that starts with continuations
    for probability, seed, epoch in ((0.15, 0, 0), (0.5, (1 << 63) + 12345, 7), (1.0, 3, 0xFFFFFFFF), (0.0, 3, 1)):
        s = M.spec(M.N_CLASS, M.MASK_ID, probability, whole_word, seed, epoch)
        got, want = M.expected_mlm(ids, cls_tab, rand_ids, s), M.expected_mlm_loop(ids, cls_tab, rand_ids, s)
        for k in ("input_ids", "labels", "selected", "info"):
            assert np.array_equal(got[k], want[k]), (k, probability)
            assert got[k].dtype == want[k].dtype


def test_structural_properties():
    cls_tab, rand_ids = M.toy_tables()
    ids = M.random_rows(64, 96, seed=9)
    ids[0, :3] = (M.CONT, M.CONT + 1, M.WORD)  # a cut word at column 0 is its own group
    cls = M.classes(ids, cls_tab, M.N_CLASS)
    for whole_word in (True, False):
        got = M.expected_mlm(ids, cls_tab, rand_ids, M.spec(M.N_CLASS, M.MASK_ID, 0.3, whole_word, seed=77))
        sel = got["selected"] == 1
        assert 0 < sel.sum() < (cls < 2).sum()
        assert (got["labels"][sel] == ids[sel]).all() and (got["labels"][~sel] == M.IGNORE).all()
        assert (got["input_ids"][~sel] == ids[~sel]).all()
        assert not sel[cls == 2].any()
        changed = got["input_ids"] != ids
        assert ((got["input_ids"][changed] == M.MASK_ID) | (M.classes(got["input_ids"], cls_tab, M.N_CLASS)[changed] < 2)).all()
        assert got["n_selected"] == got["n_masked"] + got["n_random"] + got["n_kept"] == int(sel.sum())
        assert got["n_eligible"] == int((cls < 2).sum())
        # a word -- a maximal run of eligible columns cut before every class-0 column -- is selected whole or not at all
        words = 0
        for r in range(ids.shape[0]):
            c = 0
            while c < ids.shape[1]:
                if cls[r, c] == 2:
                    c += 1
                    continue
                e = c + 1
                while whole_word and e < ids.shape[1] and cls[r, e] == 1:
                    e += 1
                assert sel[r, c:e].all() or not sel[r, c:e].any(), (r, c, e)
                words += 1
                c = e
        assert words > 64
    h = M.heads(cls, True)
    assert h[0, 0] == 0 and h[0, 1] == 0 and h[0, 2] == 2


def test_measured_shares():
    """seed 2024, epoch 0, 2048 x 512 single-token words, probability 0.15, shares 0.8 / 0.1: each share within 4 binomial
    standard deviations sqrt(q (1 - q) / n) of its nominal value"""
    cls_tab = np.zeros(1100, dtype=np.uint8)
    cls_tab[:5] = 2
    rand_ids = np.arange(5, 1005, dtype=np.uint32)
    ids = np.full((2048, 512), 1050, dtype=np.int32)
    got = M.expected_mlm(ids, cls_tab, rand_ids, M.spec(1100, 4, 0.15, True, seed=2024, epoch=0))
    n = ids.size
    assert got["n_eligible"] == n

    def within(share, q, count):
        sigma = math.sqrt(q * (1 - q) / count)
        print("share %.5f nominal %.2f: %.2f sigma" % (share, q, (share - q) / sigma))
        return abs(share - q) <= 4 * sigma

    k = got["n_selected"]
    assert within(k / n, 0.15, n)
    assert within(got["n_masked"] / k, 0.8, k)
    assert within(got["n_random"] / k, 0.1, k)
    drawn = got["input_ids"][(got["selected"] == 1) & (got["input_ids"] != 4) & (got["input_ids"] != 1050)]
    assert drawn.size == got["n_random"]
    assert np.bincount(drawn - 5, minlength=1000).min() > 0  # 1,000 values, no empty bucket
    assert drawn.min() >= 5 and drawn.max() < 1005


# ---- the built library, without a device

def _call(native, ids=True, out_ids=True, out_labels=True, cls_tab=True, rand_ids=True, n_rand=None, spec=True, rows=None, width=None,
          selected=None, info=None, **fields):
    a = np.arange(5, 17, dtype=np.int32).reshape(3, 4)
    bufs = {"ids": a, "out_ids": np.zeros_like(a), "out_labels": np.zeros_like(a), "cls_tab": np.zeros(40, dtype=np.uint8),
            "rand_ids": np.arange(5, 40, dtype=np.uint32)}
    given = {"ids": ids, "out_ids": out_ids, "out_labels": out_labels, "cls_tab": cls_tab, "rand_ids": rand_ids}
    p = {}
    for k, v in given.items():
        p[k] = bufs[k].ctypes.data if v is True else None if v in (False, None) else v
    s = native.mlm_spec(40, 4, 1 << 30, 1 << 31, 3 << 30)
    for k, v in fields.items():
        setattr(s, k, v)
    lib = native.lib()
    at = lambda x, typ: C.cast(C.c_void_p(x), typ)
    rc = lib.swt_mlm_mask(p["ids"], 3 if rows is None else rows, 4 if width is None else width, at(p["cls_tab"], native.u8p),
                          at(p["rand_ids"], native.u32p), 35 if n_rand is None else n_rand, C.byref(s) if spec else None, p["out_ids"],
                          p["out_labels"], at(selected, native.u8p), at(info, native.u64p))
    return rc, lib.swt_last_error().decode(), bufs


def test_host_form_refuses_bad_arguments_without_a_device(native):
    INV = native.ERR_INVALID
    for name in ("ids", "out_ids", "out_labels", "cls_tab", "spec"):
        rc, msg, _ = _call(native, **{name: False})
        assert rc == INV and name in msg, name
    bad = [({"width": 0}, "width"), ({"rows": 1 << 32}, "rows"), ({"flags": 2}, "flag"), ({"flags": 8}, "flag"),
           ({"select_below": (1 << 32) + 1}, "select_below"), ({"mask_below": (1 << 32) + 1, "random_below": (1 << 32) + 1}, "mask_below"),
           ({"random_below": (1 << 32) + 1}, "random_below"), ({"mask_below": 3 << 30, "random_below": 1 << 31}, "mask_below"),
           ({"n_class": 0}, "n_class"), ({"rand_ids": False}, "rand_ids"), ({"n_rand": 0}, "n_rand")]
    for kw, word in bad:
        rc, msg, _ = _call(native, **kw)
        assert rc == INV and word in msg, (kw, msg)
    # an output that overlaps the input: the same array, and one shifted by a row
    _, _, bufs = _call(native, spec=False)
    at = bufs["ids"].ctypes.data
    for name in ("out_ids", "out_labels"):
        for shift in (0, 16, -16, 47):
            rc, msg, _ = _call(native, ids=at, **{name: at + shift})
            assert rc == INV and name in msg, (name, shift)
    rc, msg, _ = _call(native, ids=at, selected=at + 40)
    assert rc == INV and "out_selected" in msg
    # nothing to draw a random id from is no obstacle where none is drawn
    rc, _, _ = _call(native, rows=0, rand_ids=False, mask_below=5, random_below=5)
    assert rc == 0
    # no row: success without a device, info zeroed
    info = np.full(5, 9, dtype=np.uint64)
    rc, _, _ = _call(native, rows=0, info=info.ctypes.data)
    assert rc == 0 and info.tolist() == [0] * 5
    rc, _, _ = _call(native, rows=0, width=0)
    assert rc == 0
    if native.device_count() == 0:  # everything in order: only now is a device looked for
        rc, _, _ = _call(native)
        assert rc == native.ERR_NO_DEVICE


def test_symbols_and_constants(native):
    lib = C.CDLL(native._build.LIB_PATH)
    for name in ("swt_mlm_mask", "swt_mlm_mask_dev", "swt_mlm_capacity"):
        assert hasattr(lib, name) and name in native.SIGNATURES
    cols, per_wave = native.mlm_capacity()
    assert cols >= 64 and cols % 4 == 0 and 1 <= per_wave <= 64
    assert (native.MLM_WHOLE_WORD, native.MLM_IDS64) == (1, native.BATCH_IDS64)
    assert C.sizeof(native.MlmSpec) == 48


def test_mask_tokens_refuses_bad_arguments(swt):
    """decided from the arguments alone, before a vocabulary or a device is looked for"""
    tok = swt.FastWP()
    ids = np.zeros((2, 3), dtype=np.int32)
    for bad in ({"probability": -0.1}, {"probability": 1.5}, {"mask_share": 1.1}, {"random_share": -1}, {"mask_share": 0.8, "random_share": 0.3},
                {"seed": -1}, {"seed": 1 << 64}, {"epoch": -1}, {"epoch": 1 << 32}):
        with pytest.raises(ValueError):
            tok.mask_tokens(ids, **bad)
        with pytest.raises(ValueError):
            tok.encode_batch(["a"], mlm=bad)
    with pytest.raises(TypeError):
        tok.encode_batch(["a"], mlm={"chance": 0.5})
    with pytest.raises(TypeError):
        tok.encode_batch(["a"], mlm=0.15)


@pytest.mark.parametrize("cls", ["FastBPE", "NaiveBPE", "FastWP", "NaiveWP"])
def test_vocabulary_tables(swt, ref_dir, cls):
    tok = getattr(swt, cls)()
    tok.load_resources(os.path.join(ref_dir, "resources/pretrained", "FastBPE" if "BPE" in cls else "FastWordPiece"))
    tokens, voc = tok.vocab_list(), tok._batch_vocabulary()
    assert voc.cls_tab.dtype == np.uint8 and voc.cls_tab.size == len(tokens)
    never = {"[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"}
    for i, t in enumerate(tokens):
        assert voc.cls_tab[i] == (2 if t in never else 1 if t.startswith("##") and len(t) > 2 else 0), (i, t)
    assert voc.rand_ids.dtype == np.uint32 and (np.diff(voc.rand_ids.astype(np.int64)) > 0).all()
    assert voc.rand_ids.tolist() == [i for i, t in enumerate(tokens) if t not in never]
    assert not set(voc.rand_ids.tolist()) & set(tok.special_ids().values())
    assert voc.cls_tab is voc.cls_tab and voc.rand_ids is voc.rand_ids  # built once
    assert tok.mask_id() == (tokens.index("[MASK]") if "[MASK]" in tokens else len(tokens))
    if "BPE" in cls:
        assert tok.mask_id() == len(tokens)
    assert tok.mask_id() not in voc.rand_ids.tolist()
    for bad in (np.zeros((2, 3), dtype=np.int16), np.zeros(6, dtype=np.int32), np.zeros((3, 4), dtype=np.int32).T, [[1, 2]],
                np.zeros((2, 3), dtype=np.uint32), np.zeros((2, 2, 2), dtype=np.int64)):
        with pytest.raises(TypeError):
            tok.mask_tokens(bad)
