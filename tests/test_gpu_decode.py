"""swt_decode_plan / swt_decode_rows and their `_dev` forms on the GPU against the Python model (tests/decode_cases.py), byte for
byte, with text_off, status and info, at the smallest shapes that reach each seam of the kernel: the scalar and the wide path,
one, two and three steps a row, rows that share a wavefront and a last wavefront that is partly dead, a token of each kind and a
stretch of skipped columns across every quad, lane and step seam, the seam of the plan's scan group.  Every `_dev` call runs with
fences before and after each output.  Then the tokenizer classes end to end against the reference's recorded strings
(tests/golden/recover_sentence.json)."""
import os

import numpy as np
import pytest

from tests import decode_cases as D

pytestmark = pytest.mark.gpu

FENCE, GARBAGE, FRONT, BACK = 0xEE, 0x5A, 64, 64
FORMS = ["host", "dev"]
DTYPES = [np.int32, np.int64]


@pytest.fixture(scope="module")
def dev(native):
    if native.device_count() < 1:
        pytest.fail("no HIP device")
    native.init(0)
    return native


@pytest.fixture(scope="module")
def cols(dev):
    return dev.decode_capacity()[0]


@pytest.fixture(scope="module")
def tabs():
    return D.tables(D.TOY, len(D.TOY))


def fenced(n):
    import torch
    h = np.full(FRONT + n + BACK, GARBAGE, dtype=np.uint8)
    h[:FRONT] = FENCE
    h[FRONT + n:] = FENCE
    return torch.from_numpy(h).cuda()


def unfenced(buf, n, what):
    h = buf.cpu().numpy()
    assert (h[:FRONT] == FENCE).all() and (h[FRONT + n:] == FENCE).all(), "%s: a byte outside the output was written" % what
    return h[FRONT:FRONT + n].copy()


def run(dev, form, ids, mask, tabs, skip=True, shift=0, text_cap=None):
    """plan and rows in one form -> (text, text_off, status, info).  The `_dev` form: every output lies behind FRONT fence bytes and
    before BACK more; shift moves the ids pointer off 16-byte alignment by that many elements; text_cap, below the plan's total,
    leaves the bytes from there on as they were."""
    tok_bytes, tok_off, tok_flags, n_tok = tabs
    if form == "host":
        assert not shift
        text_off, status, info = dev.decode_plan(ids, mask, tok_off, tok_flags, n_tok, skip)
        return dev.decode_rows(ids, mask, tok_bytes, tok_off, tok_flags, n_tok, text_off, skip, text_cap), text_off, status, info
    import torch
    rows, width = ids.shape
    size = ids.dtype.itemsize
    flags = (dev.DECODE_SKIP_SPECIAL if skip else 0) | (dev.DECODE_IDS64 if ids.dtype == np.int64 else 0)
    d_in = torch.from_numpy(np.concatenate([np.zeros(shift, dtype=ids.dtype), ids.reshape(-1), np.zeros(4, dtype=ids.dtype)])).cuda()
    d_mask = torch.from_numpy(np.concatenate([mask.reshape(-1), np.zeros(4, dtype=np.uint8)])).cuda() if mask is not None else None
    d_bytes = torch.from_numpy(np.concatenate([tok_bytes, np.zeros(4, dtype=np.uint8)])).cuda()
    d_off, d_flags = torch.from_numpy(tok_off.view(np.int32)).cuda(), torch.from_numpy(tok_flags).cuda()
    b_off, b_status, b_info = fenced(8 * (rows + 1)), fenced(rows), fenced(24)
    head = (d_in.data_ptr() + shift * size, d_mask.data_ptr() if d_mask is not None else None, rows, width)
    dev.check(dev.lib().swt_decode_plan_dev(*head, d_off.data_ptr(), d_flags.data_ptr(), n_tok, flags, b_off.data_ptr() + FRONT,
                                            b_status.data_ptr() + FRONT, b_info.data_ptr() + FRONT, None))
    torch.cuda.synchronize()
    text_off = unfenced(b_off, 8 * (rows + 1), "text_off").view(np.uint64)
    status, info = unfenced(b_status, rows, "status"), unfenced(b_info, 24, "info").view(np.uint64)
    total = int(info[0])
    cap = total if text_cap is None else text_cap
    b_text = fenced(total)
    dev.check(dev.lib().swt_decode_rows_dev(*head, d_bytes.data_ptr(), d_off.data_ptr(), d_flags.data_ptr(), n_tok, flags, b_off.data_ptr() + FRONT,
                                            b_text.data_ptr() + FRONT, cap, None))
    torch.cuda.synchronize()
    text = unfenced(b_text, total, "text")
    assert (text[cap:] == GARBAGE).all(), "a byte at or beyond text_cap was written"
    assert np.array_equal(unfenced(b_off, 8 * (rows + 1), "text_off").view(np.uint64), text_off), "the rows call wrote text_off"
    return text[:cap], text_off, status, info


def check(dev, form, ids, mask, tabs, what, skip=True, **kw):
    want = D.decode(ids, mask, tabs, D.SKIP_SPECIAL if skip else 0)
    got = run(dev, form, ids, mask, tabs, skip, **kw)
    for k, name in enumerate(("text", "text_off", "status", "info")):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, form, name, got[k].shape, want[k].shape)
        if not np.array_equal(got[k], want[k]):
            bad = np.flatnonzero(got[k] != want[k])
            at = int(bad[0])
            row = int(np.searchsorted(want[1], at, side="right")) - 1 if name == "text" else at
            raise AssertionError("%s %s %s: %s differs at %d places, first %d (row %d): got %r, want %r"
                                 % (what, form, ids.dtype, name, bad.size, at, row, got[k][at:at + 8].tolist(), want[k][at:at + 8].tolist()))
    return want


@pytest.mark.parametrize("skip", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", FORMS)
def test_widths(dev, cols, tabs, form, dtype, skip):
    """the scalar and the wide path; one, two and three steps a row; 11 rows, so that groups of every size share a wavefront and
    leave it partly dead; mask_id one past the end of the token list, skipped or spelled"""
    for width in (1, 3, 4, 5, cols - 1, cols, cols + 1, 2 * cols + 1):
        ids, mask = D.random_rows(11, width, seed=width, dtype=dtype)
        want = check(dev, form, ids, mask, tabs, ("width", width), skip)
        assert width < 16 or want[3][0] > width
        check(dev, form, ids, None, tabs, ("width without a mask", width), skip)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", FORMS)
def test_seams(dev, cols, tabs, form, dtype):
    """a glued token, a P token, a Q token, the three-byte quote, a glued Q token and a token of 84 bytes on either side of every
    quad, lane and step boundary; mask zeros, specials and left padding between two kept tokens across each boundary and before
    a first kept glued token; rows with nothing kept, the last row empty"""
    for width in (13, cols + 9, 2 * cols + 1):
        ids, mask = D.seam_rows(width, cols)
        want = check(dev, form, ids.astype(dtype), mask, tabs, ("seams", width))
        assert want[1][-1] == want[1][-2] == want[1][-3]  # the last two rows hold nothing
        assert not want[2].any()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", FORMS)
def test_reported_rows(dev, cols, tabs, form, dtype):
    """ids at -1, -100, n_tok and (64-bit) 2^31 and 2^32 + 4 on kept columns set bit 0, on columns not kept nothing; the BAD token
    sets bit 1; such columns write nothing and are no neighbours of those that do"""
    ix, mask_id = D.toy_ids()
    n_tok = tabs[3]
    outside = [-1, -100, n_tok, n_tok + 7] + ([1 << 31, (1 << 32) + 4] if dtype == np.int64 else [(1 << 31) - 1])
    width = cols + 7
    ids = np.full((2 * len(outside) + 4, width), ix["ab"], dtype=dtype)
    mask = np.ones(ids.shape, dtype=np.uint8)
    for k, bad in enumerate(outside):
        ids[2 * k, [0, 3, 4, cols - 1, cols, width - 1]] = bad  # kept
        ids[2 * k, 5] = ix["##cd"]  # its neighbour to the left is the "ab" of column 2
        ids[2 * k + 1, [1, 4, cols, width - 1]] = bad  # not kept
        mask[2 * k + 1, [1, 4, cols, width - 1]] = 0
    base = 2 * len(outside)
    ids[base, [3, 4]] = D.TOY_BAD
    ids[base, 5] = ix["##cd"]
    ids[base + 1, 2], mask[base + 1, 2] = D.TOY_BAD, 0
    ids[base + 2, [0, 7]] = [D.TOY_BAD, -1]
    ids[base + 3, :] = mask_id + 1 if dtype == np.int32 else 1 << 40
    want = check(dev, form, ids, mask, tabs, "reported")
    assert want[2].tolist() == [1, 0] * len(outside) + [2, 0, 3, 1] and want[3][1] == len(outside) + 3
    check(dev, form, ids, mask, tabs, "reported, specials spelled", skip=False)


@pytest.mark.parametrize("dtype", DTYPES)
def test_ids_off_alignment(dev, cols, tabs, dtype):
    for width, shift in ((8, 1), (cols, 1), (cols, 3), (12, 2)):
        ids, mask = D.random_rows(11, width, seed=90 + width + shift, dtype=dtype)
        check(dev, "dev", ids, mask, tabs, ("shift", width, shift), shift=shift)


@pytest.mark.parametrize("form", FORMS)
def test_scan_group_seam(dev, tabs, form):
    group = dev.decode_capacity()[1]
    assert group == 1024
    for rows in (group - 1, group, group + 1):
        ids, mask = D.random_rows(rows, 2, seed=rows)
        check(dev, form, ids, mask, tabs, ("rows", rows))


def test_capacity_one_byte_short(dev, tabs):
    ids, mask = D.random_rows(11, 37, seed=5)
    want = D.decode(ids, mask, tabs)
    total = int(want[3][0])
    text_off = dev.decode_plan(ids, mask, tabs[1], tabs[2], tabs[3])[0]
    with pytest.raises(dev.SwtError) as e:
        dev.decode_rows(ids, mask, *tabs, text_off, text_cap=total - 1)
    assert e.value.code == dev.ERR_CAPACITY
    got = run(dev, "dev", ids, mask, tabs, text_cap=total - 1)  # asserts that the last byte stayed as it was
    assert np.array_equal(got[0], want[0][:total - 1])
    got = run(dev, "dev", ids, mask, tabs, text_cap=int(want[1][5]) + 1)  # the cap inside a row
    assert np.array_equal(got[0], want[0][:int(want[1][5]) + 1])


@pytest.mark.parametrize("form", FORMS)
def test_no_rows(dev, tabs, form):
    for width in (0, 5):
        got = run(dev, form, np.zeros((0, width), dtype=np.int32), None, tabs)
        assert got[0].size == 0 and got[1].tolist() == [0] and got[2].size == 0 and got[3].tolist() == [0, 0, 0]


# ---- the tokenizer classes, end to end

RESOURCES = {"FastBPE": "FastBPE", "NaiveBPE": "FastBPE", "FastWP": "FastWordPiece", "NaiveWP": "FastWordPiece"}


@pytest.fixture(scope="module")
def toks(swt, dev, ref_dir):
    out = {}
    for cls, res in RESOURCES.items():
        out[cls] = getattr(swt, cls)()
        out[cls].load_resources(os.path.join(ref_dir, "resources/pretrained", res))
    return out


def as_numpy(x):
    return x if isinstance(x, np.ndarray) else x.cpu().numpy()


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("cls", ["FastBPE", "FastWP"])
def test_round_trip_equals_the_reference(toks, corpora, golden, cls, device):
    """decode_batch(encode_batch(texts)) is the reference's recover_sentence of the reference's recorded tokens, all 989 rows"""
    want = golden("recover_sentence.json")["pan_tadeusz"][RESOURCES[cls]]
    out = toks[cls].encode_batch(corpora["pan"], device=device, int64=device)
    got = toks[cls].decode_batch(out["input_ids"], out["attention_mask"])
    assert len(got) == len(want) == 989
    assert got == want
    assert got == toks[cls].decode_batch(out["input_ids"])  # skipping [PAD] does what the mask does
    text, off = toks[cls].decode_batch_bytes(out["input_ids"], out["attention_mask"])
    assert isinstance(text, np.ndarray) != device and as_numpy(off).dtype == np.uint64 and as_numpy(text).dtype == np.uint8
    assert as_numpy(text).tobytes().decode("utf-8") == "".join(want)


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("cls", ["NaiveBPE", "NaiveWP"])
def test_round_trip_of_the_naive_classes(toks, corpora, cls, device):
    texts = corpora["pan"][:120]
    known = set(toks[cls].vocab_list())
    want = [D.join([t if t in known else "[UNK]" for t in row]) for row in toks[cls].tokenize_batch(texts)]
    out = toks[cls].encode_batch(texts, device=device)
    assert toks[cls].decode_batch(out["input_ids"], out["attention_mask"]) == want


def test_packed_batch(toks, corpora):
    tok, texts = toks["FastWP"], corpora["pan"][:60]
    out = tok.encode_batch(texts, max_length=512, packing="whole", device=True)
    assert out["n_truncated"] == 0 and out["input_ids"].shape[0] < len(texts)
    rows = [[] for _ in range(out["input_ids"].shape[0])]
    for row, tokens in zip(as_numpy(out["segment_row"]).tolist(), tok.tokenize_batch(texts)):
        rows[row] += tokens
    assert tok.decode_batch(out["input_ids"], out["attention_mask"]) == [D.join(r) for r in rows]


@pytest.mark.parametrize("device", [False, True])
def test_masked_batch(toks, corpora, device):
    tok = toks["FastBPE"]
    out = tok.encode_batch(corpora["pan"][:60], device=device, mlm={"seed": 3, "probability": 0.3})
    assert out["n_masked"] > 0 and tok.mask_id() == len(tok.vocab_list())
    ids, mask = as_numpy(out["input_ids"]), as_numpy(out["attention_mask"])
    tabs = D.tables(tok.vocab_list(), tok.mask_id())
    for skip in (True, False):
        text, off, status, _ = D.decode(ids, mask, tabs, D.SKIP_SPECIAL if skip else 0)
        got = tok.decode_batch(out["input_ids"], out["attention_mask"], skip_special_tokens=skip)
        assert got == D.strings(text, off) and not status.any()
        assert any("[MASK]" in s for s in got) != skip and all(s.startswith("[CLS]") for s in got) != skip


def test_decode_one_sequence_and_reported_rows(toks):
    tok = toks["FastWP"]
    ix = {t: i for i, t in enumerate(tok.vocab_list())}
    seq = [ix["[CLS]"], ix["l"], ix["##i"], ix["!"], ix["[SEP]"], ix["[PAD]"]]
    assert tok.decode(seq) == "li !" and tok.decode(np.array(seq, dtype=np.int32), skip_special_tokens=False) == "[CLS] li ! [SEP] [PAD]"
    import torch
    assert tok.decode(torch.tensor(seq, device="cuda")) == "li !"
    ids = np.array([[ix["l"], ix["[PAD]"]], [ix["l"], -1], [len(ix) + 5, ix["[PAD]"]]], dtype=np.int64)
    for given in (ids, torch.from_numpy(ids).cuda()):
        with pytest.raises(ValueError, match="row 1 holds an id outside the vocabulary"):
            tok.decode_batch(given)
    mask = np.array([[1, 1], [1, 0], [0, 1]], dtype=np.uint8)
    assert tok.decode_batch(ids, mask) == ["l", "l", ""]
