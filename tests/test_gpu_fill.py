"""swt_mlm_positions and swt_mlm_predict on the GPU, host and `_dev` forms, against the NumPy model (tests/fill_cases.py): element
by element and `info` included, out_lse alone within lse_tol of the float64 model.  The shapes are the smallest that reach each
seam of the kernels, the seams placed from swt_fill_capacity: rows shorter than a quad, of one, two and three steps with and
without a peeled head and tail, logits at every offset from 16-byte alignment, positions that fill a workgroup and do not, counts
that cross the scan groups of the positions call.  Every `_dev` output lies behind fence bytes before and after it, and an output
that is not given stays unwritten."""
import math
import os

import numpy as np
import pytest

from tests import fill_cases as F

pytestmark = pytest.mark.gpu

FENCE, GARBAGE, FRONT, BACK = 0xEE, 0x5A, 64, 64
FORMS = ["host", "dev"]
OUT = (("lse", np.float32), ("top_id", np.int32), ("top_logit", np.float32), ("label_id", np.int32), ("label_logit", np.float32),
       ("label_rank", np.int32))
WORST = {}  # V -> the largest error of a finite lse seen, in units of 2^-24 max(1, |lse|)


@pytest.fixture(scope="module")
def dev(native):
    if native.device_count() < 1:
        pytest.fail("no HIP device")
    native.init(0)
    return native


@pytest.fixture(scope="module")
def capacity(dev):
    yield dev.fill_capacity()
    for V in sorted(WORST):  # what DESIGN.md 4.16 quotes
        print("lse: V %d, largest error %.3f x 2^-24 max(1, |lse|) (lse_tol at lse 0: %.1f x 2^-24)"
              % (V, WORST[V], F.lse_tol(V, dev.fill_capacity()[0]) / F.U))


class Device:
    """the arrays of one `_dev` call: inputs uploaded `shift` elements off 16-byte alignment, every output behind FRONT fence bytes
    (and `shift` elements) and before BACK more; an output that is not given is still laid out, and must come back untouched"""

    def __init__(self, shift=0):
        import torch
        self.torch, self.shift, self.keep, self.outs = torch, shift, [], {}

    def up(self, a):
        if a is None:
            return None
        a = np.ascontiguousarray(a)
        flat = np.concatenate([np.zeros(self.shift, dtype=a.dtype), a.reshape(-1), np.zeros(4, dtype=a.dtype)])
        t = self.torch.from_numpy(flat.view(np.uint8)).cuda()
        self.keep.append(t)
        assert t.data_ptr() % 16 == 0
        return t.data_ptr() + self.shift * a.dtype.itemsize

    def out(self, name, shape, dtype, given=True):
        size = np.dtype(dtype).itemsize
        n, lead = int(np.prod(shape)) * size, FRONT + self.shift * size
        h = np.full(lead + n + BACK, GARBAGE, dtype=np.uint8)
        h[:lead] = FENCE
        h[lead + n:] = FENCE
        t = self.torch.from_numpy(h).cuda()
        self.outs[name] = (t, lead, n, shape, dtype, given)
        return t.data_ptr() + lead if given else None

    def collect(self):
        self.torch.cuda.synchronize()
        res = {}
        for name, (t, lead, n, shape, dtype, given) in self.outs.items():
            h = t.cpu().numpy()
            assert (h[:lead] == FENCE).all() and (h[lead + n:] == FENCE).all(), "%s: a byte outside the output was written" % name
            body = h[lead:lead + n].copy()
            if not given:
                assert (body == GARBAGE).all(), "%s was not given and was written" % name
            res[name] = body.view(dtype).reshape(shape) if given else None
        return res


def agree(got, want, what, V=None, step=None, lse_bound=None):
    """element by element; lse within lse_tol(V, step) -- or lse_bound(lse) -- of the float64 model where that is finite"""
    for k, g in got.items():
        w = want[k]
        if g is None:
            continue
        assert w is not None, (what, k)
        if k == "lse":
            assert g.dtype == np.float32 and g.shape == w.shape, (what, k, g.dtype, g.shape, w.shape)
            finite = np.isfinite(w)
            assert np.array_equal(np.isfinite(g), finite) and np.array_equal(g[~finite].astype(np.float64), w[~finite], equal_nan=True), (what, k, g, w)
            for a, b in zip(g[finite].astype(np.float64), w[finite]):
                err = abs(a - b)
                tol = lse_bound(b) if lse_bound else F.lse_tol(V, step, b)
                WORST[V] = max(WORST.get(V, 0.0), err / F.U / max(1.0, abs(b)))
                assert err <= tol, (what, k, a, b, err / F.U, tol / F.U)
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        if not np.array_equal(g, w, equal_nan=g.dtype.kind == "f"):
            bad = np.argwhere(~((g == w) | ((g != g) & (w != w))))
            raise AssertionError("%s: %s differs at %d places, first %s: got %s, want %s"
                                 % (what, k, len(bad), bad[0].tolist(), g[tuple(bad[0])], w[tuple(bad[0])]))


def run_positions(dev, form, ids, value, not_equal, shift=0, what=""):
    want = F.expected_positions(ids, value, not_equal)
    rows, width = ids.shape
    if form == "host":
        pos, info = dev.mlm_positions(ids, value, not_equal)
        got = {"pos": pos, "info": info}
    else:
        d = Device(shift)
        dev.check(dev.lib().swt_mlm_positions_dev(d.up(ids), rows, width, int(value), int(not_equal), 4 if ids.dtype == np.int64 else 0,
                                                  d.out("pos", (rows * width,), np.uint64), d.out("info", (2,), np.uint64), None))
        got = d.collect()
    agree(got, want, ("positions", what, form, str(ids.dtype), value, not_equal))
    return want


def run_predict(dev, capacity, form, x, pos, labels=None, k=0, shift=0, given=None, lse_bound=None, what=""):
    """both forms give the model's arrays; the host form is not given positions outside the rows"""
    rows, width, V = x.shape
    pos = np.asarray(pos, dtype=np.uint64)
    want = F.expected_predict(x, pos, labels, k)
    n = pos.size
    if form == "host":
        got = dev.mlm_predict(x, pos, labels, k)
    else:
        d = Device(shift)
        on = lambda name: (given is None or name in given) and want[name] is not None
        args = [d.up(x), rows, width, V, d.up(pos), n, d.up(labels), 4 if labels is not None and labels.dtype == np.int64 else 0, k]
        args += [d.out(name, (n, k) if name.startswith("top") else (n,), t, on(name)) for name, t in OUT]
        args += [d.out("info", (5,), np.uint64, given is None or "info" in given), None]
        dev.check(dev.lib().swt_mlm_predict_dev(*args))
        got = d.collect()
    agree(got, want, ("predict", what, form, V, k, shift), V, capacity[0], lse_bound)
    return want


def vocab_sizes(s):
    return (1, 2, 3, 4, 5, 63, 64, 65, s - 1, s, s + 1, 2 * s + 1, 3 * s + 3)


# ---- the rows of logits

@pytest.mark.parametrize("form", FORMS)
def test_vocab_sizes(dev, capacity, form):
    """every V across the quad, the step and its multiples, all cells of a 2 x 3 batch and a few of them, k = 5 below and above V"""
    rng = np.random.default_rng(11)
    for V in vocab_sizes(capacity[0]):
        x = F.logits_of([F.normal_row(rng, V) for _ in range(6)], 2, 3)
        labels = rng.integers(0, V, size=(2, 3)).astype(np.int32)
        run_predict(dev, capacity, form, x, np.arange(6), labels, 5)
        run_predict(dev, capacity, form, x, [4, 1], labels.astype(np.int64), 1)


@pytest.mark.parametrize("form", FORMS)
def test_one_long_row(dev, capacity, form):
    rng = np.random.default_rng(12)
    V = 70001
    x = F.logits_of([F.normal_row(rng, V) for _ in range(2)], 1, 2)
    run_predict(dev, capacity, form, x, [1], np.array([[3, V - 1]], dtype=np.int32), 5)


@pytest.mark.parametrize("k", [0, 1, 2, 5, 8, 63, 64])
def test_k_below_at_and_above_the_vocabulary(dev, capacity, k):
    rng = np.random.default_rng(13 + k)
    for V in sorted({1, max(k - 1, 1), max(k, 1), k + 1, 2 * capacity[0] + 3}):
        x = F.logits_of([F.normal_row(rng, V) if i % 2 else F.tie_row(rng, V, 3) for i in range(4)], 2, 2)
        labels = rng.integers(0, V, size=(2, 2)).astype(np.int32)
        for form in FORMS:
            run_predict(dev, capacity, form, x, np.arange(4), labels, k, what="k")


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_logits_off_alignment(dev, capacity, shift):
    """the base 4, 8 and 12 bytes off a 16-byte boundary, crossed with V % 4: every head and tail of the peel step, in rows of no
    quad, of one step and of three"""
    rng = np.random.default_rng(20 + shift)
    s = capacity[0]
    for V0 in (4, s, 3 * s):
        for V in range(V0, V0 + 4):
            x = F.logits_of([F.tie_row(rng, V, 5) if i == 2 else F.normal_row(rng, V) for i in range(5)], 1, 5)
            labels = rng.integers(0, V, size=(1, 5)).astype(np.int64)
            run_predict(dev, capacity, "dev", x, np.arange(5), labels, 8, shift=shift, what="shift")
    x = F.logits_of([F.normal_row(rng, 2) for _ in range(5)], 1, 5)  # rows that end before the first boundary
    run_predict(dev, capacity, "dev", x, np.arange(5), None, 2, shift=shift)


@pytest.mark.parametrize("form", FORMS)
def test_position_counts(dev, capacity, form):
    """no position, one, two; a workgroup short of one, full, and one over; positions out of order and repeated"""
    rng = np.random.default_rng(30)
    per = capacity[1]
    V, rows, width = 67, 3, per + 1
    x = F.logits_of([F.normal_row(rng, V) for _ in range(rows * width)], rows, width)
    labels = rng.integers(0, V, size=(rows, width)).astype(np.int32)
    for n in (0, 1, 2, per - 1, per, per + 1, 2 * per + 1):
        run_predict(dev, capacity, form, x, rng.integers(0, rows * width, size=n), labels, 2, what="n %d" % n)
    run_predict(dev, capacity, form, x, [5, 5, 0, rows * width - 1, 5], labels, 2)


def test_outputs_not_given_stay_unwritten(dev, capacity):
    rng = np.random.default_rng(31)
    V = 130
    x = F.logits_of([F.normal_row(rng, V) for _ in range(6)], 2, 3)
    labels = rng.integers(0, V, size=(2, 3)).astype(np.int32)
    for given in (("lse",), ("top_id",), ("top_logit", "info"), ("label_rank",), ("label_id", "label_logit"), ("info",), ()):
        run_predict(dev, capacity, "dev", x, [0, 3, 5], labels, 3, given=given, what=str(given))
    run_predict(dev, capacity, "dev", x, [0, 3, 5], None, 0, given=("lse", "info"))


# ---- which cells

@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_selected_cells(dev, capacity, form, dtype):
    """none and all, a row's first or last cell alone, the tensor's first and last, both modes, a negative value"""
    rows, width = 5, 7
    rng = np.random.default_rng(40)
    base = rng.integers(0, 50, size=(rows, width)).astype(dtype)
    cases = {"none": [], "all": [(r, c) for r in range(rows) for c in range(width)], "a row's first": [(2, 0)], "a row's last": [(2, width - 1)],
             "the first and the last": [(0, 0), (rows - 1, width - 1)], "some": [(0, 3), (1, 1), (4, 0), (4, 5)]}
    for what, cells in cases.items():
        for value in (-100, -1, 103, (-1 << 40) if dtype == np.int64 else -(1 << 31)):
            ids = base.copy()
            for r, c in cells:
                ids[r, c] = value
            want = run_positions(dev, form, ids, value, False, what=what)
            assert int(want["info"][0]) == len(cells)
            # labels != value: everything but the cells
            inv = np.full((rows, width), value, dtype=dtype)
            for r, c in cells:
                inv[r, c] = base[r, c]
            want = run_positions(dev, form, inv, value, True, what=what)
            assert int(want["info"][0]) == len(cells)
    if dtype == np.int64:  # the compare is of all 64 bits and signed
        ids = np.array([[5, 5 + (1 << 32), -5, (1 << 63) - 1]], dtype=np.int64)
        for value in (5, -5, 5 + (1 << 32), (1 << 63) - 1):
            run_positions(dev, form, ids, value, False)
    run_positions(dev, "dev", base, 3, False, shift=1, what="ids off 16-byte alignment")


@pytest.mark.parametrize("form", FORMS)
def test_positions_across_the_scan_groups(dev, capacity, form):
    """cells of more than one scan group, the selected ones sparse, dense, and only behind the first group"""
    scan = capacity[3]
    rows, width = scan // 256 + 3, 257  # a width that is no multiple of anything in the kernel
    assert rows * width > scan + 256
    rng = np.random.default_rng(41)
    ids = np.where(rng.random((rows, width)) < 0.15, 7, -100).astype(np.int32)
    run_positions(dev, form, ids, -100, True, what="sparse")
    run_positions(dev, form, ids, -100, False, what="dense")
    ids[:scan // width + 1] = -100
    run_positions(dev, form, ids, -100, True, what="behind the first group")


# ---- exact sums, the order, special values

@pytest.mark.parametrize("form", FORMS)
def test_exact_sums(dev, capacity, form):
    """rows of 0.0 and -inf alone: S is an integer and lse = log(count), held to 3 x 2^-24 max(1, lse) -- a dropped or doubled
    element shows whatever the general tolerance is"""
    rng = np.random.default_rng(50)
    s = capacity[0]
    bound = lambda lse: 3.0 * F.U * max(1.0, abs(lse))
    for V, shift in ((2 * s + 3, 1), (3 * s + 2, 3), (s + 1, 0)):
        counts = [c for c in (1, 2, s, s + 1, V - 1, V) if c <= V]
        x = F.logits_of([F.zeros_row(rng, V, c) for c in counts], 1, len(counts))
        want = run_predict(dev, capacity, form, x, np.arange(len(counts)), None, 4, shift=shift, lse_bound=bound, what="zeros")
        assert np.allclose(want["lse"], np.log(counts), rtol=1e-15)


def order_rows(rng, V):
    """-> (rows, labels): the order's cases in a row of V entries"""
    asc = np.arange(V, dtype=np.float32) * 0.25 - 7.0
    last_max = F.normal_row(rng, V)
    last_max[V - 1] = 50.0  # the maximum in the last peeled element
    first_max = F.normal_row(rng, V)
    first_max[0] = 50.0
    arg = F.normal_row(rng, V)
    arg[V // 2] = 40.0  # the label as the argmax
    tied = F.tie_row(rng, V, 2)
    rows = [np.full(V, 1.5, dtype=np.float32), F.tie_row(rng, V, 3), F.tie_row(rng, V, 7), asc, asc[::-1].copy(), last_max, first_max, arg, tied,
            tied.copy(), F.normal_row(rng, V), np.full(V, -0.0, dtype=np.float32)]
    ones = np.flatnonzero(tied == 1.0)
    labels = [V // 3, V - 1, 0, V - 1, V - 1, V - 1, 0, V // 2, int(ones[0]) if ones.size else 0, int(ones[-1]) if ones.size else 0, V - 1, V - 1]
    rows[-1][::2] = 0.0  # -0.0 and 0.0 are one value: the ids decide
    return rows, labels


@pytest.mark.parametrize("form", FORMS)
def test_order(dev, capacity, form):
    """all entries equal (the top-k is ids 0 .. k - 1, the rank the label); ties from small integers across lanes, steps and the
    peels; ascending (every entry enters the list) and descending rows; the maximum in the last peeled element; the label as the
    argmax, tied with smaller and larger ids, and last"""
    rng = np.random.default_rng(60)
    s = capacity[0]
    for V, shift, k in ((2 * s + 3, 1, 8), (s + 6, 2, 64), (7, 3, 5)):
        rows, labels = order_rows(rng, V)
        x = F.logits_of(rows, 1, len(rows))
        lab = np.array([labels], dtype=np.int32)
        want = run_predict(dev, capacity, form, x, np.arange(len(rows)), lab, k, shift=shift, what="order")
        assert want["top_id"][0].tolist() == list(range(min(k, V))) + [-1] * (k - min(k, V)) and want["label_rank"][0] == V // 3
        assert want["label_rank"][3] == 0 and want["label_rank"][4] == V - 1 and want["label_rank"][7] == 0 and want["label_rank"][5] == 0


@pytest.mark.parametrize("form", FORMS)
def test_special_values(dev, capacity, form):
    """NaN at the start, in the middle and at the end, all NaN, fewer than k entries that are no NaN, +inf once and twice, all -inf"""
    rng = np.random.default_rng(70)
    s = capacity[0]
    nan, inf = np.float32("nan"), np.float32("inf")
    for V, shift in ((2 * s + 3, 1), (9, 0)):
        rows = [F.normal_row(rng, V) for _ in range(10)]
        rows[0][0] = nan
        rows[1][V // 2] = nan
        rows[2][V - 1] = nan
        rows[3][:] = nan
        rows[4][:] = nan
        rows[4][[1, V - 2]] = [2.0, 2.0]  # two entries against k = 5
        rows[5][V // 3] = inf
        rows[6][[2, V - 1]] = inf
        rows[7][:] = -inf
        rows[8][V // 2] = -inf
        rows[9][[0, V - 1]] = [inf, nan]
        x = F.logits_of(rows, 2, 5)
        labels = np.array([[0, 1, V - 1, 2, 1], [V // 3, V - 1, 0, V // 2, 0]], dtype=np.int64)
        want = run_predict(dev, capacity, form, x, np.arange(10), labels, 5, shift=shift, what="special")
        assert want["info"].tolist()[3] == 6 and want["top_id"][4].tolist() == [1, V - 2, -1, -1, -1] and want["lse"][7] == -inf


@pytest.mark.parametrize("form", FORMS)
def test_labels_out_of_range(dev, capacity, form):
    rng = np.random.default_rng(80)
    V = 300
    x = F.logits_of([F.normal_row(rng, V) for _ in range(6)], 2, 3)
    labels = np.array([[-100, -1, V], [1 << 31, V - 1, (1 << 32) + 5]], dtype=np.int64)
    want = run_predict(dev, capacity, form, x, np.arange(6), labels, 3)
    assert want["info"].tolist()[4] == 5 and want["label_id"].tolist() == [-1, -1, -1, -1, V - 1, -1]
    run_predict(dev, capacity, form, x, np.arange(6), np.array([[-100, -1, V], [0, V - 1, -(1 << 31)]], dtype=np.int32), 3)


def test_dev_form_with_positions_outside_the_rows(dev, capacity):
    """UINT64_MAX (what swt_mlm_positions leaves behind the count) and rows * width: the "nothing" record and no read"""
    rng = np.random.default_rng(81)
    V = 2 * capacity[0] + 1
    x = F.logits_of([F.normal_row(rng, V) for _ in range(4)], 2, 2)
    labels = rng.integers(0, V, size=(2, 2)).astype(np.int32)
    pos = np.array([0, F.NO_POS, 3, 4, 1 << 40, 2], dtype=np.uint64)
    want = run_predict(dev, capacity, "dev", x, pos, labels, 3)
    assert want["top_id"][1].tolist() == [-1, -1, -1] and math.isnan(want["lse"][3]) and want["info"].tolist()[0] == 6
    with pytest.raises(dev.SwtError, match="pos"):
        dev.mlm_predict(x, pos, labels, 3)


# ---- through the classes

def _tokenizer(swt, ref_dir, cls):
    tok = getattr(swt, cls)()
    tok.load_resources(os.path.join(ref_dir, "resources/tests", "FastBPE" if "BPE" in cls else "FastWordPiece"))
    return tok


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else a


@pytest.mark.parametrize("cls", ["FastBPE", "FastWP", "NaiveBPE", "NaiveWP"])
def test_fill_mask_and_mlm_scores_end_to_end(swt, dev, capacity, ref_dir, corpora, cls):
    """rows masked by encode_batch(mlm=...) with every selected token a [MASK]; logits in which each label is the argmax by a
    margin: mlm_scores is right everywhere, fill_mask puts the label first, the rows with the winners filled in decode as the
    unmasked rows do, and the NumPy and torch paths agree"""
    import torch
    tok = _tokenizer(swt, ref_dir, cls)
    texts = list(corpora["t5k"])[:48]  # the test vocabularies are small: most of a text's tokens are [UNK] and never selected
    kw = {"max_length": 24, "padding": "max_length"}
    plain = tok.encode_batch(texts, **kw)
    V = max(len(tok.vocab_list()), tok.mask_id() + 1)
    results = []
    for device in (False, True):
        masked = tok.encode_batch(texts, device=device, mlm={"probability": 0.5, "seed": 9, "mask_share": 1.0, "random_share": 0.0}, **kw)
        ids, labels = _np(masked["input_ids"]), _np(masked["labels"])
        on = labels != -100
        assert on.sum() >= 3 and np.array_equal(on, ids == tok.mask_id()) and np.array_equal(labels[on], plain["input_ids"][on])
        rng = np.random.default_rng(90)
        x = rng.standard_normal((ids.shape[0], ids.shape[1], V)).astype(np.float32)
        r, c = np.nonzero(on)
        x[r, c, labels[on]] = 12.0  # the label above every other entry by a margin
        logits = torch.from_numpy(x).cuda() if device else x
        scores = tok.mlm_scores(logits, masked["labels"], top_k=3)
        assert scores["n_positions"] == on.sum() == scores["n_correct"] == scores["n_correct_at_k"] and scores["accuracy"] == 1.0
        assert scores["n_nan"] == 0 and scores["n_out_of_range"] == 0
        assert not _np(scores["label_rank"]).any() and np.array_equal(_np(scores["label"]), labels[on])
        assert np.array_equal(_np(scores["row"]), r) and np.array_equal(_np(scores["col"]), c)
        want = F.expected_predict(x, r * ids.shape[1] + c, labels, 3)
        assert np.array_equal(_np(scores["token_ids"]), want["top_id"]) and np.array_equal(_np(scores["logit"]), want["top_logit"])
        lp = want["label_logit"].astype(np.float64) - want["lse"]
        assert np.allclose(_np(scores["label_logprob"]), lp, rtol=0, atol=2 * F.lse_tol(V, capacity[0], 12.0) + 12.0 * F.U)
        assert float(scores["loss"]) == pytest.approx(-lp.mean(), abs=1e-5) and float(scores["perplexity"]) == pytest.approx(math.exp(-lp.mean()), rel=1e-4)
        filled = tok.fill_mask(masked["input_ids"], logits, top_k=2, tokens=True)
        assert filled["n_positions"] == on.sum() and np.array_equal(_np(filled["token_ids"]), want["top_id"][:, :2])
        assert np.array_equal(_np(filled["row"]), r) and np.array_equal(_np(filled["col"]), c)
        assert np.allclose(_np(filled["score"]), np.exp(_np(filled["logprob"]))) and (_np(filled["score"])[:, 0] > 0.5).all()
        names = tok.vocab_list()
        assert [t[0] for t in filled["tokens"]] == [names[i] if i < len(names) else "[MASK]" for i in labels[on]]
        back = ids.copy()
        back[r, c] = _np(filled["token_ids"])[:, 0]
        assert np.array_equal(back, plain["input_ids"]) and tok.decode_batch(back) == tok.decode_batch(plain["input_ids"])
        results.append((scores, filled))
    for a, b in zip(results[0], results[1]):
        for key in a:
            va, vb = _np(a[key]), _np(b[key])
            if key in ("loss", "perplexity"):  # a float64 mean, in each library's own order
                continue
            if key == "score":  # exp of equal log-probabilities, by NumPy and by torch
                assert np.allclose(va, vb, rtol=1e-6, atol=0), key
                continue
            if isinstance(va, np.ndarray):
                assert va.dtype == vb.dtype and np.array_equal(va, vb, equal_nan=va.dtype.kind == "f"), key
            else:
                assert va == vb, key
    assert float(results[0][0]["loss"]) == pytest.approx(float(results[1][0]["loss"]), abs=1e-6)
