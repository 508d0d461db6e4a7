"""swt_label_words, swt_answer_positions and swt_answer_best on the GPU, host and `_dev` forms, against the NumPy model
(tests/label_cases.py), element by element and `info` included, at the smallest shapes that reach each seam of the kernels -- the
seams placed from swt_label_capacity: the scalar and the wide path, one, two and three steps a row, rows that share a wavefront
and a last wavefront that is partly dead, words, answers and span windows laid across quad, lane and step seams, texts whose rows
cross the workgroups of the reduction.  Every `_dev` output lies behind fence bytes before and after it."""
import json
import os

import numpy as np
import pytest

from tests import label_cases as L

pytestmark = pytest.mark.gpu

FENCE, GARBAGE, FRONT, BACK = 0xEE, 0x5A, 64, 64
FORMS = ["host", "dev"]


@pytest.fixture(scope="module")
def dev(native):
    if native.device_count() < 1:
        pytest.fail("no HIP device")
    native.init(0)
    return native


@pytest.fixture(scope="module")
def cols(dev):
    return dev.label_capacity()[0]


def widths(cols):
    return (1, 3, 4, 5, 63, 64, 65, cols - 1, cols, cols + 1, 2 * cols + 1)


class Device:
    """the arrays of one `_dev` call: inputs uploaded (`shift` elements off 16-byte alignment), every output behind FRONT fence
    bytes and before BACK more (`shift` elements further in)"""

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
        return t.data_ptr() + self.shift * a.dtype.itemsize

    def out(self, name, shape, dtype, given=True):
        n, lead = int(np.prod(shape)) * np.dtype(dtype).itemsize, FRONT + self.shift * np.dtype(dtype).itemsize
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


def agree(got, want, what):
    for k, g in got.items():
        if g is None:
            continue
        w = want[k]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        if not np.array_equal(g, w, equal_nan=g.dtype.kind == "f"):
            bad = np.argwhere(g != w)
            raise AssertionError("%s: %s differs at %d places, first %s: got %s, want %s"
                                 % (what, k, len(bad), bad[0].tolist(), g[tuple(bad[0])], w[tuple(bad[0])]))


# ---- 1. word labels

def run_labels(dev, form, b, lab_off, lab, side=0, inside=None, all_tokens=False, ids64=False, status=True, info=True, shift=0, what=""):
    want = L.expected_labels(b["word"], lab_off, lab, b["seq"], side, b["sample"], inside, all_tokens, dtype=np.int64 if ids64 else np.int32)
    rows, width = b["word"].shape
    if form == "host":
        got = dev.label_words(b["word"], lab_off, lab, b["seq"], side, b["sample"], inside, all_tokens, ids64, status=status, info=info)
    else:
        d = Device(shift)
        args = (d.up(b["word"]), d.up(b["seq"]), side, d.up(b["sample"]), rows, width, d.up(np.asarray(lab_off, dtype=np.uint64)),
                d.up(np.asarray(lab, dtype=np.int32)), len(lab), len(lab_off) - 1, d.up(None if inside is None else np.asarray(inside, dtype=np.int32)),
                0 if inside is None else len(inside), L.IGNORE, (dev.LABEL_ALL_TOKENS if all_tokens else 0) | (dev.LABEL_IDS64 if ids64 else 0),
                d.out("labels", (rows, width), np.int64 if ids64 else np.int32), d.out("status", (rows,), np.uint8, status),
                d.out("info", (4,), np.uint64, info), None)
        dev.check(dev.lib().swt_label_words_dev(*args))
        got = d.collect()
    agree(got, want, (what, form, ids64))
    return want


def label_case(rows, width, seed, pair, **kw):
    b = L.make_rows(rows, width, seed=seed, pair=pair, **kw)
    if rows > 2:
        b["sample"][rows // 2] = b["n_samples"] + 5  # a row of no text
    lab_off, lab = L.make_labels(b, 1 if pair else 0, seed, short=(0,) if rows > 4 else ())
    return b, lab_off, lab


INSIDE = np.array([0, 2, 2, 4, 4, 6, 6], dtype=np.int32)


@pytest.mark.parametrize("ids64", [False, True])
@pytest.mark.parametrize("form", FORMS)
def test_label_widths(dev, cols, form, ids64):
    """the scalar and the wide path; one, two and three steps a row; 11 rows, so that groups of every size leave a wavefront
    partly dead; single rows and side 1 of pair rows; a row of no text and a text with a label too few"""
    for n, width in enumerate(widths(cols)):
        pair = width >= 5 and n % 2 == 1
        b, lab_off, lab = label_case(11, width, width, pair, fill=None if width < 64 else width - n % 3)
        for all_tokens, inside in ((False, None), (True, None), (True, INSIDE)):
            want = run_labels(dev, form, b, lab_off, lab, 1 if pair else 0, inside, all_tokens, ids64, what=("width", width))
        assert width < 16 or (want["info"][0] > 0 and want["info"][3] == 1)
    assert want["info"][2] > 0


@pytest.mark.parametrize("form", FORMS)
def test_label_row_counts(dev, form):
    """several narrow rows share a wavefront (widths 3 and 4: one lane a row, 5 and 8: two): 1, 2, 65 and 257 rows"""
    for width in (3, 4, 5, 8):
        for rows in (1, 2, 65, 257):
            b, lab_off, lab = label_case(rows, width, rows + width, False, specials=False)
            run_labels(dev, form, b, lab_off, lab, what=("rows", rows, width), status=rows != 65, info=rows != 2)


@pytest.mark.parametrize("ids64", [False, True])
@pytest.mark.parametrize("form", FORMS)
def test_label_words_across_the_seams(dev, cols, form, ids64):
    """a word of cols_per_step + 5 tokens across every quad, lane and step seam, from four starting columns, column 0 among
    them; words of two tokens astride every column; the same word index on both sides of a [SEP]; a row that is one word"""
    width = 2 * cols + 7
    word = np.full((8, width), -1, dtype=np.int32)
    for r in range(4):  # single tokens, then the long word from column r on, then single tokens
        word[r, :r] = np.arange(r)
        word[r, r:r + cols + 5] = r
        word[r, r + cols + 5:] = np.arange(r + 1, r + 1 + width - (r + cols + 5))
    word[4] = np.arange(width) // 2          # pairs that start on even columns
    word[5] = (np.arange(width) + 1) // 2    # and on odd ones
    word[6] = 0                              # one word from end to end
    word[7] = np.arange(width) // 3
    seq = np.zeros((8, width), dtype=np.int8)
    for c in (3, 4, cols - 1, cols, cols + 1, 2 * cols):  # a [SEP] inside a word: what follows is the first column of its word again
        seq[7, c] = -1
    seq[6, cols:] = 1  # the other side takes over in the middle of a word, at a step seam
    b = {"word": word, "seq": None, "sample": np.zeros(8, dtype=np.uint32)}
    lab = np.arange(1, width + 2, dtype=np.int32) % 7
    for all_tokens, inside in ((False, None), (True, INSIDE)):
        want = run_labels(dev, form, b, [0, width + 1], lab, 0, inside, all_tokens, ids64, what="long words")
        if not all_tokens:
            assert ((want["labels"][0] != L.IGNORE).sum(), (want["labels"][6] != L.IGNORE).sum()) == (width - cols - 4, 1)
        for side in (0, 1):
            run_labels(dev, form, dict(b, seq=seq), [0, width + 1], lab, side, inside, all_tokens, ids64, what=("long words, seq", side))


@pytest.mark.parametrize("ids64", [False, True])
def test_label_pointers_off_16_bytes(dev, cols, ids64):
    """every pointer one element off: the width is a multiple of four and the wide path still must not be taken"""
    for width in (8, cols + 4):
        b, lab_off, lab = label_case(5, width, width, True)
        run_labels(dev, "dev", b, lab_off, lab, 1, INSIDE, True, ids64, shift=1, what=("shifted", width))


# ---- 2. answer positions

def run_positions(dev, form, b, ans, side=0, cls=False, pad_left=False, ids64=False, has=True, hit=True, info=True, shift=0, what=""):
    t = np.int64 if ids64 else np.int32
    want = L.expected_positions(b["spans"], ans, b["word"], b["seq"], side, b["sample"], b["length"], cls, pad_left, dtype=t)
    rows, width = b["spans"].shape[:2]
    ans = np.ascontiguousarray(ans, dtype=np.uint32).reshape(-1, 2)
    if form == "host":
        got = dev.answer_positions(b["spans"], ans, b["word"], b["seq"], side, b["sample"], b["length"], cls, pad_left, ids64, has=has, hit=hit,
                                   info=info)
    else:
        d = Device(shift)
        flags = (dev.ANSWER_CLS if cls else 0) | (dev.ANSWER_PAD_LEFT if pad_left else 0) | (dev.LABEL_IDS64 if ids64 else 0)
        args = (d.up(b["spans"]), d.up(b["word"]), d.up(b["seq"]), side, d.up(b["sample"]), rows, width, d.up(ans), ans.shape[0], d.up(b["length"]),
                L.IGNORE, flags, d.out("start", (rows,), t), d.out("end", (rows,), t), d.out("has", (rows,), np.uint8, has),
                d.out("hit", (ans.shape[0],), np.uint8, hit), d.out("info", (3,), np.uint64, info), None)
        dev.check(dev.lib().swt_answer_positions_dev(*args))
        got = d.collect()
    agree(got, want, (what, form, ids64))
    return want


@pytest.mark.parametrize("ids64", [False, True])
@pytest.mark.parametrize("form", FORMS)
def test_position_widths(dev, cols, form, ids64):
    """random rows and answers at every width: single and pair rows, both paddings, with and without [CLS]"""
    seen = 0
    for n, width in enumerate(widths(cols)):
        pair, pad_left = width >= 5 and n % 2 == 1, n % 3 == 1
        b = L.make_rows(11, width, seed=width, pair=pair, pad_left=pad_left, fill=None if width < 64 else width - n % 3)
        if width > 4:
            b["sample"][5] = b["n_samples"] + 1
        side = 1 if pair else 0
        ans = L.make_answers(b, side, width)
        for cls in (False, True):
            want = run_positions(dev, form, b, ans, side, cls, pad_left and cls, ids64, what=("width", width))
        seen += int(want["info"][0])
        run_positions(dev, form, dict(b, sample=None), np.resize(ans, (11, 2)), side, True, False, ids64, has=n % 2 == 0, hit=n % 2 == 1,
                      info=n % 4 != 0, what=("width, no sample", width))
    assert seen > 20


@pytest.mark.parametrize("form", FORMS)
def test_position_and_best_row_counts(dev, form):
    """several narrow rows share a wavefront (widths 3 and 4: one lane a row, 5 and 8: two): 1, 2, 65 and 257 rows"""
    for width in (3, 4, 5, 8):
        for rows in (1, 2, 65, 257):
            b = L.make_rows(rows, width, seed=rows + width, specials=False, pad_left=width == 5)
            run_positions(dev, form, b, L.make_answers(b, 0, rows), what=("rows", rows, width))
            sl, el = L.small_logits((rows, width), rows, -2, 3), L.small_logits((rows, width), width, -2, 3)
            run_best(dev, form, b, sl, el, b["n_samples"], 2, what=("rows", rows, width))


@pytest.mark.parametrize("form", FORMS)
def test_position_boundaries(dev, cols, form):
    """token c of a full row of 2 cols + 7 columns spans [3 c, 3 c + 2): the answer's boundaries at c0, at c1, on each side of
    the lane, quad and step seams, in the gap between two tokens, one code point past the last token"""
    width = 2 * cols + 7
    places = sorted({1, 2, 3, 4, 5, 255, cols - 1, cols, cols + 1, 2 * cols - 1, 2 * cols, 2 * cols + 1, width - 3, width - 2})
    cases = [(a, e) for a in places for e in places if a <= e]
    rows = len(cases) * 3 + 2
    spans = np.zeros((rows, width, 2), dtype=np.uint32)
    word = np.full((rows, width), -1, dtype=np.int32)
    c = np.arange(1, width - 1)  # [CLS] tokens [SEP]
    spans[:, 1:width - 1, 0], spans[:, 1:width - 1, 1], word[:, 1:width - 1] = 3 * c, 3 * c + 2, c
    ans = []
    for a, e in cases:
        ans += [(3 * a, 3 * e + 2), (3 * a - 1, 3 * e + 3), (3 * a + 1, 3 * e + 1)]  # exact; in the gaps around; inside the tokens
    ans += [(3, 3 * (width - 2) + 3), (2, 5)]  # one code point past the last token; one before the first
    b = {"word": word, "seq": None, "spans": spans, "sample": None, "length": np.full(rows, width, dtype=np.uint32)}
    want = run_positions(dev, form, b, ans, cls=True, what="boundaries")
    got = [(int(s), int(e), int(h)) for s, e, h in zip(want["start"], want["end"], want["has"])]
    for k, (a, e) in enumerate(cases):
        assert got[3 * k] == (a, e, 1)
        assert got[3 * k + 1] == ((a - 1, e + 1, 1) if a > 1 and e < width - 2 else (0, 0, 0))  # else it lies outside the tokens
        assert got[3 * k + 2] == ((a, e, 1) if a < e else (0, 0, 0))  # inside one token: start + 1 >= end + 1, no answer
    assert got[-2:] == [(0, 0, 0), (0, 0, 0)]


def test_position_pointers_off_16_bytes(dev, cols):
    for width in (8, cols + 4):
        b = L.make_rows(7, width, seed=width, pair=True, pad_left=True)
        run_positions(dev, "dev", b, L.make_answers(b, 1, 3), 1, True, True, True, shift=1, what=("shifted", width))


# ---- 3. best spans

TEXT = ("score", "null_score", "row", "start_col", "end_col", "char_start", "char_end")
ROW = ("row_score", "row_start", "row_end")


def run_best(dev, form, b, sl, el, n_samples, max_len, side=0, cls=False, pad_left=False, per_row=True, info=True, shift=0, what=""):
    want = L.expected_best(sl, el, b["spans"], n_samples, b["word"], b["seq"], side, b["sample"], max_len, b["length"], cls, pad_left)
    rows, width = sl.shape
    if form == "host":
        got = dev.answer_best(sl, el, b["spans"], n_samples, b["word"], b["seq"], side, b["sample"], max_len, b["length"], cls, pad_left,
                              per_row=per_row, info=info)
    else:
        d = Device(shift)
        types = dict(dev.BEST_TEXT + dev.BEST_ROW)
        flags = (dev.ANSWER_CLS if cls else 0) | (dev.ANSWER_PAD_LEFT if pad_left else 0)
        args = (d.up(sl), d.up(el), d.up(b["spans"]), d.up(b["word"]), d.up(b["seq"]), side, d.up(b["sample"]), rows, width, n_samples, max_len,
                d.up(b["length"]), flags, *[d.out(k, (n_samples,), types[k]) for k in TEXT], *[d.out(k, (rows,), types[k], per_row) for k in ROW],
                d.out("info", (2,), np.uint64, info), None)
        dev.check(dev.lib().swt_answer_best_dev(*args))
        got = d.collect()
    agree(got, want, (what, form, max_len))
    return want


@pytest.mark.parametrize("form", FORMS)
def test_best_widths(dev, cols, form):
    """every width, max_len in {1, 2, 5, width, width + 7}: logits of small integers, so that sums are exact and ties real"""
    for n, width in enumerate(widths(cols)):
        pair, pad_left = width >= 5 and n % 2 == 1, n % 3 == 1
        rows = 11 if width <= cols + 1 else 5
        b = L.make_rows(rows, width, seed=width + 1, pair=pair, pad_left=pad_left, fill=None if width < 64 else width - n % 3)
        n_samples = b["n_samples"] + 1  # a text with no row
        if width > 4:
            b["sample"][rows - 1] = n_samples + 2  # a row of no text
        sl, el = L.small_logits((rows, width), width, -4, 5), L.small_logits((rows, width), width + 7, -4, 5)
        if width > 8:
            sl[1, ::3], el[1, 5], el[2, :] = np.nan, np.nan, -np.inf
        for max_len in sorted({1, 2, 5, width, width + 7}):
            want = run_best(dev, form, b, sl, el, n_samples, max_len, 1 if pair else 0, n % 2 == 0, pad_left and n % 2 == 0,
                            per_row=max_len != 2, info=max_len != 5, what=("width", width))
        assert width < 16 or want["info"][0] > 0


def full_rows(rows, width):
    """rows that are all tokens: token c spans [2 c, 2 c + 1)"""
    c = np.arange(width)
    spans = np.zeros((rows, width, 2), dtype=np.uint32)
    spans[..., 0], spans[..., 1] = 2 * c, 2 * c + 1
    return {"word": np.tile(c.astype(np.int32), (rows, 1)), "seq": None, "spans": spans, "sample": None, "length": np.full(rows, width, dtype=np.uint32)}


@pytest.mark.parametrize("form", FORMS)
def test_best_corners_and_ties(dev, cols, form):
    """the winning pair at each corner of the band -- (i, i) and (i, i + max_len - 1), its start in the step before its end's,
    astride lane and quad seams -- and exact ties placed in different lanes and steps: the smaller i, then the smaller j wins"""
    width = 2 * cols + 9
    for max_len in (1, 2, 5, 70, width, width + 7):
        reach = min(max_len, width) - 1
        ends = sorted({j for j in (0, 3, 4, 5, 255, cols - 1, cols, cols + 1, cols + 3, 2 * cols, 2 * cols + 2, width - 1) if j < width})
        wins = [(j - k, j) for j in ends for k in sorted({0, min(reach, j)})]  # both corners of the band behind j
        b = full_rows(len(wins) + 4, width)
        sl, el = np.zeros((len(wins) + 4, width), dtype=np.float32), np.zeros((len(wins) + 4, width), dtype=np.float32)
        for r, (i, j) in enumerate(wins):
            sl[r, i], el[r, j] = 4, 4
            if i > 0:
                el[r, i - 1] = 4  # ends before it starts: no span
            if j - i == reach and j + 1 < width:
                el[r, j + 1] = 4  # one column too long
        r = len(wins)
        # ties: the same score from pairs in different lanes and steps
        sl[r, [cols + 2, 7]], el[r, [cols + 2, 7]] = 3, 3
        sl[r + 1, [2 * cols + 1, cols - 1]], el[r + 1, [2 * cols + 1, cols - 1]] = 3, 3
        sl[r + 2, 5], el[r + 2, [5 + min(reach, 1), 5]] = 3, 3      # the same i: the smaller j
        sl[r + 3, :], el[r + 3, :] = 1, 1                            # every candidate ties: (0, 0)
        want = run_best(dev, form, b, sl, el, len(wins) + 4, max_len, what=("corners", max_len))
        got = list(zip(want["row_start"].tolist(), want["row_end"].tolist()))
        assert got[:r] == wins and got[r:] == [(7, 7), (cols - 1, cols - 1), (5, 5), (0, 0)], max_len
        assert want["row_score"][:r].tolist() == [8.0] * r


@pytest.mark.parametrize("form", FORMS)
def test_best_texts(dev, form):
    """texts of 1, 2, 3, 64, 65 and 130 rows, a text with no row among them, and text boundaries at the wavefront and workgroup
    seams of the reduction; ties between the rows of a text go to the lower row; NaN and missing [CLS] scores"""
    scan_rows = dev.label_capacity()[1]
    counts = [1, 2, 3, 0, 64, 65, 130]
    sample = np.repeat(np.arange(len(counts)), counts)
    edges = sorted({63, 64, 65, scan_rows - 1, scan_rows, scan_rows + 1, 2 * scan_rows, 2 * scan_rows + 1})
    rows = 2 * scan_rows + 3
    more = np.searchsorted(np.array(edges), np.arange(rows), side="right") + len(counts) + 1  # a text boundary at every edge
    for name, s in (("sizes", sample), ("edges", more)):
        s = s.astype(np.uint32)
        n_samples = int(s.max()) + 2
        for width in (6, 8):
            b = L.make_rows(s.size, width, seed=width, texts=s, fill=width)
            sl, el = L.small_logits((s.size, width), 1, -2, 3), L.small_logits((s.size, width), 2, -2, 3)  # few values: many ties
            sl[::7, 0], el[5::11, 0] = np.nan, np.nan
            sl[3, :] = np.nan  # a row without a candidate
            want = run_best(dev, form, b, sl, el, n_samples, 3, cls=True, what=(name, width))
            assert want["info"][1] == len(np.unique(s)) and want["row"][3 if name == "sizes" else 0] == -1
            assert (want["row"][want["row"] >= 0] < s.size).all()


def test_best_pointers_off_16_bytes(dev, cols):
    for width in (8, cols + 4):
        b = L.make_rows(6, width, seed=width, pair=True)
        sl, el = L.small_logits((6, width), 3), L.small_logits((6, width), 4)
        run_best(dev, "dev", b, sl, el, b["n_samples"], 6, 1, True, shift=1, what=("shifted", width))


def test_dev_forms_refuse_and_take_no_row(dev):
    import torch
    d = torch.zeros(256, dtype=torch.int32, device="cuda")
    p, lib = d.data_ptr(), dev.lib()
    info = torch.full((4,), 7, dtype=torch.int64, device="cuda")
    hit = torch.full((8,), 7, dtype=torch.uint8, device="cuda")
    text = [torch.full((2,), 7, dtype=torch.int32, device="cuda") for _ in range(7)]
    tp = [t.data_ptr() for t in text]
    label = lambda **kw: lib.swt_label_words_dev(kw.get("word", p), None, 0, None, kw.get("rows", 2), 4, p + 64, p + 128, 4, 1, None, 0, -100, 0,
                                                 kw.get("out", p + 256), None, kw.get("info"), None)
    assert label(out=p + 16) == dev.ERR_INVALID and "out_labels" in lib.swt_last_error().decode()
    assert label(word=p + 2) == dev.ERR_INVALID and "word" in lib.swt_last_error().decode()
    assert label() == 0
    assert label(rows=0, info=info.data_ptr()) == 0
    torch.cuda.synchronize()
    assert info.tolist() == [0] * 4
    info.fill_(7)
    assert lib.swt_answer_positions_dev(p, p + 512, None, 0, None, 0, 4, p + 64, 2, None, -100, 0, p + 256, p + 320, None, hit.data_ptr(),
                                        info.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert info.tolist() == [0, 0, 0, 7] and hit.tolist() == [0, 0] + [7] * 6
    info.fill_(7)
    assert lib.swt_answer_positions_dev(p, p + 512, None, 0, None, 2, 4, p + 64, 2, None, -100, 0, p + 32, p + 320, None, None, None,
                                        None) == dev.ERR_INVALID and "out_start" in lib.swt_last_error().decode()
    assert lib.swt_answer_best_dev(p, p + 64, p + 128, p + 512, None, 0, None, 0, 4, 2, 3, None, 0, *tp, None, None, None, info.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert info.tolist() == [0, 0, 7, 7]
    assert [t.tolist() for t in text[2:]] == [[-1, -1]] * 3 + [[0, 0]] * 2
    assert text[0].view(torch.float32).tolist() == [-np.inf] * 2 and text[1].view(torch.float32).tolist() == [np.inf] * 2


# ---- through the classes

SENTENCES = ["The quick brown fox jumps over the lazy dog near the river bank.", "Pan Tadeusz czyli ostatni zajazd na Litwie.",
             "Tokenizers split words into smaller pieces, called subwords!", "A short one.", "",
             "Unbelievably, long words count; abbreviations help.",
             "İstanbul is a city that straddles two continents.", "Numbers like 12345 and 67890 are split too.",
             "She said: (well) maybe - or maybe not.", "The answer to the question lies somewhere in the middle of this long context sentence.",
             "Windows overlap by a stride so that no answer is lost at an edge.", "Last sentence of the dozen."]
QUESTIONS = ["who?", "what?", "which?", "how?", "why?", "what?", "where?", "which?", "what?", "where?", "why?", "who?"]
ANSWERS = ["brown", "czyli", "split words", None, None, "long", "is", None, "well", "answer to", "overlap", None]


def _tokenizer(swt, ref_dir, cls):
    tok = getattr(swt, cls)()
    tok.load_resources(os.path.join(ref_dir, "resources/tests", "FastBPE" if "BPE" in cls else "FastWordPiece"))
    return tok


def _np(res):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in res.items()}


def _same(a, b):
    a, b = _np(a), _np(b)
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


@pytest.mark.parametrize("cls", ["FastBPE", "NaiveWP"])  # FastWP refuses texts on which this small vocabulary does not terminate
def test_align_word_labels_end_to_end(swt, dev, ref_dir, cls):
    tok = _tokenizer(swt, ref_dir, cls)
    labels = [[(3 * i + k) % 5 for k in range(len(s) + 1)] for i, s in enumerate(SENTENCES)]  # a label for every word at the least
    inside = [0, 2, 2, 4, 4]
    results = []
    for device in (False, True):
        batch = tok.encode_batch(SENTENCES, max_length=12, stride=3, return_overflowing=True, return_offsets=True, device=device,
                                 padding="max_length", int64=device)
        h = _np(batch)
        for all_tokens, ins in ((False, None), (True, inside)):
            got = tok.align_word_labels(batch, labels, label_all_tokens=all_tokens, inside=ins)
            assert ("torch" in str(type(got["labels"]))) == device
            lab_off = np.concatenate([[0], np.cumsum([len(x) for x in labels])])
            want = L.expected_labels(h["word_ids"], lab_off, np.concatenate(labels), None, 0, h["overflow_to_sample_mapping"], ins, all_tokens,
                                     dtype=h["input_ids"].dtype)
            assert np.array_equal(_np(got)["labels"], want["labels"]) and got["labels"].dtype == batch["input_ids"].dtype
            assert (got["n_labelled"], got["n_continuation"]) == (int(want["info"][0]), int(want["info"][1])) and got["n_labelled"] > 12
            results.append(_np(got)["labels"].astype(np.int64))
        short = [[] if i == 2 else x for i, x in enumerate(labels)]
        with pytest.raises(ValueError, match="text 2"):
            tok.align_word_labels(batch, short)
        with pytest.raises(ValueError, match="beyond the 11"):
            tok.align_word_labels(batch, labels[:11])
    assert np.array_equal(results[0], results[2]) and np.array_equal(results[1], results[3])
    assert cls != "FastBPE" or h["input_ids"].shape[0] > len(SENTENCES)  # there were windows


@pytest.mark.parametrize("cls", ["FastBPE", "NaiveWP"])  # FastWP refuses texts on which this small vocabulary does not terminate
@pytest.mark.parametrize("padding_side", ["right", "left"])
def test_answers_end_to_end(swt, dev, ref_dir, cls, padding_side):
    """answer_positions and best_answers over question / context pairs in windows of 40 columns that overlap by 12: an answer
    of 13 tokens or fewer lies whole in some window, whatever the vocabulary makes of its letters"""
    tok = _tokenizer(swt, ref_dir, cls)
    answers = [None if w is None else (s.index(w), s.index(w) + len(w)) for s, w in zip(SENTENCES, ANSWERS)]
    kept = {}
    for device in (False, True):
        batch = tok.encode_batch(QUESTIONS, text_pairs=SENTENCES, max_length=40, stride=12, truncation="only_second", return_overflowing=True,
                                 return_offsets=True, device=device, padding="max_length", padding_side=padding_side)
        h = _np(batch)
        rows, width = h["input_ids"].shape
        got = tok.answer_positions(batch, answers, texts=SENTENCES)
        mapped = L.NONE * np.ones((len(SENTENCES), 2), dtype=np.int64)
        for i, (a, s) in enumerate(zip(answers, SENTENCES)):
            if a is not None:
                mapped[i] = [len(s[:a[0]].lower()), len(s[:a[1]].lower())]
        want = L.expected_positions(h["offset_mapping"], mapped, h["word_ids"], h["sequence_ids"], 1, h["overflow_to_sample_mapping"],
                                    h["length"], True, padding_side == "left", dtype=h["input_ids"].dtype)
        g = _np(got)
        for k, w in (("start_positions", "start"), ("end_positions", "end"), ("has_answer", "has"), ("sample_has_answer_row", "hit")):
            assert np.array_equal(g[k], want[w]), k
        assert (got["n_with"], got["n_without"]) == (int(want["info"][0]), int(want["info"][1])) and got["n_with"] >= 8
        assert g["sample_has_answer_row"].tolist() == [int(a is not None) for a in answers]
        cls_col = np.where(padding_side == "left", width - h["length"].astype(np.int64), 0)
        assert np.array_equal(g["start_positions"][g["has_answer"] == 0], cls_col[g["has_answer"] == 0])
        # logits that peak on the labelled positions give the answers back
        sl = L.small_logits((rows, width), 5, -3, 1)
        el = L.small_logits((rows, width), 6, -3, 1)
        on = np.flatnonzero(g["has_answer"])
        sl[on, g["start_positions"][on]], el[on, g["end_positions"][on]] = 6, 6
        if device:
            import torch
            d_sl, d_el = torch.from_numpy(sl).cuda(), torch.from_numpy(el).cuda()
        else:
            d_sl, d_el = sl, el
        best = tok.best_answers(batch, d_sl, d_el, max_answer_length=16, texts=SENTENCES)
        want = L.expected_best(sl, el, h["offset_mapping"], len(SENTENCES), h["word_ids"], h["sequence_ids"], 1, h["overflow_to_sample_mapping"],
                               16, h["length"], True, padding_side == "left")
        gb = _np({k: v for k, v in best.items() if k != "text"})
        for k in TEXT:
            assert np.array_equal(gb[k], want[k]), k
        for i, a in enumerate(answers):
            if a is not None:
                assert best["text"][i] == SENTENCES[i][a[0]:a[1]].lower() and gb["score"][i] == 12.0, i
        with pytest.raises(TypeError):
            tok.best_answers(batch, d_sl.astype(np.float64) if not device else d_sl.double(), d_el)
        kept[device] = (g, gb, best["text"])
    _same(kept[False][0], kept[True][0])
    _same(kept[False][1], kept[True][1])
    assert kept[False][2] == kept[True][2]
    assert json.dumps(kept[False][2])  # plain strings
