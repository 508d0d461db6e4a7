"""swt_word_plan, swt_word_predict and swt_entity_spans on the GPU, host and `_dev` forms, against the NumPy model
(tests/tag_cases.py): element by element and `info` included, the score of swt_word_predict alone within score_rtol(n_labels) of
the float64 model.  The shapes are the smallest that reach each seam of the kernels, the seams placed from swt_tag_capacity: the
scalar and the wide path, one, two and three steps a row, rows that share a wavefront, runs across every quad, lane and step seam,
words whose rows lie in different workgroups, entities across the workgroups and the groups of the scan.  Every `_dev` output lies
behind fence bytes before and after it, and an output that is not given stays unwritten."""
import os

import numpy as np
import pytest

from tests import tag_cases as T

pytestmark = pytest.mark.gpu

FENCE, GARBAGE, FRONT, BACK = 0xEE, 0x5A, 64, 64
FORMS = ["host", "dev"]
LABEL_COUNTS = (1, 2, 3, 4, 5, 9, 33)  # a row stride that is and is not a multiple of 16 bytes
WORD_OUT = ("label", "score", "row", "col", "n_tokens", "char_start", "char_end")
ENTITY_OUT = ("text_index", "type", "first_word", "last_word", "char_start", "char_end", "score")
WORST = {}  # n_labels -> the largest relative error of a finite score seen, in units of 2^-24


@pytest.fixture(scope="module")
def dev(native):
    if native.device_count() < 1:
        pytest.fail("no HIP device")
    native.init(0)
    return native


@pytest.fixture(scope="module")
def capacity(dev):
    return dev.tag_capacity()


def widths(cols):
    return (1, 3, 4, 5, 63, 64, 65, cols - 1, cols, cols + 1, 2 * cols + 1)


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


def agree(got, want, what, score_labels=None):
    """element by element; with score_labels (the n_labels of swt_word_predict) the score within score_rtol where it is finite"""
    for k, g in got.items():
        if g is None:
            continue
        w = want[k]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        if k == "score" and score_labels:
            finite = np.isfinite(w)
            assert np.array_equal(np.isfinite(g), finite) and np.array_equal(g[~finite], w[~finite], equal_nan=True), (what, k)
            err = np.abs(g[finite].astype(np.float64) - w[finite]) / np.abs(w[finite].astype(np.float64)).clip(1e-300)
            if err.size:
                WORST[score_labels] = max(WORST.get(score_labels, 0.0), float(err.max()) * 2.0 ** 24)
                print("score: n_labels %d, largest relative error %.3f x 2^-24 (allowed %d)" % (score_labels, err.max() * 2.0 ** 24,
                                                                                               4 * (score_labels + 1)))
                assert err.max() <= T.score_rtol(score_labels), (what, k, float(err.max()), T.score_rtol(score_labels))
            continue
        if not np.array_equal(g, w, equal_nan=g.dtype.kind == "f"):
            bad = np.argwhere(~((g == w) | ((g != g) & (w != w))))
            raise AssertionError("%s: %s differs at %d places, first %s: got %s, want %s"
                                 % (what, k, len(bad), bad[0].tolist(), g[tuple(bad[0])], w[tuple(bad[0])]))


def run_plan(dev, form, b, side=0, n_samples=None, shift=0, what=""):
    n = b["n_samples"] if n_samples is None else n_samples
    want = T.expected_plan(b["word"], n, b["seq"], side, b["sample"])
    rows, width = b["word"].shape
    if form == "host":
        off, info = dev.word_plan(b["word"], n, b["seq"], side, b["sample"])
        got = {"word_off": off, "info": info}
    else:
        d = Device(shift)
        dev.check(dev.lib().swt_word_plan_dev(d.up(b["word"]), d.up(b["seq"]), side, d.up(b["sample"]), rows, width, n,
                                              d.out("word_off", (n + 1,), np.uint64), d.out("info", (2,), np.uint64), None))
        got = d.collect()
    agree(got, want, ("plan", what, form))
    return want["word_off"]


def run_predict(dev, form, b, x, off, strategy, side=0, n_words=None, given=None, shift=0, what=""):
    want = T.expected_predict(x, b["word"], b["spans"], off, b["seq"], side, b["sample"], strategy, n_words)
    rows, width, n_labels = x.shape
    n_words = want["label"].size
    types = dict(dev.WORD_OUT)
    if form == "host":
        got = dev.word_predict(x, b["word"], b["spans"], off, b["seq"], side, b["sample"], strategy, n_words, word_logits=True)
    else:
        d = Device(shift)
        on = lambda name: given is None or name in given
        args = [d.up(x), d.up(b["word"]), d.up(b["seq"]), side, d.up(b["sample"]), d.up(b["spans"]), rows, width, n_labels,
                d.up(np.asarray(off, dtype=np.uint64)), len(off) - 1, n_words, strategy]
        args += [d.out(name, (n_words,), types[name], on(name)) for name in WORD_OUT]
        args += [d.out("logits", (n_words, n_labels), np.float32, on("logits")), d.out("info", (4,), np.uint64, on("info")), None]
        dev.check(dev.lib().swt_word_predict_dev(*args))
        got = d.collect()
    agree(got, want, ("predict", what, form, strategy, n_labels), n_labels)
    return want


def run_entities(dev, form, label, score, cs, ce, off, etype, begins, info=True, shift=0, what=""):
    want = T.expected_entities(label, score, cs, ce, off, etype, begins)
    n = len(label)
    if form == "host":
        got = dev.entity_spans(label, score, cs, ce, off, etype, begins, info=info)
    else:
        d = Device(shift)
        types = dict(dev.ENTITY_OUT)
        args = [d.up(np.asarray(label, np.int32)), d.up(np.asarray(score, np.float32)), d.up(np.asarray(cs, np.uint32)),
                d.up(np.asarray(ce, np.uint32)), d.up(np.asarray(off, np.uint64)), len(off) - 1, n, d.up(np.asarray(etype, np.int32)),
                d.up(np.asarray(begins, np.uint8)), len(etype)]
        args += [d.out(name, (n,), types[name]) for name in ENTITY_OUT] + [d.out("info", (2,), np.uint64, info), None]
        dev.check(dev.lib().swt_entity_spans_dev(*args))
        got = d.collect()
    agree(got, want, ("entities", what, form))
    return want


def logits_for(shape, seed, exact):
    """small integers (every sum exact, ties real), or normal values of scale 4"""
    if exact:
        return T.small_logits(shape, seed)
    return (4 * np.random.default_rng(seed).standard_normal(shape)).astype(np.float32)


def rows_case(rows, width, seed, pair, **kw):
    b = T.make_rows(rows, width, seed=seed, pair=pair, **kw)
    if rows > 2:
        b["sample"][-1] = b["n_samples"] + 5  # a row of no text; the samples still do not decrease
    return b


# ---- shapes

@pytest.mark.parametrize("form", FORMS)
def test_widths_and_label_counts(dev, capacity, form):
    """the scalar and the wide path; one, two and three steps a row; 11 rows, so that groups of every size leave a wavefront partly
    dead; single rows and both sides of pair rows, padded right and left; every n_labels; pointers off 16-byte alignment"""
    seen = 0
    for n, width in enumerate(widths(capacity[0])):
        pair, n_labels = width >= 5 and n % 2 == 1, LABEL_COUNTS[n % len(LABEL_COUNTS)]
        b = rows_case(11, width, width, pair, pad_left=n % 3 == 0, fill=None if width < 64 else width - n % 3)
        for side in ((0, 1) if pair else (0,)):
            off = run_plan(dev, form, b, side, shift=n % 4, what=("width", width))
            x = logits_for((11, width, n_labels), width, n % 2 == 0)
            for strategy in (T.FIRST, T.MEAN, T.MAX):
                want = run_predict(dev, form, b, x, off, strategy, side, shift=n % 4, what=("width", width))
            seen += int(want["info"][2])
            assert width < 64 or (want["info"][0] > 0 and want["info"][3] > 0)
    assert seen > 0  # runs lost to another row's


@pytest.mark.parametrize("form", FORMS)
def test_row_counts(dev, form):
    """several narrow rows share a wavefront (widths 3 and 4: one lane a row, 5 and 8: two): 1, 2, 65 and 257 rows"""
    for width in (3, 4, 5, 8):
        for rows in (1, 2, 65, 257):
            b = rows_case(rows, width, rows + width, False, specials=False)
            off = run_plan(dev, form, b, what=("rows", rows, width))
            x = logits_for((rows, width, 3 if width % 2 else 4), rows, rows % 2 == 0)
            run_predict(dev, form, b, x, off, (rows + width) % 3, what=("rows", rows, width))


@pytest.mark.parametrize("form", FORMS)
def test_runs_across_the_seams(dev, capacity, form):
    """runs of 1, 2, 5 and 9 columns starting and ending at every column of a row of three steps, so across every quad, lane and
    step seam; one run that fills a row"""
    width = 2 * capacity[0] + 7
    b = T.rows_of_runs((1, 2, 5, 9), width)
    x = logits_for((b["word"].shape[0], width, 3), 11, False)
    off = run_plan(dev, form, b, what="runs")
    for strategy in (T.FIRST, T.MEAN, T.MAX):
        want = run_predict(dev, form, b, x, off, strategy, what="runs")
    assert sorted(set(want["n_tokens"].tolist())) == [1, 2, 3, 4, 5, 6, 7, 8, 9] and want["info"][1] == 0
    whole = dict(b, word=np.zeros((1, width), dtype=np.int32), spans=b["spans"][:1], sample=np.zeros(1, np.uint32), n_samples=1)
    for strategy in (T.MEAN, T.MAX):
        want = run_predict(dev, form, whole, x[:1], [0, 1], strategy, what="one run")
    assert want["n_tokens"].tolist() == [width]


@pytest.mark.parametrize("form", FORMS)
def test_words_in_several_rows(dev, capacity, form):
    """words in two and in three rows of a text at a width of one row a wavefront: contexts unequal; equal (columns p and W - s - n
    - p of neighbouring windows, and the two halves of a cut word at stride 0), with the rows in one workgroup and in two; three
    rows that tie"""
    W = capacity[0]
    per_group = 4  # rows of a workgroup at this width
    parts, sample = [], []
    for text, (n_tokens, stride) in enumerate(((500, 100), (500, 100), (300, 0), (330, 200))):
        word, spans = T.windows(n_tokens, W, stride, (np.arange(n_tokens) + 1) // 2)
        parts.append((word, spans))
        sample += [text] * word.shape[0]
    tie = np.full((3, W), -1, dtype=np.int32)
    tie[:, :3] = (5, 5, 6)
    parts.append((tie, np.ones((3, W, 2), dtype=np.uint32) * np.arange(3, dtype=np.uint32)[:, None, None]))
    sample += [4] * 3
    b = {"word": np.concatenate([p[0] for p in parts]), "spans": np.concatenate([p[1] for p in parts]), "seq": None,
         "sample": np.array(sample, dtype=np.uint32), "n_samples": 5}
    rows = b["word"].shape[0]
    assert sample == [0] * 3 + [1] * 3 + [2] * 2 + [3] * 3 + [4] * 3 and 3 // per_group != 4 // per_group and 11 // per_group != 12 // per_group
    p = (2 * W - 100 - 2) // 2  # the word of two tokens at column p of a window has the context W - p - 2 there and in the next
    assert p % 2 == 1 and min(p, W - p - 2) == min(p - (W - 100), 2 * W - 100 - p - 2)
    off = run_plan(dev, form, b, what="several rows")
    x = logits_for((rows, W, 4), 5, True)
    for strategy in (T.FIRST, T.MEAN):
        want = run_predict(dev, form, b, x, off, strategy, what="several rows")
    at = int(off[1]) + (p + 1) // 2
    assert (want["row"][at], want["col"][at]) == (3, p)  # equal contexts, rows 3 and 4 in two workgroups: the earlier row
    at = int(off[1]) + (W - 100 + p + 1) // 2
    assert (want["row"][at], want["col"][at]) == (4, p)  # rows 4 and 5 in one workgroup
    at = int(off[2]) + W // 2
    assert (want["row"][at], want["col"][at], want["n_tokens"][at]) == (6, W - 1, 1)  # the halves tie at context 0
    assert want["row"][int(off[4]) + 5] == 11 and want["row"][int(off[4]) + 6] == 11 and want["info"][1] == 5  # words 0 .. 4 of text 4
    in_three = int(off[3]) + 100
    assert want["row"][in_three] == 9 and want["info"][2] > 100


@pytest.mark.parametrize("form", FORMS)
def test_missing_words_and_foreign_offsets(dev, form):
    """texts with no row, word ids no row names, a row of no text; offsets with a word more and a word fewer per text than the rows
    name, and more words than the offsets end at"""
    b = T.make_rows(9, 21, seed=4, texts=[0, 0, 2, 2, 2, 3, 5, 5, 9])
    b["n_samples"] = 7
    off = run_plan(dev, form, b, what="missing").astype(np.int64)
    assert off[2] == off[1] and off[5] == off[4] and off[7] == off[6]
    x = logits_for((9, 21, 5), 1, False)
    want = run_predict(dev, form, b, x, off, T.MEAN, what="missing")
    assert want["info"][1] > 0 and want["info"][3] > 0
    more = off + np.arange(8)
    want = run_predict(dev, form, b, x, more, T.FIRST, n_words=int(more[-1]) + 3, what="a word more")
    assert want["info"][1] >= 10
    fewer = np.concatenate([[0], np.cumsum(np.maximum(np.diff(off) - 1, 0))])
    base = run_predict(dev, form, b, x, off, T.MAX, what="missing")
    want = run_predict(dev, form, b, x, fewer, T.MAX, what="a word fewer")
    assert want["info"][3] > base["info"][3]
    if form == "dev":  # the host form refuses offsets that end beyond the words
        run_predict(dev, form, b, x, off, T.FIRST, n_words=int(off[-1]) - 2, what="fewer words than the offsets")
    # no text at all; no row at all
    run_plan(dev, form, b, n_samples=0, what="no text")
    want = run_predict(dev, form, b, x, [0], T.FIRST, n_words=2, what="no text")
    assert want["info"].tolist() == [0, 2, 0, want["info"][3]] and want["info"][3] > 9
    none = dict(b, word=b["word"][:0], spans=b["spans"][:0], sample=b["sample"][:0])
    run_plan(dev, form, none, what="no row")
    run_predict(dev, form, none, x[:0], off, T.FIRST, what="no row")


@pytest.mark.parametrize("strategy", [T.FIRST, T.MEAN, T.MAX])
@pytest.mark.parametrize("form", FORMS)
def test_argmax_ties_and_special_values(dev, form, strategy):
    """ties from small integers at label 0, at the last label and between; one NaN entry, words that are all NaN, +inf and -inf
    entries, a NaN in one column of a run: the label stands and the score is what IEEE makes of it"""
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    width = 48
    for n_labels in LABEL_COUNTS:
        per = 1 if strategy == T.FIRST else 2
        b = T.rows_of_runs((per,), width)
        b = {k: (v[:1] if isinstance(v, np.ndarray) else v) for k, v in b.items()}
        b["n_samples"] = 1
        x = T.small_logits((1, width, n_labels), n_labels, -1, 2)
        last = n_labels - 1
        x[0, 0:2], x[0, 2:4] = 5, 0
        x[0, 2:4, last] = 3
        x[0, 4:6], x[0, 6:8, 0] = nan, nan
        x[0, 8:10, last], x[0, 10:12, 0], x[0, 12:14] = inf, -inf, -inf
        x[0, 14, last // 2], x[0, 16] = nan, nan  # one column of a run of two
        x[0, 18, 0], x[0, 19, 0], x[0, 20, last], x[0, 21, last] = inf, -inf, -inf, inf
        want = run_predict(dev, form, b, x, [0, width // per], strategy, what=("special", n_labels))
        lab = want["label"]
        assert lab[0] == 0 and lab[2 // per] == last and lab[4 // per] == -1 and lab[8 // per] == last and lab[12 // per] == 0
        assert np.isnan(want["score"][4 // per]) and np.isnan(want["score"][8 // per]) and np.isnan(want["score"][12 // per])
        assert want["score"][0] == np.float32(1 / n_labels) or n_labels in (3, 5, 9, 33)


def test_outputs_not_given_stay_unwritten(dev):
    b = rows_case(7, 37, 2, True)
    off = run_plan(dev, "dev", b, 1)
    x = logits_for((7, 37, 9), 2, False)
    for given in ((), ("label",), ("score", "info"), ("logits", "char_end"), ("row", "col", "n_tokens", "char_start")):
        run_predict(dev, "dev", b, x, off, T.MEAN, 1, given=given, shift=1, what=("given", given))
    n = 300
    etype, begins = T.scheme(5)
    rng = np.random.default_rng(0)
    run_entities(dev, "dev", rng.integers(0, 5, n), rng.random(n, dtype=np.float32), np.arange(n), np.arange(n) + 1, [0, 100, n], etype, begins,
                 info=False, shift=3)


# ---- entities

@pytest.mark.parametrize("form", FORMS)
def test_entities_across_the_seams(dev, capacity, form):
    """heads and ends of entities and the boundaries of texts at the seams of the workgroups and of the scan's groups; an entity
    that spans a whole group's words; no entity; every word an entity"""
    _, group, scan = capacity
    n = 2 * scan + 3
    etype, begins = T.scheme(5)  # O, B-0, I-0, B-1, I-1
    rng = np.random.default_rng(7)
    score = rng.random(n, dtype=np.float32)
    cs, ce = (3 * np.arange(n)).astype(np.uint32), (3 * np.arange(n) + 2).astype(np.uint32)
    seams = sorted({k * group + d for k in range(1, n // group + 1) for d in (-1, 0, 1)} | {scan - 1, scan, scan + 1, 2 * scan, n - 1})
    one = [0, n]
    # random labels, labels outside the scheme among them; texts that begin at every seam, some of them empty
    label = rng.integers(-1, 7, n)
    want = run_entities(dev, form, label, score, cs, ce, [0, 0] + seams + [n, n], etype, begins, shift=1, what="random")
    assert 0 < want["info"][0] < want["info"][1] < n
    # one text, all I-0: one entity over every group; B-0 at the seams: heads there; texts at the seams: heads there as well
    label = np.full(n, 2)
    want = run_entities(dev, form, label, score, cs, ce, one, etype, begins, what="one entity")
    assert want["info"].tolist() == [1, n] and want["last_word"][0] == n - 1
    label[seams] = 1
    want = run_entities(dev, form, label, score, cs, ce, one, etype, begins, what="heads at the seams")
    assert want["info"].tolist() == [len(seams) + 1, n]
    want = run_entities(dev, form, np.full(n, 2), score, cs, ce, [0] + seams + [n], etype, begins, what="texts at the seams")
    assert want["info"].tolist() == [len(seams) + 1, n] and want["first_word"][:5].tolist() == [0] * 5
    # entities that end at the seams: an O behind them
    label = np.full(n, 2)
    label[seams] = 0
    run_entities(dev, form, label, score, cs, ce, [0, scan, n], etype, begins, what="ends at the seams")
    want = run_entities(dev, form, np.zeros(n, np.int64), score, cs, ce, one, etype, begins, what="no entity")
    assert want["info"].tolist() == [0, 0] and (want["type"] == -1).all()
    want = run_entities(dev, form, np.full(n, 1), score, cs, ce, one, etype, begins, what="all heads")
    assert want["info"].tolist() == [n, n]
    want = run_entities(dev, form, np.full(n, 4), score, cs, ce, [0, 5], etype, begins, what="words of no text")
    assert want["info"].tolist() == [1, 5]


# ---- through the classes

SENTENCES = ["Yesterday evening Anna Maria Kowalska travelled from Warsaw to New York City with her two old friends and a dog",
             "The quick brown fox visited Pan Tadeusz near the river bank while the lazy dog slept under a tree",
             "Short text about Adam here",
             "Nobody is named in this sentence at all so it has no entity whatever the model says about it"]
ID2LABEL = ["O", "B-PER", "I-PER", "B-LOC", "I-LOC"]
MARKED = [{2: 1, 3: 2, 4: 2, 7: 3, 9: 3, 10: 4, 11: 4}, {5: 1, 6: 2}, {3: 1}, {}]  # word -> label; every other word is "O"
ENTITIES = [(0, "PER", "anna maria kowalska"), (0, "LOC", "warsaw"), (0, "LOC", "new york city"), (1, "PER", "pan tadeusz"), (2, "PER", "adam")]


def _np(res):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in res.items()}


def _like(got, want, names):
    """the arrays `names` of got, a torch path's int32 read as the uint32 it holds"""
    return {k: got[k].view(want[k].dtype) if got[k].dtype != want[k].dtype and got[k].dtype.kind in "iu" else got[k] for k in names}


@pytest.mark.parametrize("cls", ["FastBPE", "NaiveWP"])  # FastWP refuses texts on which this small vocabulary does not terminate
@pytest.mark.parametrize("strategy", ["first", "mean", "max"])
def test_words_and_entities_end_to_end(swt, dev, ref_dir, cls, strategy):
    """windows of 22 tokens that overlap by 10: a word of ten tokens or fewer lies whole, with a token on either side, in some
    window.  Logits that peak on every token's word's label give the labels back per word, and the entities as strings"""
    tok = getattr(swt, cls)()
    tok.load_resources(os.path.join(ref_dir, "resources/tests", "FastBPE" if "BPE" in cls else "FastWordPiece"))
    labels = [[marked.get(k, 0) for k in range(len(s.split()))] for s, marked in zip(SENTENCES, MARKED)]
    kept = {}
    for device in (False, True):
        batch = tok.encode_batch(SENTENCES, max_length=24, stride=10, return_overflowing=True, return_offsets=True, device=device,
                                 padding="max_length")
        h = _np(batch)
        rows, width = h["input_ids"].shape
        assert rows > len(SENTENCES) or cls != "FastBPE"  # there were windows
        x = T.small_logits((rows, width, len(ID2LABEL)), 3, -3, 1)
        for r in range(rows):
            for c in np.flatnonzero(h["word_ids"][r] >= 0):
                x[r, c, labels[h["overflow_to_sample_mapping"][r]][h["word_ids"][r, c]]] = 6
        if device:
            import torch
            logits = torch.from_numpy(x).cuda()
        else:
            logits = x
        words = tok.word_predictions(batch, logits, strategy=strategy, return_logits=True)
        assert ("torch" in str(type(words["label"]))) == device
        w = _np(words)
        assert w["word_offsets"].tolist() == np.concatenate([[0], np.cumsum([len(x) for x in labels])]).tolist()
        assert w["label"].tolist() == [l for text in labels for l in text] and (w["n_words"], w["n_missing"]) == (len(w["label"]), 0)
        assert ((w["score"] > 0.5) & (w["score"] <= 1)).all()
        off = T.expected_plan(h["word_ids"], len(SENTENCES), sample=h["overflow_to_sample_mapping"])["word_off"]
        want = T.expected_predict(x, h["word_ids"], h["offset_mapping"], off, sample=h["overflow_to_sample_mapping"], strategy=T.STRATEGIES[strategy])
        agree(_like(w, want, WORD_OUT + ("logits",)), want, ("end to end", cls, strategy, device), len(ID2LABEL))
        ents = tok.entities(words, ID2LABEL, texts=SENTENCES)
        e = _np({k: v for k, v in ents.items() if k not in ("text", "type_names")})
        assert ents["type_names"] == ["PER", "LOC"] and ents["n_entities"] == len(ENTITIES) and ents["n_entity_words"] == 10
        assert [(int(t), ents["type_names"][int(k)], s) for t, k, s in zip(e["text_index"], e["type"], ents["text"])] == ENTITIES
        etype, begins = np.array([-1, 0, 0, 1, 1]), np.array([0, 1, 0, 1, 0])
        model = T.expected_entities(w["label"], w["score"], w["char_start"], w["char_end"], w["word_offsets"], etype, begins)
        agree(_like(e, model, ENTITY_OUT), {k: model[k][:len(ENTITIES)] for k in ENTITY_OUT}, ("entities end to end", cls, strategy, device))
        # the way back: the predicted labels, aligned onto the rows again, are the labels the logits were built from
        again = tok.align_word_labels(batch, (w["label"], w["word_offsets"]))
        first = tok.align_word_labels(batch, labels)
        assert np.array_equal(_np(again)["labels"], _np(first)["labels"]) and again["n_labelled"] == first["n_labelled"] > len(w["label"]) - 1
        kept[device] = (w, e, ents["text"])
    for a, b in zip(kept[False][:2], kept[True][:2]):
        assert a.keys() == b.keys()
        for k in a:
            x, y = np.asarray(a[k]), np.asarray(b[k])
            assert np.array_equal(x, y.view(x.dtype) if x.dtype != y.dtype else y, equal_nan=x.dtype.kind == "f"), k
    assert kept[False][2] == kept[True][2]
    with pytest.raises(TypeError):
        tok.word_predictions(batch, x)  # a batch on the GPU and logits on the host
