"""The NumPy model of token-classification inference (tests/tag_cases.py) against a restatement of include/swt.h in plain Python
loops and against cases worked out by hand; what the built library exports; what the host forms refuse before a device is
touched.  No GPU."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import tag_cases as T

NONE = 0xFFFFFFFF


# ---- the rules again, in loops

def loop_runs(word, seq, side, r):
    """the runs of row r: [(first column, columns, word id, context)]"""
    width = len(word[r])
    tok = [(int(seq[r][c]) == side) if seq is not None else (int(word[r][c]) & NONE) != NONE for c in range(width)]
    out, c = [], 0
    while c < width:
        if not tok[c]:
            c += 1
            continue
        k, e = int(word[r][c]) & NONE, c + 1
        while e < width and tok[e] and (int(word[r][e]) & NONE) == k:
            e += 1
        out.append((c, e - c, k, min(sum(tok[:c]), sum(tok[e:]))))
        c = e
    return out


def loop_predict(x, word, spans, off, seq=None, side=0, sample=None, strategy=T.FIRST, n_words=None):
    rows, width, L = x.shape
    n_words = int(off[-1]) if n_words is None else n_words
    n_samples = len(off) - 1
    best, skipped, taking = {}, 0, []
    for r in range(rows):
        s = r if sample is None else int(sample[r])
        for c, n, k, context in loop_runs(word, seq, side, r):
            if s >= n_samples or k >= int(off[s + 1]) - int(off[s]) or int(off[s]) + k >= n_words:
                skipped += 1
                continue
            at, rank = int(off[s]) + k, (context, -r, -c)
            taking.append((at, r))
            if at not in best or rank > best[at][0]:
                best[at] = (rank, r, c, n)
    out = {"label": [-1] * n_words, "score": [0.0] * n_words, "row": [-1] * n_words, "col": [-1] * n_words, "n_tokens": [-1] * n_words,
           "char_start": [0] * n_words, "char_end": [0] * n_words, "logits": [[math.nan] * L for _ in range(n_words)]}
    for at, (_, r, c, n) in best.items():
        v = []
        for l in range(L):
            cols = [np.float32(x[r, c + i, l]) for i in range(n)]
            if strategy == T.FIRST:
                v.append(cols[0])
            elif strategy == T.MEAN:
                total = cols[0]
                with np.errstate(invalid="ignore", over="ignore"):
                    for y in cols[1:]:
                        total = np.float32(total + y)
                    v.append(np.float32(total / np.float32(n)))
            else:
                real = [y for y in cols if not math.isnan(y)]
                v.append(max(real) if real else np.float32(math.nan))
        real = [y for y in v if not math.isnan(y)]
        label = min(l for l in range(L) if not math.isnan(v[l]) and v[l] >= max(real)) if real else -1
        score = math.nan
        if label >= 0 and len(real) == L and not math.isinf(v[label]):
            score = 1.0 / sum(math.exp(float(y) - float(v[label])) for y in v)
        out["label"][at], out["score"][at], out["logits"][at] = label, score, [float(y) for y in v]
        out["row"][at], out["col"][at], out["n_tokens"][at] = r, c, n
        out["char_start"][at], out["char_end"][at] = int(spans[r, c, 0]), int(spans[r, c + n - 1, 1])
    lost = sum(1 for at, r in taking if best[at][1] != r)
    out["info"] = [len(best), n_words - len(best), lost, skipped]
    return out


def same_as_loops(got, want):
    for k, w in want.items():
        g = np.asarray(got[k])
        if k == "score":
            assert np.allclose(g, np.asarray(w, dtype=np.float32), rtol=1e-6, atol=0, equal_nan=True), k
        else:
            assert np.array_equal(g.astype(np.float64), np.asarray(w, dtype=np.float64), equal_nan=True), (k, g, w)


def test_model_against_loops_on_random_rows():
    for seed, (rows, width, pair, L) in enumerate(((7, 9, False, 3), (9, 17, True, 5), (12, 6, False, 1), (5, 33, True, 9))):
        b = T.make_rows(rows, width, seed=seed, pair=pair, specials=seed % 2 == 0)
        if rows > 6:
            b["sample"][rows // 2] = b["n_samples"] + 3  # a row of no text
        side = 1 if pair else 0
        plan = T.expected_plan(b["word"], b["n_samples"], b["seq"], side, b["sample"])
        need = [0] * b["n_samples"]
        for r in range(rows):
            if b["sample"][r] < b["n_samples"]:
                for _, _, k, _ in loop_runs(b["word"], b["seq"], side, r):
                    need[b["sample"][r]] = max(need[b["sample"][r]], k + 1)
        assert plan["word_off"].tolist() == np.concatenate([[0], np.cumsum(need)]).tolist()
        assert plan["info"].tolist() == [sum(need), int((b["sample"] >= b["n_samples"]).sum())]
        x = T.small_logits((rows, width, L), seed)
        x[x == 7] = np.nan
        for strategy in (T.FIRST, T.MEAN, T.MAX):
            for off, n_words in ((plan["word_off"], None), (np.maximum(plan["word_off"].astype(np.int64) - 1, 0), int(plan["word_off"][-1]) + 2)):
                got = T.expected_predict(x, b["word"], b["spans"], off, b["seq"], side, b["sample"], strategy, n_words)
                same_as_loops(got, loop_predict(x, b["word"], b["spans"], off, b["seq"], side, b["sample"], strategy, n_words))


def test_a_cut_words_whole_copy_wins():
    """twelve tokens in three windows of six that overlap by three: word 3 (tokens 5 and 6) is cut at the end of the first window
    and at the start of the third, and lies whole in the middle of the second"""
    words = [0, 0, 1, 1, 2, 3, 3, 4, 4, 5, 5, 6]
    word, spans = T.windows(12, 6, 3, words)
    assert word.tolist() == [[0, 0, 1, 1, 2, 3], [1, 2, 3, 3, 4, 4], [3, 4, 4, 5, 5, 6]]
    sample = np.zeros(3, dtype=np.uint32)
    plan = T.expected_plan(word, 1, sample=sample)
    assert plan["word_off"].tolist() == [0, 7] and plan["info"].tolist() == [7, 0]
    x = np.zeros((3, 6, 3), dtype=np.float32)
    x[0, 5], x[1, 2], x[1, 3], x[2, 0] = (9, 0, 0), (0, 1, 0), (0, 0, 5), (9, 0, 0)  # the cut copies shout label 0
    got = T.expected_predict(x, word, spans, plan["word_off"], sample=sample)
    assert (got["row"][3], got["col"][3], got["n_tokens"][3], got["label"][3]) == (1, 2, 2, 1)
    assert (got["char_start"][3], got["char_end"][3]) == (10, 14)
    assert got["row"].tolist() == [0, 0, 0, 1, 2, 2, 2]  # word 1: contexts 2 and 0; word 2: 1 and 1, the earlier row; word 4: 0 and 1
    assert got["info"].tolist() == [7, 0, 5, 0]
    assert T.expected_predict(x, word, spans, plan["word_off"], sample=sample, strategy=T.MEAN)["label"][3] == 2  # (0, .5, 2.5)
    assert T.expected_predict(x, word, spans, plan["word_off"], sample=sample, strategy=T.MAX)["logits"][3].tolist() == [0, 1, 5]
    same_as_loops(got, loop_predict(x, word, spans, plan["word_off"], sample=sample))


def test_halves_of_a_word_tie_and_the_earlier_row_wins():
    """stride 0: word 2 is tokens 3 and 4, the last column of the first window and the first of the second, context 0 in both"""
    word, spans = T.windows(8, 4, 0, [0, 1, 1, 2, 2, 3, 3, 3])
    assert word.tolist() == [[0, 1, 1, 2], [2, 3, 3, 3]]
    sample = np.zeros(2, dtype=np.uint32)
    x = T.small_logits((2, 4, 4), 3)
    got = T.expected_predict(x, word, spans, [0, 4], sample=sample, strategy=T.MEAN)
    assert (got["row"][2], got["col"][2], got["n_tokens"][2], got["char_start"][2], got["char_end"][2]) == (0, 3, 1, 6, 8)
    assert got["logits"][2].tolist() == x[0, 3].tolist() and got["info"].tolist() == [4, 0, 1, 0]
    assert got["logits"][3].tolist() == ((x[1, 1] + x[1, 2] + x[1, 3]) / np.float32(3)).tolist()
    same_as_loops(got, loop_predict(x, word, spans, [0, 4], sample=sample, strategy=T.MEAN))
    # a text with no row, a word id no row names, words beyond the offsets
    got = T.expected_predict(x, word, spans, [0, 0, 5], sample=np.ones(2, dtype=np.uint32), n_words=6)
    assert got["label"][4:].tolist() == [-1, -1] and got["row"][4:].tolist() == [-1, -1] and np.isnan(got["logits"][4:]).all()
    assert got["score"][4:].tolist() == [0, 0] and got["info"].tolist() == [4, 2, 1, 0]


def test_labels_scores_and_special_values():
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    v = np.array([[1, 3, 3, 0], [nan, 2, 1, 2], [nan, nan, nan, nan], [0, inf, 1, 2], [-inf, 0, -inf, 0], [-inf, -inf, -inf, -inf],
                  [5, 5, 5, 5]], dtype=np.float32)
    label, score = T.labels_and_scores(v)
    assert label.tolist() == [1, 1, -1, 1, 1, 0, 0]
    assert math.isclose(score[0], 1 / (math.exp(-2) + 2 + math.exp(-3)), rel_tol=1e-6)
    assert np.isnan(score[[1, 2, 3, 5]]).all() and score[4] == 0.5 and score[6] == 0.25
    x = np.array([[[nan, 1], [2, nan], [nan, nan]]], dtype=np.float32)
    assert np.array_equal(T.word_vectors(x, np.array([0]), np.array([0]), np.array([3]), T.MAX), [[2, 1]])
    assert np.isnan(T.word_vectors(x, np.array([0]), np.array([0]), np.array([3]), T.MEAN)).all()
    assert np.array_equal(T.word_vectors(x, np.array([0]), np.array([2]), np.array([1]), T.MAX), [[nan, nan]], equal_nan=True)


ID2LABEL = ["O", "B-PER", "I-PER", "B-LOC", "I-LOC"]
ETYPE, BEGINS = np.array([-1, 0, 0, 1, 1], dtype=np.int32), np.array([0, 1, 0, 1, 0], dtype=np.uint8)


def test_entities_by_hand():
    #         text 0: B B | B I | O | I I | I-PER I-LOC | -1 inside | ends at the text's last word    text 1: starts with I-PER
    label = [1, 1, 1, 2, 0, 2, 2, 2, 4, 2, -1, 2, 1, 2, 2, 0, 2]
    n = len(label)
    score = (np.arange(n, dtype=np.float32) + 1) / np.float32(7)
    cs, ce = 10 * np.arange(n, dtype=np.uint32), 10 * np.arange(n, dtype=np.uint32) + 7
    got = T.expected_entities(label, score, cs, ce, [0, 14, 14, n], ETYPE, BEGINS)
    want = [(0, 0, 0, 0), (0, 0, 1, 1), (0, 0, 2, 3), (0, 0, 5, 7), (0, 1, 8, 8), (0, 0, 9, 9), (0, 0, 11, 11), (0, 0, 12, 13),
            (2, 0, 0, 0), (2, 0, 2, 2)]
    k = len(want)
    assert got["info"].tolist() == [k, 14]
    rec = list(zip(*(got[f].tolist() for f in ("text_index", "type", "first_word", "last_word"))))
    assert rec[:k] == want and rec[k:] == [(-1, -1, -1, -1)] * (n - k)
    assert got["char_start"][:k].tolist() == [0, 10, 20, 50, 80, 90, 110, 120, 140, 160] and got["char_end"][3] == 77
    assert got["char_start"][k:].tolist() == [0] * (n - k) and got["score"][k:].tolist() == [0] * (n - k)
    assert got["score"][3] == np.float32(np.float32(score[5] + score[6]) + score[7]) / np.float32(3)
    # a name without B- or I- is its own type and never begins; a label beyond the scheme is outside
    got = T.expected_entities([5, 5, 1, 9, 5], np.ones(5, np.float32), cs[:5], ce[:5], [0, 5], [-1, 0, 0, 1, 1, 2], [0, 1, 0, 1, 0, 0])
    assert got["info"].tolist() == [3, 4] and got["last_word"][:3].tolist() == [1, 2, 4] and got["type"][:3].tolist() == [2, 0, 2]
    assert T.expected_entities([], [], [], [], [0], ETYPE, BEGINS)["info"].tolist() == [0, 0]


def test_label_scheme_of_names(swt):
    from subword_tokenizers_amd import batching
    etype, begins, names = batching._label_scheme(ID2LABEL + ["MISC", "B-", "I-PER"])
    assert etype.tolist() == [-1, 0, 0, 1, 1, 2, 3, 0] and begins.tolist() == [0, 1, 0, 1, 0, 0, 0, 0] and names == ["PER", "LOC", "MISC", "B-"]
    assert [x.tolist() for x in batching._label_scheme(ID2LABEL)[:2]] == [ETYPE.tolist(), BEGINS.tolist()]
    for bad in (None, [], ["O", 1], "O"):
        with pytest.raises(TypeError):
            batching._label_scheme(bad)


# ---- the built library, without a device

NAMES = ("swt_word_plan", "swt_word_plan_dev", "swt_word_predict", "swt_word_predict_dev", "swt_entity_spans", "swt_entity_spans_dev",
         "swt_tag_capacity")


def test_symbols_and_constants(native):
    lib = C.CDLL(native._build.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name) and name in native.SIGNATURES, name
    cols, text_rows, scan_words = native.tag_capacity()
    assert cols >= 64 and cols % 4 == 0 and text_rows >= 64 and scan_words >= text_rows and scan_words % text_rows == 0
    assert (native.TAG_FIRST, native.TAG_MEAN, native.TAG_MAX) == (T.FIRST, T.MEAN, T.MAX) and native.TAG_STRATEGIES == T.STRATEGIES
    assert [n for n, _ in native.WORD_OUT] == ["label", "score", "row", "col", "n_tokens", "char_start", "char_end"]


ROWS, WIDTH, TEXTS, LABELS, WORDS = 3, 4, 2, 3, 4
CELLS = ROWS * WIDTH


def _arrays():
    """an array for every pointer of the three host forms, all apart from each other"""
    u32, i32, f32 = np.uint32, np.int32, np.float32
    a = {"logits": np.zeros(CELLS * LABELS, f32), "word": np.zeros(CELLS, u32), "seq": np.zeros(CELLS, np.int8), "sample": np.zeros(ROWS, u32),
         "spans": np.zeros(2 * CELLS, u32), "word_off": np.array([0, 2, 4], np.uint64), "out_word_off": np.full(4, 9, np.uint64),
         "info": np.full(4, 9, np.uint64), "out_logits": np.zeros(WORDS * LABELS, f32), "label": np.zeros(WORDS, i32),
         "score": np.zeros(WORDS, f32), "char_start": np.zeros(WORDS, u32), "char_end": np.zeros(WORDS, u32), "etype": np.zeros(LABELS, i32),
         "begins": np.zeros(LABELS, np.uint8)}
    a.update((k, np.full(WORDS, 5, t)) for k, t in (("out_label", i32), ("out_score", f32), ("out_row", i32), ("out_col", i32),
                                                    ("out_ncols", i32), ("out_char_start", u32), ("out_char_end", u32), ("ent_text", i32),
                                                    ("ent_type", i32), ("ent_first_word", i32), ("ent_last_word", i32),
                                                    ("ent_char_start", u32), ("ent_char_end", u32), ("ent_score", f32)))
    return a


# the arguments of each host form in order: a name of _arrays(), or (name, value) for a scalar
FORMS = {
    "swt_word_plan": ["word", "seq", ("side", 0), "sample", ("rows", ROWS), ("width", WIDTH), ("n_samples", TEXTS), "out_word_off", "info"],
    "swt_word_predict": ["logits", "word", "seq", ("side", 0), "sample", "spans", ("rows", ROWS), ("width", WIDTH), ("n_labels", LABELS),
                         "word_off", ("n_samples", TEXTS), ("n_words", WORDS), ("strategy", 0), "out_label", "out_score", "out_row", "out_col",
                         "out_ncols", "out_char_start", "out_char_end", "out_logits", "info"],
    "swt_entity_spans": ["label", "score", "char_start", "char_end", "word_off", ("n_samples", TEXTS), ("n_words", WORDS), "etype", "begins",
                         ("n_labels", LABELS), "ent_text", "ent_type", "ent_first_word", "ent_last_word", "ent_char_start", "ent_char_end",
                         "ent_score", "info"],
}
REQUIRED = {"swt_word_plan": ("word", "out_word_off", "info"), "swt_word_predict": ("logits", "word", "spans", "word_off"),
            "swt_entity_spans": ("label", "score", "char_start", "char_end", "word_off", "etype", "begins", "ent_text", "ent_type",
                                 "ent_first_word", "ent_last_word", "ent_char_start", "ent_char_end", "ent_score")}
FALLING_OFF, FALLING_SAMPLE = np.array([0, 3, 2], np.uint64), np.array([1, 0, 0], np.uint32)
BAD = {"swt_word_plan": [({"width": 0}, "width"), ({"rows": 1 << 32}, "rows"), ({"n_samples": 1 << 32}, "n_samples"), ({"side": 2}, "side"),
                         ({"side": -1}, "side"), ({"sample": FALLING_SAMPLE.ctypes.data}, "sample")],
       "swt_word_predict": [({"width": 0}, "width"), ({"rows": 1 << 31}, "rows"), ({"n_samples": 1 << 32}, "n_samples"), ({"side": 2}, "side"),
                            ({"n_labels": 0}, "n_labels"), ({"strategy": 3}, "strategy"), ({"strategy": 1 << 31}, "strategy"),
                            ({"n_labels": 1 << 30, "rows": 1 << 10}, "logits"), ({"n_words": 1 << 40}, "n_words"),
                            ({"width": 1 << 30, "rows": 1 << 8, "n_labels": 1}, "key"), ({"sample": FALLING_SAMPLE.ctypes.data}, "sample"),
                            ({"word_off": FALLING_OFF.ctypes.data}, "word_off"), ({"n_words": 3}, "word_off")],
       "swt_entity_spans": [({"n_samples": 1 << 32}, "n_samples"), ({"n_labels": 0}, "n_labels"), ({"n_words": 1 << 40}, "n_words"),
                            ({"word_off": FALLING_OFF.ctypes.data}, "word_off"), ({"n_words": 3}, "word_off")]}


def _call(native, form, arrays=None, **over):
    """one call of a host form; over: a pointer's name -> None or an address, a scalar's name -> its value"""
    arrays = arrays or _arrays()
    args = []
    for a in FORMS[form]:
        name, value = a if isinstance(a, tuple) else (a, arrays[a].ctypes.data)
        args.append(over.get(name, value))
    lib = native.lib()
    rc = getattr(lib, form)(*args)
    return rc, lib.swt_last_error().decode(), arrays


@pytest.mark.parametrize("form", sorted(FORMS))
def test_host_forms_refuse_bad_arguments_without_a_device(native, form):
    INV = native.ERR_INVALID
    pointers = [a for a in FORMS[form] if not isinstance(a, tuple)]
    for name in REQUIRED[form]:
        rc, msg, _ = _call(native, form, **{name: None})
        assert rc == INV and name in msg, (name, msg)
    for kw, word in BAD[form]:
        rc, msg, _ = _call(native, form, **kw)
        assert rc == INV and word in msg, (kw, msg)
    # every array off the alignment of its element type
    arrays = _arrays()
    for name in pointers:
        if arrays[name].dtype.itemsize > 1:
            rc, msg, _ = _call(native, form, arrays, **{name: arrays[name].ctypes.data + 1})
            assert rc == INV and name in msg and "aligned" in msg, (name, msg)
    # every output over every input, and over another output: the same address, and one shifted into it
    for out in [n for n in pointers if n.startswith(("out_", "ent_")) or n == "info"]:
        for other in pointers:
            if other == out:
                continue
            shift = 0 if arrays[other].nbytes < 16 else 8
            rc, msg, _ = _call(native, form, arrays, **{out: arrays[other].ctypes.data + shift})
            assert rc == INV and out in msg and "overlaps" in msg, (out, other, msg)
    # nothing to do: success without a device, the offsets and info zeroed, every word's "nothing" record written
    no_words = np.zeros(TEXTS + 1, np.uint64)
    empty = {"n_words": 0, "word_off": no_words.ctypes.data} if form == "swt_entity_spans" else {"rows": 0}
    rc, msg, arrays = _call(native, form, **empty)
    assert rc == 0, msg
    if form == "swt_word_plan":
        assert arrays["info"].tolist() == [0, 0, 9, 9] and arrays["out_word_off"].tolist() == [0, 0, 0, 9]
    elif form == "swt_word_predict":
        assert arrays["info"].tolist() == [0, WORDS, 0, 0]
        for k in ("out_label", "out_row", "out_col", "out_ncols"):
            assert arrays[k].tolist() == [-1] * WORDS
        for k in ("out_score", "out_char_start", "out_char_end"):
            assert arrays[k].tolist() == [0] * WORDS
        assert np.isnan(arrays["out_logits"]).all()
        rc, msg, arrays = _call(native, form, rows=0, seq=None, sample=None, **{k: None for k in pointers if k.startswith("out_")}, info=None)
        assert rc == 0, msg
    else:
        assert arrays["info"].tolist() == [0, 0, 9, 9] and arrays["ent_text"].tolist() == [5] * WORDS
        rc, msg, _ = _call(native, form, n_words=0, n_samples=0, info=None, **{k: None for k in REQUIRED[form] if k.startswith("ent_")})
        assert rc == 0, msg
    rc, msg, _ = _call(native, form, **empty, width=0, seq=None, sample=None)
    assert rc == 0, msg
    if native.device_count() == 0:  # everything in order: only now is a device looked for
        rc, _, _ = _call(native, form)
        assert rc == native.ERR_NO_DEVICE


# ---- the Python methods, where no device is needed

def _batch(rows=2, width=5, pair=False):
    b = {"input_ids": np.zeros((rows, width), dtype=np.int32), "attention_mask": np.ones((rows, width), dtype=np.uint8),
         "length": np.full(rows, width, dtype=np.uint32), "n_unknown": 0, "offset_mapping": np.zeros((rows, width, 2), dtype=np.uint32),
         "word_ids": np.full((rows, width), -1, dtype=np.int32)}
    if pair:
        b["sequence_ids"] = np.full((rows, width), -1, dtype=np.int8)
    return b


def test_methods_refuse_bad_arguments(swt):
    tok = swt.FastWP()
    f32 = np.zeros((2, 5, 3), dtype=np.float32)
    packed = {"input_ids": np.zeros((2, 5), dtype=np.int32), "sample_ids": np.zeros((2, 5), dtype=np.int32)}
    plain = {k: v for k, v in _batch().items() if k not in ("word_ids", "offset_mapping")}
    for bad in (None, [1, 2], {"labels": 1}, dict(_batch(), input_ids=[[0] * 5] * 2), dict(_batch(), word_ids=[[0] * 5] * 2)):
        with pytest.raises(TypeError):
            tok.word_predictions(bad, f32)
    for bad in (packed, plain):
        with pytest.raises(ValueError):
            tok.word_predictions(bad, f32)
    with pytest.raises(ValueError):
        tok.word_predictions(_batch(), f32, side=1)  # single rows have one side
    with pytest.raises(ValueError):
        tok.word_predictions(_batch(pair=True), f32)  # pair rows: whose words?
    for bad in (f32.astype(np.float64), f32.astype(np.float16), f32.tolist()):
        with pytest.raises(TypeError):
            tok.word_predictions(_batch(), bad)
    for bad in (f32[:, :4].copy(), f32[:, :, 0].copy(), f32[:, :, :0].copy(), f32[None]):
        with pytest.raises(ValueError):
            tok.word_predictions(_batch(), bad)
    with pytest.raises(ValueError):
        tok.word_predictions(_batch(), f32, strategy="last")
    words = {"word_offsets": np.array([0, 1], np.uint64), "label": np.zeros(1, np.int32), "score": np.zeros(1, np.float32),
             "char_start": np.zeros(1, np.uint32), "char_end": np.zeros(1, np.uint32)}
    for bad in (None, {"label": words["label"]}):
        with pytest.raises(TypeError):
            tok.entities(bad, ["O"])
    for bad in (None, [], ["O", 3]):
        with pytest.raises(TypeError):
            tok.entities(words, bad)
    with pytest.raises(TypeError):
        tok.entities(words, ["O"], texts="a")
    with pytest.raises(ValueError):
        tok.entities(words, ["O"], texts=["a", "b"])
