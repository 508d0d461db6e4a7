"""The NumPy model of the fine-tuning labels (tests/label_cases.py) held, without a GPU, to a literal restatement in plain Python
loops -- the recipes' own loops, bounded to the context's columns -- and to hand-written cases; what the host forms refuse before
they look for a device; and the decisions of the Python methods that need none."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import label_cases as L


# ---- the literal restatement

def _is_token(b, side, r, c):
    return b["seq"][r, c] == side if b["seq"] is not None else b["word"][r, c] != -1


def labels_loop(b, side, lab_off, lab, inside, all_tokens, ignore=L.IGNORE):
    rows, width = b["word"].shape
    out = np.full((rows, width), ignore, dtype=np.int64)
    status, info = np.zeros(rows, dtype=np.uint8), [0, 0, 0, 0]
    n = len(lab_off) - 1
    for r in range(rows):
        s = int(b["sample"][r])
        if s >= n:
            info[3] += 1
            continue
        labels = [int(x) for x in lab[int(lab_off[s]):int(lab_off[s + 1])]]
        previous = None
        for c in range(width):
            k = int(b["word"][r, c]) if _is_token(b, side, r, c) else None
            if k is None:
                pass
            elif k >= len(labels):
                info[2] += 1
                status[r] = 1
            elif k != previous:
                out[r, c] = labels[k]
                info[0] += 1
            elif all_tokens:
                l = labels[k]
                out[r, c] = inside[l] if inside is not None and 0 <= l < len(inside) else l
                info[0] += 1
            else:
                info[1] += 1
            previous = k
    return out, status, info


def positions_loop(b, side, ans, cls, pad_left, ignore=L.IGNORE):
    rows, width = b["word"].shape
    start, end, has = np.zeros(rows, dtype=np.int64), np.zeros(rows, dtype=np.int64), np.zeros(rows, dtype=np.uint8)
    hit, info = np.zeros(len(ans), dtype=np.uint8), [0, 0, 0]
    for r in range(rows):
        s = int(b["sample"][r])
        nothing = ignore if not cls else (width - int(b["length"][r])) % width if pad_left else 0
        start[r] = end[r] = nothing
        if s >= len(ans):
            info[2] += 1
            continue
        a, e = int(ans[s][0]), int(ans[s][1])
        cols = [c for c in range(width) if _is_token(b, side, r, c)]
        off = b["spans"][r]
        if not cols or a == L.NONE or a >= e or not (off[cols[0]][0] <= a and off[cols[-1]][1] >= e):
            info[1] += 1
            continue
        i = 0
        while i < len(cols) and off[cols[i]][0] <= a:
            i += 1
        j = len(cols) - 1
        while j >= 0 and off[cols[j]][1] >= e:
            j -= 1
        start[r], end[r], has[r], hit[s] = cols[i - 1], cols[j + 1], 1, 1
        info[0] += 1
    return start, end, has, hit, info


def best_loop(b, side, sl, el, n_samples, max_len, cls, pad_left):
    rows, width = sl.shape
    per_row = []
    for r in range(rows):
        best = (-math.inf, L.INT_MAX, L.INT_MAX)
        if int(b["sample"][r]) < n_samples:
            for i in range(width):
                for j in range(i, min(i + max_len, width)):
                    if not (_is_token(b, side, r, i) and _is_token(b, side, r, j)):
                        continue
                    score = float(np.float32(sl[r, i]) + np.float32(el[r, j]))
                    if math.isnan(score):
                        continue
                    if score > best[0] or (score == best[0] and (i, j) < best[1:]):
                        best = (score, i, j)
        per_row.append(best if best[1] != L.INT_MAX else (-math.inf, -1, -1))
    texts = [[-math.inf, math.inf, -1, -1, -1, 0, 0] for _ in range(n_samples)]
    for r, (score, i, j) in enumerate(per_row):
        s = int(b["sample"][r])
        if s >= n_samples:
            continue
        t = texts[s]
        if i >= 0 and (t[2] < 0 or score > t[0]):
            t[0], t[2], t[3], t[4], t[5], t[6] = score, r, i, j, int(b["spans"][r, i, 0]), int(b["spans"][r, j, 1])
        if cls:
            c = (width - int(b["length"][r])) % width if pad_left else 0
            z = float(np.float32(sl[r, c]) + np.float32(el[r, c]))
            if z < t[1]:
                t[1] = z
    return per_row, texts


LAYOUTS = [(pair, side, pad_left, specials) for pair in (False, True) for side in ((0, 1) if pair else (0,)) for pad_left in (False, True)
           for specials in (False, True)]


@pytest.mark.parametrize("pair,side,pad_left,specials", LAYOUTS)
def test_model_equals_the_loops(pair, side, pad_left, specials):
    """36 rows a layout, 12 layouts: single and pair rows, both sides, left and right padding, with and without specials"""
    for width, seed in ((9, 1), (16, 2), (23, 3)):
        b = L.make_rows(12, width, seed=seed + 10 * side, pair=pair, specials=specials, pad_left=pad_left)
        n = b["n_samples"]
        b["sample"][-1] = n + 3  # a row of no text
        lab_off, lab = L.make_labels(b, side, seed, short=(1,))
        inside = np.array([0, 2, 2, 4, 4], dtype=np.int32)
        for all_tokens, ins in ((False, None), (True, None), (True, inside)):
            got = L.expected_labels(b["word"], lab_off, lab, b["seq"], side, b["sample"], ins, all_tokens)
            out, status, info = labels_loop(b, side, lab_off, lab, ins, all_tokens)
            assert np.array_equal(got["labels"], out) and np.array_equal(got["status"], status) and got["info"].tolist() == info
        assert info[2] > 0 or not L.token_columns(b["word"], b["seq"], side)[b["sample"] == 1].any()
        ans = L.make_answers(b, side, seed)
        got = L.expected_positions(b["spans"], ans, b["word"], b["seq"], side, b["sample"], b["length"], specials, pad_left)
        start, end, has, hit, info = positions_loop(b, side, ans, specials, pad_left)
        for k, want in (("start", start), ("end", end), ("has", has), ("hit", hit)):
            assert np.array_equal(got[k], want), k
        assert got["info"].tolist() == info
        sl, el = L.small_logits((12, width), seed, -3, 4), L.small_logits((12, width), seed + 50, -3, 4)
        sl[2, :] = np.nan
        el[3, ::2] = -np.inf
        for max_len in (1, 3, width + 2):
            got = L.expected_best(sl, el, b["spans"], n, b["word"], b["seq"], side, b["sample"], max_len, b["length"], specials, pad_left)
            per_row, texts = best_loop(b, side, sl, el, n, max_len, specials, pad_left)
            assert [(float(s), int(i), int(j)) for s, i, j in zip(got["row_score"], got["row_start"], got["row_end"])] == per_row
            names = ("score", "null_score", "row", "start_col", "end_col", "char_start", "char_end")
            assert [[float(got[k][t]) if "score" in k else int(got[k][t]) for k in names] for t in range(n)] == texts
            assert got["info"].tolist() == [sum(i >= 0 for _, i, _ in per_row), sum(t[2] >= 0 for t in texts)]


# ---- hand-written cases

def _single(words, spans=None, width=None):
    """one text's rows from lists of word indices (None: no token)"""
    width = width or max(len(w) for w in words)
    word = np.full((len(words), width), -1, dtype=np.int32)
    for r, ws in enumerate(words):
        for c, k in enumerate(ws):
            if k is not None:
                word[r, c] = k
    sp = np.zeros((len(words), width, 2), dtype=np.uint32)
    for r, row in enumerate(spans or []):
        for c, x in enumerate(row):
            if x is not None:
                sp[r, c] = x
    return word, sp


def test_a_word_cut_by_a_window_edge_is_labelled_in_both_windows():
    word, _ = _single([[None, 0, 1, 1, None], [None, 1, 1, 2, None]])
    got = L.expected_labels(word, [0, 3], [5, 6, 7], sample=np.array([0, 0], dtype=np.uint32))
    assert got["labels"].tolist() == [[-100, 5, 6, -100, -100], [-100, 6, -100, 7, -100]]
    assert got["info"].tolist() == [4, 2, 0, 0] and got["status"].tolist() == [0, 0]


def test_bio_inside_maps_only_non_first_columns():
    word, _ = _single([[None, 0, 0, 0, 1, 2, 2, None]])
    inside = [0, 2, 2, 4, 4]  # O, B-x -> I-x, I-x, B-y -> I-y, I-y
    got = L.expected_labels(word, [0, 3], [1, 0, 3], inside=inside, all_tokens=True)
    assert got["labels"].tolist() == [[-100, 1, 2, 2, 0, 3, 4, -100]]
    assert got["info"].tolist() == [6, 0, 0, 0]
    got = L.expected_labels(word, [0, 3], [1, 9, -1], inside=inside, all_tokens=True)  # labels outside the map stay
    assert got["labels"].tolist() == [[-100, 1, 2, 2, 9, -1, -1, -100]]
    got = L.expected_labels(word, [0, 2], [1, 0], inside=inside, all_tokens=True)  # word 2 has no label
    assert got["labels"].tolist() == [[-100, 1, 2, 2, 0, -100, -100, -100]] and got["status"].tolist() == [1] and got["info"][2] == 2


def test_answer_positions_by_hand():
    #          [CLS]  "ab"    "cd"     "ef"      [SEP]  pad
    spans = [[None, (0, 2), (3, 5), (6, 8), None, None]]
    word, sp = _single([[None, 0, 1, 2, None, None]], spans)

    def at(a, e, **kw):
        got = L.expected_positions(sp, [[a, e]], word, **kw)
        return int(got["start"][0]), int(got["end"][0]), int(got["has"][0])

    assert at(3, 5) == (2, 2, 1)
    assert at(2, 3) == (1, 2, 1)         # the gap between two tokens: the token before it to the token behind it
    assert at(0, 8) == (1, 3, 1)         # ends exactly at the window's last token
    assert at(6, 8) == (3, 3, 1)         # starts in the window's last token: no run into [SEP] and the padding
    assert at(6, 9) == (-100, -100, 0)   # one code point past the last token
    assert at(6, 9, cls=True) == (0, 0, 0)
    assert at(L.NONE, L.NONE, cls=True) == (0, 0, 0) and at(5, 5) == (-100, -100, 0)
    # left padding: [CLS] stands at width - length
    word, sp = _single([[None, None, None, 0, 1, None]], [[None, None, None, (0, 2), (3, 5), None]])
    got = L.expected_positions(sp, [[7, 9]], word, length=np.array([4], dtype=np.uint32), cls=True, pad_left=True)
    assert (int(got["start"][0]), int(got["end"][0])) == (2, 2)
    # a refused pair's row: all padding
    none = np.full((1, 6), -1, dtype=np.int8)
    got = L.expected_positions(np.zeros((1, 6, 2), dtype=np.uint32), [[0, 1]], seq=none, side=1, cls=True)
    assert (int(got["start"][0]), int(got["end"][0]), int(got["has"][0]), got["hit"].tolist()) == (0, 0, 0, [0])
    assert got["info"].tolist() == [0, 1, 0]


def test_best_span_ties_and_specials():
    word, sp = _single([[None, 0, 1, 2, 3, None]] * 3, [[None, (0, 1), (2, 3), (4, 5), (6, 7), None]] * 3)
    sample = np.array([0, 0, 1], dtype=np.uint32)
    sl = np.zeros((3, 6), dtype=np.float32)
    el = np.zeros((3, 6), dtype=np.float32)
    got = L.expected_best(sl, el, sp, 3, word, sample=sample, max_len=4)
    assert got["row_start"].tolist() == [1, 1, 1] and got["row_end"].tolist() == [1, 1, 1]  # all equal: smaller i, then smaller j
    assert got["row"].tolist() == [0, 2, -1] and got["score"].tolist() == [0.0, 0.0, -math.inf]  # across rows: the lower row
    assert got["char_start"].tolist() == [0, 0, 0] and got["char_end"].tolist() == [1, 1, 0] and got["null_score"].tolist() == [math.inf] * 3
    sl[0, 3], el[0, 2], el[0, 4] = 2, 2, 2
    got = L.expected_best(sl, el, sp, 3, word, sample=sample, max_len=4)
    assert (got["row_start"][0], got["row_end"][0], got["row_score"][0]) == (3, 4, 4.0)  # j >= i: (3, 2) is no span
    got = L.expected_best(sl, el, sp, 3, word, sample=sample, max_len=1)
    assert (got["row_start"][0], got["row_end"][0], got["row_score"][0]) == (2, 2, 2.0)  # (2, 2), (3, 3), (4, 4) tie: the smallest i
    sl[1, 2], el[1, 3] = 2, 2  # the second row of text 0 reaches the same score: the lower row stays
    got = L.expected_best(sl, el, sp, 3, word, sample=sample, max_len=4)
    assert got["row"][0] == 0 and got["row_score"][1] == 4.0
    sl[1, 2] = 3
    got = L.expected_best(sl, el, sp, 3, word, sample=sample, max_len=4)
    assert (got["row"][0], got["start_col"][0], got["end_col"][0], got["char_start"][0], got["char_end"][0]) == (1, 2, 3, 2, 5)
    # NaN logits never win; a row whose only candidate is -inf still returns it; [CLS] scores, the least that is no NaN
    sl[:], el[:] = np.nan, 1
    sl[0, 2] = -np.inf
    sl[:, 0] = (np.nan, 5, 7)
    el[:, 0] = 1
    got = L.expected_best(sl, el, sp, 3, word, sample=sample, max_len=2, cls=True)
    assert (got["row_score"][0], got["row_start"][0], got["row_end"][0]) == (-math.inf, 2, 2)
    assert got["row_start"].tolist()[1:] == [-1, -1] and got["row"].tolist() == [0, -1, -1] and got["info"].tolist() == [1, 1]
    assert got["null_score"].tolist() == [6.0, 8.0, math.inf]
    # the [CLS] column and the other side of a pair are no candidates
    seq = np.array([[-1, 0, 0, -1, 1, 1, -1]], dtype=np.int8)
    sl, el = np.full((1, 7), 9, dtype=np.float32), np.full((1, 7), 9, dtype=np.float32)
    sl[0, 4:6], el[0, 4:6] = 1, 1
    got = L.expected_best(sl, el, np.zeros((1, 7, 2), dtype=np.uint32), 1, seq=seq, side=1, max_len=30)
    assert (got["start_col"][0], got["end_col"][0], got["score"][0]) == (4, 4, 2.0)


# ---- the built library, without a device

NAMES = ("swt_label_words", "swt_label_words_dev", "swt_answer_positions", "swt_answer_positions_dev", "swt_answer_best",
         "swt_answer_best_dev", "swt_label_capacity")


def test_symbols_and_constants(native):
    lib = C.CDLL(native._build.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name) and name in native.SIGNATURES, name
    cols, scan_rows = native.label_capacity()
    assert cols >= 64 and cols % 4 == 0 and scan_rows >= 64
    assert (native.LABEL_ALL_TOKENS, native.LABEL_IDS64, native.ANSWER_CLS, native.ANSWER_PAD_LEFT) == (1, native.BATCH_IDS64, 1, 2)
    assert native.LABEL_IGNORE == L.IGNORE and native.NO_ANSWER == L.NONE


ROWS, WIDTH, TEXTS = 3, 4, 2
CELLS = ROWS * WIDTH


def _arrays():
    """an array for every pointer of the three host forms, all apart from each other"""
    u32, i32, f32 = np.uint32, np.int32, np.float32
    return {"word": np.zeros(CELLS, u32), "seq": np.zeros(CELLS, np.int8), "sample": np.zeros(ROWS, u32), "spans": np.zeros(2 * CELLS, u32),
            "len": np.full(ROWS, WIDTH, u32), "lab_off": np.array([0, 2, 4], np.uint64), "lab": np.zeros(4, i32), "inside": np.zeros(3, i32),
            "ans": np.array([0, 1, 2, 3], u32), "start_logit": np.zeros(CELLS, f32), "end_logit": np.zeros(CELLS, f32),
            "out_labels": np.zeros(CELLS, np.int64), "out_status": np.zeros(8, np.uint8), "info": np.full(4, 9, np.uint64),
            "out_start": np.zeros(ROWS, np.int64), "out_end": np.zeros(ROWS, np.int64), "out_has": np.zeros(8, np.uint8),
            "out_hit": np.full(8, 9, np.uint8), "out_score": np.zeros(TEXTS, f32), "out_null_score": np.zeros(TEXTS, f32),
            "out_row": np.zeros(TEXTS, i32), "out_start_col": np.zeros(TEXTS, i32), "out_end_col": np.zeros(TEXTS, i32),
            "out_char_start": np.zeros(TEXTS, u32), "out_char_end": np.zeros(TEXTS, u32), "out_row_score": np.zeros(ROWS, f32),
            "out_row_start": np.zeros(ROWS, i32), "out_row_end": np.zeros(ROWS, i32)}


# the arguments of each host form in order: a name of _arrays(), or (name, value) for a scalar
FORMS = {
    "swt_label_words": ["word", "seq", ("side", 0), "sample", ("rows", ROWS), ("width", WIDTH), "lab_off", "lab", ("n_lab", 4),
                        ("n_samples", TEXTS), "inside", ("n_inside", 3), ("ignore", -100), ("flags", 0), "out_labels", "out_status", "info"],
    "swt_answer_positions": ["spans", "word", "seq", ("side", 0), "sample", ("rows", ROWS), ("width", WIDTH), "ans", ("n_samples", TEXTS), "len",
                             ("ignore", -100), ("flags", 0), "out_start", "out_end", "out_has", "out_hit", "info"],
    "swt_answer_best": ["start_logit", "end_logit", "spans", "word", "seq", ("side", 0), "sample", ("rows", ROWS), ("width", WIDTH),
                        ("n_samples", TEXTS), ("max_len", 3), "len", ("flags", 0), "out_score", "out_null_score", "out_row", "out_start_col",
                        "out_end_col", "out_char_start", "out_char_end", "out_row_score", "out_row_start", "out_row_end", "info"],
}
REQUIRED = {"swt_label_words": ("word", "lab_off", "lab", "inside", "out_labels"),
            "swt_answer_positions": ("spans", "ans", "out_start", "out_end"),
            "swt_answer_best": ("start_logit", "end_logit", "spans", "out_score", "out_null_score", "out_row", "out_start_col", "out_end_col",
                                "out_char_start", "out_char_end")}


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
    rc, msg, _ = _call(native, form, word=None, seq=None)  # no word and no seq: nothing names the token columns
    assert rc == INV and "word" in msg
    if form != "swt_label_words":
        rc, msg, _ = _call(native, form, word=None, rows=0)  # seq alone names them
        assert rc == 0, msg
        rc, msg, _ = _call(native, form, len=None, flags=native.ANSWER_PAD_LEFT | native.ANSWER_CLS)
        assert rc == INV and "len" in msg
    bad = [({"width": 0}, "width"), ({"rows": 1 << 32}, "rows"), ({"n_samples": 1 << 32}, "n_samples"), ({"side": 2}, "side"),
           ({"side": -1}, "side"), ({"flags": 8}, "flag"), ({"flags": 64}, "flag")]
    falling_off, falling_sample = np.array([0, 3, 2], np.uint64), np.array([1, 0, 0], np.uint32)
    bad += {"swt_label_words": [({"flags": 2}, "flag"), ({"lab_off": falling_off.ctypes.data}, "lab_off"),
                                ({"n_lab": 3}, "lab_off")],
            "swt_answer_positions": [],
            "swt_answer_best": [({"max_len": 0}, "max_len"), ({"flags": 4}, "flag"), ({"rows": 1 << 31}, "rows"),
                                ({"sample": falling_sample.ctypes.data}, "sample")]}[form]
    for kw, word in bad:
        rc, msg, _ = _call(native, form, **kw)
        assert rc == INV and word in msg, (kw, msg)
    # every array off the alignment of its element type
    arrays = _arrays()
    for name in pointers:
        if arrays[name].dtype.itemsize > 1:
            rc, msg, _ = _call(native, form, arrays, **{name: arrays[name].ctypes.data + 1})
            assert rc == INV and name in msg and "aligned" in msg, (name, msg)
    # every output over every input, and over another output: the same address, and one shifted into it
    outputs = [n for n in pointers if n.startswith("out_") or n == "info"]
    for out in outputs:
        for other in pointers:
            if other == out:
                continue
            shift = 0 if arrays[other].nbytes < 16 else 8
            rc, msg, _ = _call(native, form, arrays, **{out: arrays[other].ctypes.data + shift})
            assert rc == INV and out in msg and "overlaps" in msg, (out, other, msg)
    # no row: success without a device, info and the hits zeroed, every text's "nothing" record written
    rc, msg, arrays = _call(native, form, rows=0)
    assert rc == 0, msg
    n_info = {"swt_label_words": 4, "swt_answer_positions": 3, "swt_answer_best": 2}[form]
    assert arrays["info"].tolist() == [0] * n_info + [9] * (4 - n_info)
    if form == "swt_answer_positions":
        assert arrays["out_hit"].tolist() == [0] * TEXTS + [9] * (8 - TEXTS)
    if form == "swt_answer_best":
        assert arrays["out_score"].tolist() == [-math.inf] * TEXTS and arrays["out_null_score"].tolist() == [math.inf] * TEXTS
        for k in ("out_row", "out_start_col", "out_end_col"):
            assert arrays[k].tolist() == [-1] * TEXTS
        assert arrays["out_char_start"].tolist() == [0] * TEXTS and arrays["out_char_end"].tolist() == [0] * TEXTS
        rc, msg, _ = _call(native, form, rows=0, n_samples=0, **{k: None for k in REQUIRED[form] if k.startswith("out_")})
        assert rc == 0, msg
    rc, msg, _ = _call(native, form, rows=0, width=0, info=None)
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
    f32 = np.zeros((2, 5), dtype=np.float32)
    calls = (lambda b, **kw: tok.align_word_labels(b, [[0], [1]], **kw), lambda b, **kw: tok.answer_positions(b, [(0, 1), None], **kw),
             lambda b, **kw: tok.best_answers(b, f32, f32, **kw))
    packed = {"input_ids": np.zeros((2, 5), dtype=np.int32), "sample_ids": np.zeros((2, 5), dtype=np.int32)}
    plain = {k: v for k, v in _batch().items() if k not in ("word_ids", "offset_mapping")}
    for call in calls:
        for bad in (None, [1, 2], {"labels": 1}, dict(_batch(), input_ids=[[0] * 5] * 2), dict(_batch(), word_ids=[[0] * 5] * 2)):
            with pytest.raises(TypeError):
                call(bad)
        for bad in (packed, plain):
            with pytest.raises(ValueError):
                call(bad)
        with pytest.raises(ValueError):
            call(_batch(), side=1)  # single rows have one side
        with pytest.raises(ValueError):
            call(_batch(pair=True), side=2)
    with pytest.raises(ValueError):
        tok.align_word_labels(_batch(pair=True), [[0], [1]])  # pair rows: whose words?
    for bad in (3, "ab", [1, 2], (np.zeros(3), np.zeros(2), 1)):
        with pytest.raises(TypeError):
            tok.align_word_labels(_batch(), bad)
    for bad in ((np.zeros(3, dtype=np.int32), np.array([0, 2, 1])), (np.zeros(3, dtype=np.int32), np.array([0, 2, 4]))):
        with pytest.raises(ValueError):
            tok.align_word_labels(_batch(), bad)
    with pytest.raises(TypeError):
        tok.answer_positions(_batch(), 5)
    for bad in ([(0, 1, 2), None], [(0, 1 << 32), None]):
        with pytest.raises(ValueError):
            tok.answer_positions(_batch(), bad)
    with pytest.raises(ValueError):
        tok.answer_positions(_batch(), [(0, 1), None], texts=["a"])
    for bad in (f32.astype(np.float64), f32.astype(np.float16), f32.tolist()):
        with pytest.raises(TypeError):
            tok.best_answers(_batch(), bad, f32)
        with pytest.raises(TypeError):
            tok.best_answers(_batch(), f32, bad)
    with pytest.raises(ValueError):
        tok.best_answers(_batch(), f32[:, :4].copy(), f32)
    with pytest.raises(ValueError):
        tok.best_answers(_batch(), f32, f32, max_answer_length=0)


def test_positions_in_the_original_string(swt):
    """"İ".lower() is two code points: positions into the original string move by the running sum of len(ch.lower())"""
    from subword_tokenizers_amd import batching
    t = "İİ aİb"
    assert len(t.lower()) == len(t) + 3
    assert batching._lower_positions(t, (0, 1, 2, 3, 4, 5, 6)) == [0, 2, 4, 5, 6, 8, 9]
    ans = batching._answers([(3, 6), None, (-1, -1), (1, 2)], [t, "x", "y", "abc"])
    assert ans.tolist() == [[5, 9], [L.NONE, L.NONE], [L.NONE, L.NONE], [1, 2]]
    assert t.lower()[5:9] == t[3:6].lower()
