"""The project's own NumPy model of token-classification inference (include/swt.h: swt_word_plan, swt_word_predict,
swt_entity_spans) and the builders of its test cases.  The reference has nothing of the sort: this file holds the
semantics, and the kernels equal it element by element -- the score of swt_word_predict alone within score_rtol(n_labels), for it
is modelled in float64.  tests/test_tag_cases.py holds the model against a restatement in plain Python loops."""
import numpy as np

from tests.label_cases import _samples, _u, make_rows, small_logits, token_columns  # noqa: F401 (the builders are used through here)

FIRST, MEAN, MAX = 0, 1, 2
STRATEGIES = {"first": FIRST, "mean": MEAN, "max": MAX}
NOTHING_ENTITY = (-1, -1, -1, -1, 0, 0, 0.0)


def score_rtol(n_labels):
    """the relative error allowed to out_score where it is finite: the argument's rounding (2^-24 / e per term), expf within 1 ulp,
    n_labels additions and one reciprocal over a sum >= 1 come to about (3.4 L + 1) 2^-24.  The largest the MI355X has shown, in
    2^-24: 1.7 at 2 labels, 2.6 at 3, 3.1 at 4, 3.0 at 5, 4.2 at 9, 8.8 at 33"""
    return 4 * (n_labels + 1) * 2.0 ** -24


def find_runs(word, seq=None, side=0):
    """the runs of every row, in row and then column order -> int64 arrays (row, first column, columns, word id, context)"""
    w = _u(word)
    rows, width = w.shape
    tok = token_columns(word, seq, side)
    left_tok = np.concatenate([np.zeros((rows, 1), dtype=bool), tok[:, :-1]], axis=1)
    left_w = np.concatenate([np.full((rows, 1), -1, dtype=np.int64), w[:, :-1]], axis=1)
    first = tok & (~left_tok | (left_w != w))
    out = []
    for r in range(rows):
        c0 = np.flatnonzero(first[r])
        if not c0.size:
            continue
        stops = np.append(np.flatnonzero(~tok[r] | first[r]), width)  # where a run ends: no token column, or the next run's first
        end = stops[np.searchsorted(stops, c0, side="right")]
        before = np.concatenate([[0], np.cumsum(tok[r])])  # token columns left of column c
        left, right = before[c0], before[width] - before[end]
        out.append(np.stack([np.full(c0.size, r), c0, end - c0, w[r, c0], np.minimum(left, right)]))
    runs = np.concatenate(out, axis=1) if out else np.zeros((5, 0), dtype=np.int64)
    return tuple(runs.astype(np.int64))


def expected_plan(word, n_samples, seq=None, side=0, sample=None):
    """-> dict: word_off uint64[n_samples + 1], info uint64[2]"""
    w = _u(word)
    rows = w.shape[0]
    tok = token_columns(word, seq, side)
    s = _samples(sample, rows)
    n_words = np.zeros(n_samples, dtype=np.int64)
    for r in range(rows):
        if s[r] < n_samples and tok[r].any():
            n_words[s[r]] = max(n_words[s[r]], int(w[r][tok[r]].max()) + 1)
    return {"word_off": np.concatenate([[0], np.cumsum(n_words)]).astype(np.uint64),
            "info": np.array([int(n_words.sum()), int((s >= n_samples).sum())], dtype=np.uint64)}


def word_vectors(logits, row, c0, ncols, strategy):
    """v [runs, L] in float32 with the stated orders"""
    x = np.asarray(logits, dtype=np.float32)
    v = x[row, c0].copy()
    if strategy == FIRST:
        return v
    for i in range(1, int(ncols.max()) if ncols.size else 0):
        on = ncols > i
        y = x[row[on], c0[on] + i]
        if strategy == MEAN:
            with np.errstate(invalid="ignore", over="ignore"):
                v[on] = v[on] + y  # float32 + float32: one IEEE addition, in column order
        else:
            with np.errstate(invalid="ignore"):
                take = ~np.isnan(y) & (np.isnan(v[on]) | (y > v[on]))
            v[on] = np.where(take, y, v[on])
    if strategy == MEAN:
        with np.errstate(invalid="ignore", over="ignore"):
            v = v / ncols.astype(np.float32)[:, None]  # one IEEE division
    return v.astype(np.float32)


def labels_and_scores(v):
    """-> (label int32: the smallest l whose v_l is no NaN and >= every entry that is none, -1 if all are; score float32: 1 /
    sum exp(v_l - v[label]) in float64, NaN where an entry is, or the label is -1)"""
    n = v.shape[0]
    valid = ~np.isnan(v)
    top = np.where(valid, v, -np.inf).max(axis=1, initial=-np.inf)
    hit = valid & (v == top[:, None])
    label = np.where(valid.any(axis=1), hit.argmax(axis=1), -1).astype(np.int32)
    m = np.where(label >= 0, v[np.arange(n), np.maximum(label, 0)].astype(np.float64), np.nan)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        score = 1.0 / np.exp(v.astype(np.float64) - m[:, None]).sum(axis=1)
    return label, score.astype(np.float32)


def expected_predict(logits, word, spans, word_off, seq=None, side=0, sample=None, strategy=FIRST, n_words=None):
    """-> dict: label, row, col, n_tokens int32, score float32, char_start, char_end uint32 [n_words], logits float32 [n_words, L],
    info uint64[4]"""
    x = np.asarray(logits, dtype=np.float32)
    rows, width, L = x.shape
    sp = _u(spans)
    off = np.asarray(word_off).astype(np.int64)
    n_samples = off.size - 1
    n_words = int(off[-1]) if n_words is None else int(n_words)
    s = _samples(sample, rows)
    row, c0, ncols, k, context = find_runs(word, seq, side)
    text = s[row]
    known = text < n_samples
    tc = np.where(known, text, 0)
    takes = known & (k < off[np.minimum(tc + 1, n_samples)] - off[tc]) & (off[tc] + k < n_words)  # no text at all: none is known
    at = np.where(takes, off[tc] + k, -1)
    # the winner of a word: greater context, then the smaller row, then the smaller first column
    order = np.lexsort((c0, row, -context, at))
    order = order[takes[order]]
    lead = order[np.concatenate([[True], at[order][1:] != at[order][:-1]])] if order.size else order
    winner_row = np.full(n_words, -1, dtype=np.int64)
    winner_row[at[lead]] = row[lead]
    is_lead = np.zeros(row.size, dtype=bool)
    is_lead[lead] = True
    lost = takes & ~is_lead & (winner_row[np.maximum(at, 0)] != row)
    out = {"label": np.full(n_words, -1, dtype=np.int32), "score": np.zeros(n_words, dtype=np.float32),
           "row": np.full(n_words, -1, dtype=np.int32), "col": np.full(n_words, -1, dtype=np.int32),
           "n_tokens": np.full(n_words, -1, dtype=np.int32), "char_start": np.zeros(n_words, dtype=np.uint32),
           "char_end": np.zeros(n_words, dtype=np.uint32), "logits": np.full((n_words, L), np.nan, dtype=np.float32)}
    g = at[lead]
    v = word_vectors(x, row[lead], c0[lead], ncols[lead], strategy)
    out["logits"][g] = v
    out["label"][g], out["score"][g] = labels_and_scores(v)
    out["row"][g], out["col"][g], out["n_tokens"][g] = row[lead], c0[lead], ncols[lead]
    out["char_start"][g] = sp[row[lead], c0[lead], 0]
    out["char_end"][g] = sp[row[lead], c0[lead] + ncols[lead] - 1, 1]
    out["info"] = np.array([lead.size, n_words - lead.size, int(lost.sum()), int((~takes).sum())], dtype=np.uint64)
    return out


def expected_entities(label, score, char_start, char_end, word_off, etype, begins):
    """-> dict: text_index, type, first_word, last_word int32, char_start, char_end uint32, score float32 [n_words]; info uint64[2]"""
    label, score = np.asarray(label, dtype=np.int64), np.asarray(score, dtype=np.float32)
    off = np.asarray(word_off).astype(np.int64)
    etype, begins = np.asarray(etype, dtype=np.int64), np.asarray(begins)
    n = label.size
    inside = (label >= 0) & (label < etype.size)
    safe = np.where(inside, label, 0)
    text = np.searchsorted(off, np.arange(n), side="right") - 1  # the last s with off[s] <= w
    in_text = (np.arange(n) < off[-1]) & (text >= 0)
    t = np.where(inside & in_text, etype[safe], -1) if etype.size else np.full(n, -1)
    first_of_text = in_text & (np.arange(n) == off[np.clip(text, 0, off.size - 1)])
    before = np.concatenate([[-1], t])[:n]
    head = (t >= 0) & (first_of_text | (before != t) | (begins[safe] != 0))
    out = {"text_index": np.full(n, -1, dtype=np.int32), "type": np.full(n, -1, dtype=np.int32), "first_word": np.full(n, -1, dtype=np.int32),
           "last_word": np.full(n, -1, dtype=np.int32), "char_start": np.zeros(n, dtype=np.uint32), "char_end": np.zeros(n, dtype=np.uint32),
           "score": np.zeros(n, dtype=np.float32)}
    for e, w in enumerate(np.flatnonzero(head)):
        last, total = w, np.float32(score[w])
        with np.errstate(invalid="ignore", over="ignore"):
            while last + 1 < off[text[w] + 1] and t[last + 1] == t[w] and not head[last + 1]:
                last += 1
                total = np.float32(total + score[last])  # float32 additions, in order
            mean = np.float32(total / np.float32(last - w + 1))
        out["text_index"][e], out["type"][e] = text[w], t[w]
        out["first_word"][e], out["last_word"][e] = w - off[text[w]], last - off[text[w]]
        out["char_start"][e], out["char_end"][e], out["score"][e] = np.asarray(char_start)[w], np.asarray(char_end)[last], mean
    out["info"] = np.array([int(head.sum()), int((t >= 0).sum())], dtype=np.uint64)
    return out


# ---- case builders

def scheme(n_labels):
    """a BIO scheme over n_labels labels: "O", then B-x, I-x pairs; a last label left over is a type of its own that never begins
    -> (etype int32, begins uint8)"""
    etype, begins = np.full(n_labels, -1, dtype=np.int32), np.zeros(n_labels, dtype=np.uint8)
    for l in range(1, n_labels):
        etype[l], begins[l] = (l - 1) // 2, (l % 2 == 1) and l + 1 < n_labels
    return etype, begins


def rows_of_runs(lengths, width, texts=None):
    """one row per (run length n, offset) with 0 <= offset < n: single rows without specials whose columns from `offset` on are
    runs of n columns with the word ids 0, 1, 2, ... (the columns before it one short run), so that over the rows of a length a
    run starts and ends at every column -> a batch as make_rows makes it, every row its own text unless `texts` says otherwise"""
    plan = [(n, o) for n in lengths for o in range(n)]
    rows = len(plan)
    word = np.zeros((rows, width), dtype=np.int32)
    for r, (n, o) in enumerate(plan):
        word[r] = np.where(np.arange(width) < o, 0, (np.arange(width) - o) // n + (1 if o else 0))
    spans = np.zeros((rows, width, 2), dtype=np.uint32)
    spans[..., 0] = 3 * np.arange(width)
    spans[..., 1] = 3 * np.arange(width) + 2
    sample = np.arange(rows, dtype=np.uint32) if texts is None else np.asarray(texts, dtype=np.uint32)
    return {"word": word, "seq": None, "spans": spans, "sample": sample, "length": np.full(rows, width, dtype=np.uint32),
            "n_samples": int(sample.max()) + 1}


def windows(n_tokens, width, stride, words):
    """the rows of one text of n_tokens tokens cut into windows of `width` columns that overlap by `stride`, as the window plans
    cut them (no specials): words[i] is the word of token i -> (word int32 [rows, width], spans uint32 [rows, width, 2])"""
    starts = [0]
    while starts[-1] + width < n_tokens:
        starts.append(starts[-1] + width - stride)
    word = np.full((len(starts), width), -1, dtype=np.int32)
    spans = np.zeros((len(starts), width, 2), dtype=np.uint32)
    for r, a in enumerate(starts):
        n = min(width, n_tokens - a)
        word[r, :n] = words[a:a + n]
        spans[r, :n, 0] = 2 * np.arange(a, a + n)
        spans[r, :n, 1] = 2 * np.arange(a, a + n) + 2
    return word, spans
