"""The project's own NumPy model of the fine-tuning labels (include/swt.h: swt_label_words, swt_answer_positions,
swt_answer_best) and the builders of its test cases.  The reference has nothing of the sort: this file holds the
semantics, and the kernels equal it element by element.  tests/test_label_cases.py holds the model against a literal restatement
in plain Python loops."""
import numpy as np

IGNORE = -100
NONE = 0xFFFFFFFF
INT_MAX = 2 ** 31 - 1


def _u(a):
    """32-bit integers of either sign as int64 values of their uint32 reading (-1 is 0xFFFFFFFF)"""
    a = np.asarray(a)
    return (a.astype(np.int64) & 0xFFFFFFFF) if a.dtype.kind == "i" else a.astype(np.int64)


def token_columns(word, seq, side):
    """bool [rows, width]: the columns that hold a token of the side in question"""
    return (np.asarray(seq) == side) if seq is not None else (_u(word) != NONE)


def _samples(sample, rows):
    return _u(sample) if sample is not None else np.arange(rows, dtype=np.int64)


def expected_labels(word, lab_off, lab, seq=None, side=0, sample=None, inside=None, all_tokens=False, ignore=IGNORE, dtype=np.int32):
    """-> dict: labels [rows, width] of dtype, status uint8[rows], info uint64[4]"""
    w = _u(word)
    rows, width = w.shape
    tok = token_columns(word, seq, side)
    off, lab = np.asarray(lab_off).astype(np.int64), np.asarray(lab, dtype=np.int64)
    n = off.size - 1
    s = _samples(sample, rows)
    known = s < n
    sc = np.where(known, s, 0)
    n_lab = np.where(known, off[sc + 1] - off[sc], 0) if n else np.zeros(rows, dtype=np.int64)
    left_tok = np.concatenate([np.zeros((rows, 1), dtype=bool), tok[:, :-1]], axis=1)
    left_w = np.concatenate([np.full((rows, 1), -1, dtype=np.int64), w[:, :-1]], axis=1)
    first = tok & (~left_tok | (left_w != w))
    mine = tok & known[:, None]
    has = mine & (w < n_lab[:, None])
    missing = mine & ~has
    idx = np.where(has, (off[sc][:, None] if n else 0) + w, 0)
    l = lab[idx] if lab.size else np.zeros(w.shape, dtype=np.int64)
    cont = l
    if inside is not None:
        inside = np.asarray(inside, dtype=np.int64)
        ok = (l >= 0) & (l < inside.size)
        cont = np.where(ok, inside[np.where(ok, l, 0)], l) if inside.size else l
    labels = np.full(w.shape, ignore, dtype=np.int64)
    labels[has & first] = l[has & first]
    rest = has & ~first
    if all_tokens:
        labels[rest] = cont[rest]
    info = [int((has & first).sum()) + (int(rest.sum()) if all_tokens else 0), 0 if all_tokens else int(rest.sum()), int(missing.sum()),
            int((~known).sum())]
    return {"labels": labels.astype(dtype), "status": missing.any(axis=1).astype(np.uint8), "info": np.array(info, dtype=np.uint64)}


def nothing_column(rows, width, length, cls, pad_left, ignore):
    """the column both positions take where a row does not hold its answer"""
    if not cls:
        return np.full(rows, ignore, dtype=np.int64)
    if not pad_left:
        return np.zeros(rows, dtype=np.int64)
    n = _u(length)
    return np.where((n > 0) & (n <= width), width - n, 0)


def expected_positions(spans, ans, word=None, seq=None, side=0, sample=None, length=None, cls=False, pad_left=False, ignore=IGNORE,
                       dtype=np.int32):
    """-> dict: start, end [rows] of dtype, has uint8[rows], hit uint8[n], info uint64[3]"""
    sp = _u(spans)
    rows, width = sp.shape[:2]
    tok = token_columns(word, seq, side)
    ans = _u(ans).reshape(-1, 2)
    n = ans.shape[0]
    s = _samples(sample, rows)
    known = s < n
    sc = np.where(known, s, 0)
    a = np.where(known, ans[sc, 0], NONE) if n else np.full(rows, NONE, dtype=np.int64)
    e = np.where(known, ans[sc, 1], 0) if n else np.zeros(rows, dtype=np.int64)
    answer = known & (a != NONE) & (a < e)
    col = np.broadcast_to(np.arange(width, dtype=np.int64), tok.shape)
    some = tok.any(axis=1)
    c0 = np.where(tok, col, width).min(axis=1, initial=width)
    c1 = np.where(tok, col, -1).max(axis=1, initial=-1)
    r = np.arange(rows)
    st, en = sp[..., 0], sp[..., 1]
    holds = some & answer
    holds[holds] = (st[r[holds], c0[holds]] <= a[holds]) & (en[r[holds], c1[holds]] >= e[holds])
    start = np.where(tok & (st <= a[:, None]), col, -1).max(axis=1, initial=-1)
    end = np.where(tok & (en >= e[:, None]), col, width).min(axis=1, initial=width)
    nothing = nothing_column(rows, width, length, cls, pad_left, ignore)
    hit = np.zeros(n, dtype=np.uint8)
    hit[s[holds]] = 1
    info = [int(holds.sum()), int((~holds & known).sum()), int((~known).sum())]
    return {"start": np.where(holds, start, nothing).astype(dtype), "end": np.where(holds, end, nothing).astype(dtype),
            "has": holds.astype(np.uint8), "hit": hit, "info": np.array(info, dtype=np.uint64)}


def best_of_row(sl, el, tok, max_len):
    """the first candidate (i, j) of one row in the order (higher float32 score, smaller i, smaller j) -> (score, i, j);
    (-inf, -1, -1) without one.  The comparison is explicit: the greatest score, then the first (i, j) in lexicographic order
    among the candidates that have it."""
    width = sl.size
    i, j = np.arange(width)[:, None], np.arange(width)[None, :]
    with np.errstate(invalid="ignore"):
        score = sl.astype(np.float32)[:, None] + el.astype(np.float32)[None, :]  # float32 + float32: one IEEE addition
    valid = tok[:, None] & tok[None, :] & (i <= j) & (j - i < max_len) & ~np.isnan(score)
    if not valid.any():
        return np.float32(-np.inf), -1, -1
    top = score[valid].max()
    at = np.argwhere(valid & (score == top))  # row-major: by i, then by j
    return np.float32(top), int(at[0, 0]), int(at[0, 1])


def expected_best(start_logit, end_logit, spans, n_samples, word=None, seq=None, side=0, sample=None, max_len=30, length=None, cls=False,
                  pad_left=False):
    """-> dict: per text score, null_score float32, row, start_col, end_col int32, char_start, char_end uint32; per row row_score,
    row_start, row_end; info uint64[2]"""
    sl, el = np.asarray(start_logit, dtype=np.float32), np.asarray(end_logit, dtype=np.float32)
    rows, width = sl.shape
    sp = _u(spans)
    tok = token_columns(word, seq, side)
    s = _samples(sample, rows)
    known = s < n_samples
    row_score, row_start, row_end = np.full(rows, -np.inf, dtype=np.float32), np.full(rows, -1, dtype=np.int32), np.full(rows, -1, dtype=np.int32)
    for r in np.flatnonzero(known):
        row_score[r], row_start[r], row_end[r] = best_of_row(sl[r], el[r], tok[r], min(max_len, width))
    out = {"score": np.full(n_samples, -np.inf, dtype=np.float32), "null_score": np.full(n_samples, np.inf, dtype=np.float32),
           "row": np.full(n_samples, -1, dtype=np.int32), "start_col": np.full(n_samples, -1, dtype=np.int32),
           "end_col": np.full(n_samples, -1, dtype=np.int32), "char_start": np.zeros(n_samples, dtype=np.uint32),
           "char_end": np.zeros(n_samples, dtype=np.uint32)}
    cls_col = nothing_column(rows, width, length, True, pad_left, 0)
    for r in range(rows):  # in row order: a later row needs a strictly higher score
        if not known[r]:
            continue
        t = int(s[r])
        if row_start[r] >= 0 and (out["row"][t] < 0 or row_score[r] > out["score"][t]):
            out["score"][t], out["row"][t], out["start_col"][t], out["end_col"][t] = row_score[r], r, row_start[r], row_end[r]
            out["char_start"][t], out["char_end"][t] = sp[r, row_start[r], 0], sp[r, row_end[r], 1]
        if cls:
            with np.errstate(invalid="ignore"):
                z = np.float32(sl[r, cls_col[r]]) + np.float32(el[r, cls_col[r]])
            if z < out["null_score"][t]:  # false for a NaN
                out["null_score"][t] = z
    out.update({"row_score": row_score, "row_start": row_start, "row_end": row_end,
                "info": np.array([int((row_start >= 0).sum()), int((out["row"] >= 0).sum())], dtype=np.uint64)})
    return out


# ---- case builders

def make_rows(rows, width, seed=0, pair=False, specials=True, pad_left=False, texts=None, fill=None):
    """Rows as encode_batch(..., return_offsets=True) lays them out: [CLS] tokens [SEP] and padding, or [CLS] A [SEP] B [SEP];
    words of one to three tokens whose first word may be one cut by the window before; spans that rise by token with gaps
    between words; a text for every one to three rows.  fill: the content length of every row (specials included), else random
    from 0 on -- a row of no content is all padding, as a refused pair's.
    -> dict: word int32 (-1 off the tokens), seq int8 or None, spans uint32 [rows, width, 2], sample uint32 (non-decreasing),
    length uint32, n_samples"""
    rng = np.random.default_rng(seed)
    word = np.full((rows, width), -1, dtype=np.int32)
    seq = np.full((rows, width), -1, dtype=np.int8)
    spans = np.zeros((rows, width, 2), dtype=np.uint32)
    length = np.zeros(rows, dtype=np.uint32)
    n_special = (3 if pair else 2) if specials else 0
    for r in range(rows):
        n = min(int(fill if fill is not None else rng.integers(0, width + 1)), width)
        if n < n_special + (2 if pair else 1):
            continue  # too short for a token of every side: a row of no content
        length[r] = n
        n_tok = n - n_special
        sides = [n_tok] if not pair else [int(rng.integers(1, n_tok)), 0]
        if pair:
            sides[1] = n_tok - sides[0]
        c = (width - n if pad_left else 0) + (1 if specials else 0)
        for side, count in enumerate(sides):
            k, pos, left = int(rng.integers(0, 5)), int(rng.integers(0, 40)), 0
            for _ in range(count):
                if left == 0:
                    left = int(rng.integers(1, 4))
                    pos += int(rng.integers(0, 3))
                n_chars = int(rng.integers(1, 6))
                word[r, c], seq[r, c], spans[r, c] = k, side, (pos, pos + n_chars)
                pos += n_chars
                left -= 1
                if left == 0:
                    k += 1
                c += 1
            c += 1 if specials else 0
    if texts is None:
        sample = np.repeat(np.arange(rows), rng.integers(1, 4, size=rows))[:rows].astype(np.uint32)
    else:
        sample = np.asarray(texts, dtype=np.uint32)
    return {"word": word, "seq": seq if pair else None, "spans": spans, "sample": sample, "length": length,
            "n_samples": int(sample.max()) + 1 if rows else 0}


def make_labels(batch, side=0, seed=0, n_classes=7, short=()):
    """labels for every word the rows of `batch` name -> (lab_off uint64[n + 1], lab int32); the texts in `short` get one label
    fewer than their rows need"""
    rng = np.random.default_rng(seed)
    tok = token_columns(batch["word"], batch["seq"], side)
    n = batch["n_samples"]
    need = np.zeros(n, dtype=np.int64)
    for r in range(tok.shape[0]):
        if tok[r].any() and batch["sample"][r] < n:
            need[batch["sample"][r]] = max(need[batch["sample"][r]], int(batch["word"][r][tok[r]].max()) + 1)
    for t in short:
        need[t] = max(need[t] - 1, 0)
    lab_off = np.concatenate([[0], np.cumsum(need)]).astype(np.uint64)
    return lab_off, rng.integers(0, n_classes, size=int(lab_off[-1])).astype(np.int32)


def make_answers(batch, side=0, seed=0):
    """an answer for most texts, cut from the spans of a row of the text: from a token's start (or one before or behind it) to a
    token's end (or one before or behind it); some texts have none -> uint32[n, 2]"""
    rng = np.random.default_rng(seed)
    n = batch["n_samples"]
    ans = np.full((n, 2), NONE, dtype=np.uint32)
    tok = token_columns(batch["word"], batch["seq"], side)
    for r in range(tok.shape[0]):
        t = int(batch["sample"][r])
        cols = np.flatnonzero(tok[r])
        if t >= n or not cols.size or rng.integers(0, 5) == 0:
            continue
        i, j = sorted(rng.integers(0, cols.size, size=2).tolist())
        a = max(int(batch["spans"][r, cols[i], 0]) + int(rng.integers(-1, 2)), 0)
        e = int(batch["spans"][r, cols[j], 1]) + int(rng.integers(-1, 2))
        if a < e:
            ans[t] = (a, e)
    return ans


def small_logits(shape, seed=0, low=-8, high=9):
    """float32 logits of small integers: every sum is exact and ties are real"""
    return np.random.default_rng(seed).integers(low, high, size=shape).astype(np.float32)
