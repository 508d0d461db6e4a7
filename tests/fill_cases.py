"""The NumPy model of masked-LM inference (swt_mlm_positions, swt_mlm_predict; include/swt.h) and the builders of its test cases.
The reference has nothing of the sort: this file holds the semantics, and the kernels equal it element by element -- all but
out_lse, which is held to lse_tol of the float64 value.

THE ORDER of a row's entries that are no NaN: the greater logit first, among equal logits the smaller index.  The top-k is its
first k entries, the label's rank the number of entries in front of the label's."""
import math

import numpy as np

NO_POS = np.uint64(0xFFFFFFFFFFFFFFFF)
U = 2.0 ** -24  # the relative error of one float32 rounding


def expected_positions(ids, value, not_equal=False):
    """-> {"pos" uint64[cells]: the flat indices of the selected cells, ascending, NO_POS from the count on; "info": count, cells}"""
    flat = np.asarray(ids).reshape(-1).astype(np.int64)
    sel = (flat != int(value)) if not_equal else (flat == int(value))
    hits = np.flatnonzero(sel).astype(np.uint64)
    pos = np.full(flat.size, NO_POS, dtype=np.uint64)
    pos[:hits.size] = hits
    return {"pos": pos, "info": np.array([hits.size, flat.size], dtype=np.uint64)}


def row_order(x):
    """the indices of the entries of x that are no NaN, in the order: a stable sort on (-x, index)"""
    x = np.asarray(x, dtype=np.float32)
    keep = np.flatnonzero(~np.isnan(x))
    return keep[np.argsort(-x[keep].astype(np.float64), kind="stable")]


def row_lse(x):
    """m + log(sum exp(x - m)) in float64; NaN with a NaN entry, -inf when all are -inf, +inf with a +inf entry"""
    x = np.asarray(x, dtype=np.float64)
    if np.isnan(x).any():
        return float("nan")
    m = float(x.max())
    if math.isinf(m):
        return m
    return m + math.log(float(np.exp(x - m).sum()))


def row_rank(x, label):
    """the entries in front of (x[label], label) in the order, by counting; -1 for a label out of range or with a NaN logit"""
    x = np.asarray(x, dtype=np.float32)
    if not 0 <= label < x.size or np.isnan(x[label]):
        return -1
    v = x[label]
    return int((x > v).sum() + (x[:label] == v).sum())


def expected_predict(logits, pos, labels=None, k=0):
    """-> dict: lse float64[n]; top_id int32, top_logit float32 [n, k]; label_id, label_logit, label_rank [n] (None without
    labels); info uint64[5].  A position at or beyond rows * width gets the "nothing" record, as the `_dev` form gives it."""
    logits = np.asarray(logits, dtype=np.float32)
    rows, width, V = logits.shape
    flat = logits.reshape(rows * width, V)
    pos = np.asarray(pos, dtype=np.uint64)
    n = pos.size
    lab = None if labels is None else np.asarray(labels).reshape(-1).astype(np.int64)
    out = {"lse": np.full(n, np.nan, dtype=np.float64), "top_id": np.full((n, k), -1, dtype=np.int32),
           "top_logit": np.full((n, k), np.nan, dtype=np.float32), "label_id": np.full(n, -1, dtype=np.int32),
           "label_logit": np.full(n, np.nan, dtype=np.float32), "label_rank": np.full(n, -1, dtype=np.int32)}
    info = np.zeros(5, dtype=np.uint64)
    info[0] = n
    for p in range(n):
        if int(pos[p]) >= rows * width:
            continue
        x = flat[int(pos[p])]
        out["lse"][p] = row_lse(x)
        info[3] += int(np.isnan(x).any())
        first = row_order(x)[:k]
        out["top_id"][p, :first.size] = first
        out["top_logit"][p, :first.size] = x[first]
        if lab is not None:
            l = int(lab[int(pos[p])])
            if 0 <= l < V:
                out["label_id"][p] = l
                out["label_logit"][p] = x[l]
                r = out["label_rank"][p] = row_rank(x, l)
                info[1] += int(r == 0)
                info[2] += int(0 <= r < max(k, 1))
            else:
                info[4] += 1
    if lab is None:
        out["label_id"] = out["label_logit"] = out["label_rank"] = None
    if k == 0:
        out["top_id"] = out["top_logit"] = None
    out["info"] = info
    return out


# ---- the tolerance on out_lse

def chain(V, step):
    """the float32 additions with another nonzero term that a term of the sum passes at most (include/swt.h): in its lane, over
    the lane's four sums, over the wavefront; no order of V terms has more than V - 1"""
    return min(V - 1, -(-V // step) + 8)


def lse_tol(V, step, lse=0.0):
    """The absolute tolerance on out_lse for a row of V entries whose float64 log-sum-exp is `lse`.  The error of log S is the
    relative error of S = sum expf(x_i - m), m the exact maximum, and then:
      the arguments: x_i - m is one rounding, u |d_i| with d_i = m - x_i, and moves its term by d_i e^-d_i u; over the row that
        is u (sum p_i d_i) S with p_i = e^-d_i / S, and sum p_i d_i = H(p) - ln S <= ln V.  Taken as (1 + ln V) u;
      expf within 1 ulp: 2 u;
      one u per addition on the longest chain of a term, chain(V) of them; there is no rescaling;
      these compound as (1 + a)(1 + u)^(chain + 2) - 1 = r, and |d log S| <= r / (1 - r);
      logf within 1 ulp of a value in [0, ln V]: 2 u ln V;
      the rounding of m + log S: u |lse|."""
    r = (1.0 + (1.0 + math.log(V)) * U) * (1.0 + U) ** (chain(V, step) + 2) - 1.0
    return r / (1.0 - r) + 2.0 * U * math.log(V) + U * abs(lse)


def lse_cap(V, lse=0.0):
    """what no tolerance may exceed: the sum in any order"""
    return (V + math.log(V) + 8.0) * U * max(1.0, abs(lse))


# ---- case builders: rows of V float32

def normal_row(rng, V, scale=3.0):
    return (rng.standard_normal(V) * scale).astype(np.float32)


def tie_row(rng, V, values=3):
    """small integers: ties wherever two entries lie"""
    return rng.integers(0, values, size=V).astype(np.float32)


def zeros_row(rng, V, zeros):
    """`zeros` entries of 0.0 at random places among -inf: S is the integer `zeros` and lse = log(zeros)"""
    x = np.full(V, -np.inf, dtype=np.float32)
    x[rng.permutation(V)[:zeros]] = 0.0
    return x


def logits_of(rows_list, rows, width):
    """rows * width rows of V floats -> float32 [rows, width, V]"""
    a = np.stack([np.asarray(r, dtype=np.float32) for r in rows_list])
    assert a.shape[0] == rows * width
    return np.ascontiguousarray(a.reshape(rows, width, a.shape[1]))
