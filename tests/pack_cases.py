"""The project's own Python model of packed batches (include/swt.h, swt_pack_plan / swt_pack_rows) and the
generators of the GPU tests.  The reference packs nothing, so the model is the semantics; tests/test_pack_cases.py holds it,
without a GPU, to tests/batch_cases.expected_batch (itself pinned to the `tokenizers` wheel) and to properties it cannot
satisfy by accident."""
import numpy as np

from tests import batch_cases as B

NONE = 0xFFFFFFFF
WHOLE, SPLIT, DROP_LAST = 1, 2, 4


def segment_lengths(lengths, s, mode):
    """the columns of every source row's segment: [cls?] body [sep?], the body cut to cap tokens in WHOLE"""
    n_special = (s["cls_id"] is not None) + (s["sep_id"] is not None)
    cap = s["width"] - n_special
    assert cap >= 1 and s["stride"] == 0 and not s["windows"] and not s["pad_left"]
    return [(n if mode & SPLIT else min(n, cap)) + n_special for n in lengths]


def next_fit_loop(seg, width):
    """the sequential greedy loop -> the first source row of every packed row"""
    starts, used = [], 0
    for r, n in enumerate(seg):
        if r == 0 or used + n > width:
            starts.append(r)
            used = 0
        used += n
    return starts


def next_fit_search(seg, width):
    """the definition of the header: the orbit of 0 under next(r) = the largest q <= n with P[q] - P[r] <= width"""
    P = np.concatenate([[0], np.cumsum(np.array(seg, dtype=np.int64))])
    n, starts, r = len(seg), [], 0
    while r < n:
        starts.append(r)
        r = int(np.searchsorted(P, P[r] + width, side="right")) - 1
    return starts


def expected_plan(lengths, s, mode):
    """-> dict: slot uint64[n + 1], row_first uint64[n + 1], rows, longest, total, seg (the segment lengths)"""
    n, width = len(lengths), s["width"]
    seg = segment_lengths(lengths, s, mode)
    P = [0]
    for x in seg:
        P.append(P[-1] + x)
    total = P[-1]
    row_first = [n] * (n + 1)
    if mode & SPLIT:
        rows = total // width if mode & DROP_LAST else -(-total // width)
        slot = list(P)
        r = 0
        for b in range(min(rows, n + 1)):
            while P[r + 1] <= b * width:
                r += 1
            row_first[b] = r
    else:
        starts = next_fit_search(seg, width)
        rows = len(starts)
        slot, b = [], -1
        for r in range(n):
            if b + 1 < rows and starts[b + 1] == r:
                b += 1
            slot.append(b * width + P[r] - P[starts[b]])
        slot.append(slot[-1] + seg[-1] if n else 0)
        for b, r in enumerate(starts):
            row_first[b] = r
    return {"slot": np.array(slot, dtype=np.uint64), "row_first": np.array(row_first, dtype=np.uint64), "rows": rows,
            "longest": max(lengths) if n else 0, "total": total, "seg": seg}


def expected_pack(rows, s, mode, cmap=None):
    """rows: one list of raw ids per source row; s: a batch_cases.spec; cmap as expected_batch takes it.  -> the plan of
    expected_plan and the arrays of _native.pack_rows: input_ids, attention_mask, position_ids, sequence_ids and sample_ids
    (uint32, NONE on padding), length; "lost" and "n_unknown"."""
    table, n_map, flagged = (None, 1 << 31, False) if cmap is None else cmap
    width = s["width"]
    plan = expected_plan([len(r) for r in rows], s, mode)
    n_out = plan["rows"]
    cap = width - (s["cls_id"] is not None) - (s["sep_id"] is not None)
    ids = np.full(n_out * width, s["pad_id"], dtype=np.int64)
    mask = np.zeros(n_out * width, dtype=np.uint8)
    pos = np.zeros(n_out * width, dtype=np.uint32)
    seg = np.full(n_out * width, NONE, dtype=np.uint32)
    doc = np.full(n_out * width, NONE, dtype=np.uint32)
    lost = n_unknown = 0
    for r, toks in enumerate(rows):
        body = toks if mode & SPLIT else toks[:cap]
        lost += len(body) < len(toks)
        cols = ([s["cls_id"]] if s["cls_id"] is not None else []) + [None] * len(body) + ([s["sep_id"]] if s["sep_id"] is not None else [])
        first_tok = 1 if s["cls_id"] is not None else 0
        assert len(cols) == plan["seg"][r]
        at = int(plan["slot"][r])
        for p, c in enumerate(cols):
            x = at + p
            if x >= n_out * width:
                break  # the dropped last row
            if c is None:
                c = B.dense_id(body[p - first_tok], table, n_map, flagged)
                if c is None:
                    c = s["unk_id"]
                    n_unknown += 1
            assert mask[x] == 0, "two segments on one column"
            ids[x], mask[x], pos[x], doc[x] = c, 1, p, r
    # the segment number: the source row less the owner of the packed row's column 0.  SPLIT can give more packed rows than
    # row_first has entries; the model knows every owner
    P = np.concatenate([[0], np.cumsum(np.array(plan["seg"], dtype=np.int64))])
    for b in range(n_out):
        owner = int(np.searchsorted(P, b * width, side="right")) - 1 if mode & SPLIT else int(plan["row_first"][b])
        if b <= len(rows):
            assert owner == int(plan["row_first"][b])
        live = mask[b * width:(b + 1) * width] == 1
        seg[b * width:(b + 1) * width][live] = doc[b * width:(b + 1) * width][live] - owner
    out = dict(plan)
    out.update({
        "input_ids": (ids if s["ids64"] else ids.astype(np.int32)).reshape(n_out, width),
        "attention_mask": mask.reshape(n_out, width), "position_ids": pos.reshape(n_out, width),
        "sequence_ids": seg.reshape(n_out, width), "sample_ids": doc.reshape(n_out, width),
        "length": mask.reshape(n_out, width).sum(axis=1).astype(np.uint32), "lost": int(lost), "n_unknown": n_unknown,
    })
    return out


def native_mode(native, mode):
    return (native.PACK_SPLIT if mode & SPLIT else native.PACK_WHOLE) | (native.PACK_DROP_LAST if mode & DROP_LAST else 0)


def random_lengths(n, width, seed):
    """row lengths that fill rows unevenly: many short, some around the width, a few empty or long"""
    rng = np.random.RandomState(seed)
    pool = [0, 0, 1, 1, 2, 3, 3, 5, max(width // 3, 1), max(width // 2, 1), max(width - 3, 1), max(width - 2, 1), width - 1, width,
            width + 1, 2 * width + 1]
    return [int(x) for x in rng.choice(pool, size=n)]
