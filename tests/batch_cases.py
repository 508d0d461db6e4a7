"""The project's own Python model of model-ready batches (include/swt.h, swt_batch_plan / swt_batch_rows), and the
synthetic id streams the GPU tests send through the device.  The model is held to tests/golden/model_batches.json -- what the
`tokenizers` wheel gives for the same truncation, stride, template and padding -- by tests/test_batch_cases.py, without a GPU."""
import numpy as np

NONE = 0xFFFFFFFF
CONT = 0x80000000


def spec(width, stride=0, windows=False, pad_left=False, ids64=False, pad_id=0, unk_id=1, cls_id=None, sep_id=None):
    return {"width": width, "stride": stride, "windows": windows, "pad_left": pad_left, "ids64": ids64, "pad_id": pad_id,
            "unk_id": unk_id, "cls_id": cls_id, "sep_id": sep_id}


def native_spec(native, s):
    return native.batch_spec(s["width"], s["stride"], s["windows"], s["pad_left"], s["ids64"], s["pad_id"], s["unk_id"], s["cls_id"],
                             s["sep_id"])


def window_count(n, cap, step):
    return 1 if n <= cap else 1 + -(-(n - cap) // step)


def dense_id(raw, cmap, n_map, flagged):
    """-> dense id, or None for a token that goes to unk_id"""
    s = raw & 0x7FFFFFFF
    if s >= n_map:
        return None
    if cmap is None:
        return s
    d = int(cmap[s + (n_map if flagged and raw >> 31 else 0)])
    return None if d == NONE else d


def expected_batch(rows, s, cmap=None, payloads=None):
    """rows: one list of raw ids per source row.  cmap: None (the identity on every id), or (map, n_map, flagged) with map None
    for the identity below n_map.  payloads: None, or (spans, word) -- per source row a list of (start, end) and a list of word
    indices.  -> dict of NumPy arrays as _native.batch_rows returns them, plus "row_base", "lost" and "n_unknown"."""
    table, n_map, flagged = (None, 1 << 31, False) if cmap is None else cmap
    has_cls, has_sep = s["cls_id"] is not None, s["sep_id"] is not None
    cap = s["width"] - has_cls - has_sep
    assert cap >= 1 and s["stride"] < cap
    step = cap - s["stride"]
    ids, mask, length, sample, spans, word, row_base = [], [], [], [], [], [], [0]
    lost = n_unknown = 0
    for r, toks in enumerate(rows):
        n = len(toks)
        k = window_count(n, cap, step) if s["windows"] else 1
        if not s["windows"] and n > cap:
            lost += 1
        for w in range(k):
            lo = w * step
            hi = min(n, lo + cap)
            row, sp, wd = [], [], []
            if has_cls:
                row.append(s["cls_id"]); sp.append((0, 0)); wd.append(-1)
            for t in range(lo, hi):
                d = dense_id(toks[t], table, n_map, flagged)
                if d is None:
                    d = s["unk_id"]
                    n_unknown += 1
                row.append(d)
                sp.append(tuple(payloads[0][r][t]) if payloads else (0, 0))
                wd.append(payloads[1][r][t] if payloads else -1)
            if has_sep:
                row.append(s["sep_id"]); sp.append((0, 0)); wd.append(-1)
            live, pad = len(row), s["width"] - len(row)
            if s["pad_left"]:
                row, sp, wd, m = [s["pad_id"]] * pad + row, [(0, 0)] * pad + sp, [-1] * pad + wd, [0] * pad + [1] * live
            else:
                row, sp, wd, m = row + [s["pad_id"]] * pad, sp + [(0, 0)] * pad, wd + [-1] * pad, [1] * live + [0] * pad
            ids.append(row); mask.append(m); length.append(live); sample.append(r); spans.append(sp); word.append(wd)
        row_base.append(len(ids))
    width = s["width"]
    out = {
        "input_ids": np.array(ids, dtype=np.int64 if s["ids64"] else np.uint32).reshape(len(ids), width),
        "attention_mask": np.array(mask, dtype=np.uint8).reshape(len(ids), width),
        "length": np.array(length, dtype=np.uint32),
        "sample": np.array(sample, dtype=np.uint32),
        "row_base": np.array(row_base, dtype=np.uint64),
        "lost": lost,
        "n_unknown": n_unknown,
    }
    if not s["ids64"]:
        out["input_ids"] = out["input_ids"].view(np.int32)
    if payloads:
        out["offset_mapping"] = np.array(spans, dtype=np.uint32).reshape(len(ids), width, 2)
        out["word_ids"] = np.array(word, dtype=np.int32).reshape(len(ids), width)
    return out


def seam_lengths(cap, step):
    """row lengths at which the row count or the last row's fill changes"""
    return sorted({0, 1, max(cap - 1, 0), cap, cap + 1, cap + step, cap + step + 1})


def stream(lengths, seed, id_lo=10, id_hi=5000, cont=False):
    """-> (rows of raw ids, ids uint32, tok_off uint64, (spans rows, word rows)): a seeded id stream with payloads in which every
    token slot is told apart from every other"""
    rng = np.random.RandomState(seed)
    rows, spans, word, t = [], [], [], 0
    for n in lengths:
        r = rng.randint(id_lo, id_hi, size=n).astype(np.uint32)
        if cont and n:
            r |= (rng.randint(0, 2, size=n).astype(np.uint32) << np.uint32(31))
        rows.append([int(x) for x in r])
        spans.append([(2 * (t + i) + 1, 2 * (t + i) + 2) for i in range(n)])
        word.append([(7 * (t + i)) % 1000 for i in range(n)])
        t += n
    ids = np.array([x for r in rows for x in r], dtype=np.uint32)
    off = np.zeros(len(lengths) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(np.array(lengths, dtype=np.uint64))
    return rows, ids, off, (spans, word)


def flat_payloads(payloads):
    spans = np.array([p for row in payloads[0] for p in row], dtype=np.uint32).reshape(-1, 2)
    word = np.array([w for row in payloads[1] for w in row], dtype=np.uint32)
    return spans, word
