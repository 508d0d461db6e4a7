"""The project's own Python model of sentence-pair batches (include/swt.h, swt_batch_pair_plan / swt_batch_pair_rows; DESIGN.md
4.10), and the synthetic pair streams the GPU tests send through the device.  The model is held to
tests/golden/pair_batches.json -- what the `tokenizers` wheel gives for the pair template, the three truncation strategies, a
stride and padding -- by tests/test_pair_cases.py, without a GPU."""
import numpy as np

from .batch_cases import NONE, dense_id, spec, native_spec, window_count  # noqa: F401  (spec and native_spec: for the tests)

LONGEST_FIRST, ONLY_FIRST, ONLY_SECOND = 0, 1, 2
OK, REFUSED = 0, 1


def pair_cut(na, nb, cap, stride, windows, strategy):
    """-> (refused, keep_a, keep_b, side, step, k): the tokens each side keeps in a row, the side that is windowed (0 none, 1 A,
    2 B), the step of its windows and their number"""
    if na + nb <= cap:
        return False, na, nb, 0, 0, 1
    if strategy == LONGEST_FIRST:
        assert not windows
        n1, n2 = min(na, nb), max(na, nb)
        n2 = n1 if n1 > cap else max(n1, cap - n1)
        if n1 + n2 > cap:
            n1 = cap // 2
            n2 = n1 + cap % 2
        return (False, n1, n2, 0, 0, 1) if na <= nb else (False, n2, n1, 0, 0, 1)
    assert strategy in (ONLY_FIRST, ONLY_SECOND)
    kept, cut = (nb, na) if strategy == ONLY_FIRST else (na, nb)
    budget = cap - kept
    if budget < 1 or (windows and stride >= budget):
        return True, 0, 0, 0, 0, 1
    keep = (budget, nb) if strategy == ONLY_FIRST else (na, budget)
    if not windows:
        return False, keep[0], keep[1], 0, 0, 1
    step = budget - stride
    return False, keep[0], keep[1], 1 if strategy == ONLY_FIRST else 2, step, window_count(cut, budget, step)


def expected_pair_batch(rows_a, rows_b, s, strategy, cmap=None, payloads=None):
    """rows_a, rows_b: one list of raw ids per pair and side.  s: a batch_cases.spec; cls_id and sep_id both ids or both None.
    cmap: as expected_batch.  payloads: None, or ((spans of A, word of A), (spans of B, word of B)) -- per pair a list of
    (start, end) and a list of word indices.  -> dict of NumPy arrays as _native.batch_pair_rows returns them, plus "row_base",
    "status", "longest", "refused", "lost" and "n_unknown"."""
    table, n_map, flagged = (None, 1 << 31, False) if cmap is None else cmap
    sp = s["cls_id"] is not None
    assert sp == (s["sep_id"] is not None)
    width, windows = s["width"], s["windows"]
    cap = width - 3 * sp
    assert cap >= 1 and s["stride"] < cap
    cols = {k: [] for k in ("ids", "mask", "type", "special", "seq", "spans", "word")}
    length, sample, row_base, status = [], [], [0], []
    lost = refused = n_unknown = longest = 0
    pad = {"ids": s["pad_id"], "mask": 0, "type": 0, "special": 1, "seq": -1, "spans": (0, 0), "word": -1}
    for r, (ta, tb) in enumerate(zip(rows_a, rows_b)):
        na, nb = len(ta), len(tb)
        longest = max(longest, na + nb)
        no, keep_a, keep_b, side, step, k = pair_cut(na, nb, cap, s["stride"], windows, strategy)
        status.append(REFUSED if no else OK)
        refused += no
        if not no and not windows and na + nb > cap:
            lost += 1
        for w in range(k):
            row = {k_: [] for k_ in cols}

            def put(i, ty, special, seq, span=(0, 0), wd=-1):
                for k_, v in zip(("ids", "mask", "type", "special", "seq", "spans", "word"), (i, 1, ty, special, seq, span, wd)):
                    row[k_].append(v)

            def body(toks, which, lo, hi):
                nonlocal n_unknown
                for t in range(lo, hi):
                    d = dense_id(toks[t], table, n_map, flagged)
                    if d is None:
                        d = s["unk_id"]
                        n_unknown += 1
                    put(d, which, 0, which, tuple(payloads[which][0][r][t]) if payloads else (0, 0), payloads[which][1][r][t] if payloads else -1)

            if not no:
                lo_a = w * step if side == 1 else 0
                lo_b = w * step if side == 2 else 0
                if sp:
                    put(s["cls_id"], 0, 1, -1)
                body(ta, 0, lo_a, min(na, lo_a + keep_a))
                if sp:
                    put(s["sep_id"], 0, 1, -1)
                body(tb, 1, lo_b, min(nb, lo_b + keep_b))
                if sp:
                    put(s["sep_id"], 1, 1, -1)
            live = len(row["ids"])
            for k_ in cols:
                fill = [pad[k_]] * (width - live)
                cols[k_].append(fill + row[k_] if s["pad_left"] else row[k_] + fill)
            length.append(live)
            sample.append(r)
        row_base.append(len(length))
    n = len(length)
    idt = np.int64 if s["ids64"] else np.int32
    out = {
        "input_ids": np.array(cols["ids"], dtype=np.int64).astype(idt).reshape(n, width),
        "attention_mask": np.array(cols["mask"], dtype=np.uint8).reshape(n, width),
        "token_type_ids": np.array(cols["type"], dtype=idt).reshape(n, width),
        "special_tokens_mask": np.array(cols["special"], dtype=np.uint8).reshape(n, width),
        "sequence_ids": np.array(cols["seq"], dtype=np.int8).reshape(n, width),
        "length": np.array(length, dtype=np.uint32),
        "sample": np.array(sample, dtype=np.uint32),
        "row_base": np.array(row_base, dtype=np.uint64),
        "status": np.array(status, dtype=np.uint8),
        "longest": longest, "refused": refused, "lost": lost, "n_unknown": n_unknown,
    }
    if payloads:
        out["offset_mapping"] = np.array(cols["spans"], dtype=np.uint32).reshape(n, width, 2)
        out["word_ids"] = np.array(cols["word"], dtype=np.int32).reshape(n, width)
    return out


def side_seams(cap, stride, other):
    """lengths of the cut side at which its kept length or its window count changes, the other side holding `other` tokens"""
    budget = max(cap - other, 1)
    step = max(budget - stride, 1)
    return sorted({0, 1, max(budget - 1, 0), budget, budget + 1, budget + step, budget + step + 1})


def pair_stream(lengths, seed, id_lo=10, id_hi=5000, cont=False):
    """lengths: (na, nb) per pair -> (rows_a, rows_b, ids uint32, off_a, off_b uint64[n + 1], payloads): one seeded id stream that
    holds every A and then every B, as one encode of texts + text_pairs leaves it (off_b = the offsets from n on), with payloads
    in which every token slot is told apart from every other.  payloads as expected_pair_batch takes them."""
    rng = np.random.RandomState(seed)
    n = len(lengths)
    flat = [a for a, _ in lengths] + [b for _, b in lengths]
    rows, spans, word, t = [], [], [], 0
    for m in flat:
        r = rng.randint(id_lo, id_hi, size=m).astype(np.uint32)
        if cont and m:
            r |= (rng.randint(0, 2, size=m).astype(np.uint32) << np.uint32(31))
        rows.append([int(x) for x in r])
        spans.append([(2 * (t + i) + 1, 2 * (t + i) + 2) for i in range(m)])
        word.append([(7 * (t + i)) % 1000 for i in range(m)])
        t += m
    ids = np.array([x for r in rows for x in r], dtype=np.uint32)
    off = np.zeros(2 * n + 1, dtype=np.uint64)
    off[1:] = np.cumsum(np.array(flat, dtype=np.uint64))
    payloads = ((spans[:n], word[:n]), (spans[n:], word[n:]))
    return rows[:n], rows[n:], ids, off[:n + 1].copy(), off[n:].copy(), payloads


def flat_payloads(payloads):
    """-> (spans uint32[n, 2], word uint32[n]) in the order of pair_stream's ids"""
    spans = np.array([p for side in payloads for row in side[0] for p in row], dtype=np.uint32).reshape(-1, 2)
    word = np.array([w for side in payloads for row in side[1] for w in row], dtype=np.uint32)
    return spans, word
