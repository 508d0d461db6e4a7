"""The project's own model of span-corruption batches (include/swt.h, swt_denoise_rows) in plain Python, row by
row, and the builders of its test cases.  The reference has no span corruption: this file holds the semantics.  All arithmetic
is integer, so the kernel equals it exactly."""
import functools

import numpy as np

from tests import mlm_cases as M

ONE, MASK, SENTINEL, INFILL = 1 << 32, 0, 1, 2
COUNTS = ("n_eligible", "n_noise", "n_runs", "n_runs_returned", "n_rows_cut", "max_length", "max_label_length")

# the toy vocabulary: twelve ids of all three classes; the sentinels lie outside the class table, which makes them class 2
N_CLASS, PAD, UNK, SEP, MASK_ID, WORD, CONT = 12, 0, 1, 2, 3, 4, 8
CLS_TAB = np.array([2] * 4 + [0] * 4 + [1] * 4, dtype=np.uint8)
SENTINELS = np.arange(100, 140, dtype=np.uint32)


def spec(mode, start_below, len_below, whole_word=True, seed=0, epoch=0, n_sentinel=len(SENTINELS), label_width=None):
    """label_width None: that of the longest label row"""
    return {"mode": mode, "start_below": start_below, "len_below": list(len_below), "whole_word": whole_word, "seed": seed, "epoch": epoch,
            "n_sentinel": n_sentinel, "label_width": label_width, "n_class": N_CLASS, "mask_id": MASK_ID, "pad_id": PAD}


def noise_runs(ids, cls_tab, s):
    """per row the runs of noise columns, each a list of columns, and the eligible columns of all rows"""
    cls = M.classes(ids, cls_tab, s["n_class"])
    head = M.heads(cls, s["whole_word"])
    key = (s["seed"] & 0xFFFFFFFF, s["seed"] >> 32)
    rows = []
    for r in range(ids.shape[0]):
        unit, reach, runs, last = -1, 0, [], None
        for c in range(ids.shape[1]):
            if cls[r, c] == 2:
                continue
            if head[r, c] == c:  # a new unit, and its draw
                unit += 1
                x = M.philox_scalar((c, r, s["epoch"], 1), key)
                if x[0] < s["start_below"]:
                    reach = max(reach, unit + 1 + sum(x[1] >= t for t in s["len_below"]))
            if reach > unit:
                if last == c - 1:
                    runs[-1].append(c)
                else:
                    runs.append([c])
                last = c
        rows.append(runs)
    return rows, int((cls < 2).sum())


def expected(ids, cls_tab, s, sentinels=SENTINELS):
    """-> dict: input_ids, labels, attention_mask, length, label_length (None where the mode has none), info uint64[7]"""
    ids = np.asarray(ids)
    n_rows, width = ids.shape
    all_runs, eligible = noise_runs(ids, cls_tab, s)
    mode = s["mode"]
    cap = s["n_sentinel"] - 1 if mode == SENTINEL else width + 1
    rows, labels, info = [], [], [eligible, 0, 0, 0, 0, 0, 0]
    for r, runs in enumerate(all_runs):
        info[2] += len(runs)
        info[3] += len(runs[cap:])
        runs = runs[:cap]
        info[1] += sum(map(len, runs))
        start = {run[0]: k for k, run in enumerate(runs)}
        noise = {c for run in runs for c in run}
        row, lab = [], []
        for c in range(width):
            i = int(ids[r, c])
            if mode == MASK:
                row.append((s["mask_id"], 1) if c in noise else (i, 1))
                lab.append(i if c in noise else M.IGNORE)
                continue
            if c in start:
                mark = int(sentinels[start[c]]) if mode == SENTINEL else s["mask_id"]
                row.append((mark, 1))
                lab.append(mark)
            if c in noise:
                lab.append(i)
            else:
                row.append((i, int(i != s["pad_id"])))
        if mode == SENTINEL:
            lab.append(int(sentinels[len(runs)]))
        rows.append(row)
        labels.append(lab if mode != INFILL else [])
    lab_len = [len(lab) if mode == SENTINEL else 0 for lab in labels]
    lab_width = width if mode == MASK else max(lab_len, default=0) if s["label_width"] is None else s["label_width"]
    info[4] = sum(n > lab_width for n in lab_len)
    info[5], info[6] = max(map(len, rows), default=0), max(lab_len, default=0)
    res = {"input_ids": np.array([[i for i, _ in row] + [s["pad_id"]] * (width - len(row)) for row in rows], dtype=ids.dtype).reshape(n_rows, width),
           "labels": np.array([(lab + [M.IGNORE] * lab_width)[:lab_width] for lab in labels], dtype=ids.dtype).reshape(n_rows, lab_width),
           "attention_mask": np.array([[m for _, m in row] + [0] * (width - len(row)) for row in rows], dtype=np.uint8).reshape(n_rows, width),
           "length": np.array(list(map(len, rows)), dtype=np.uint32), "label_length": np.array(lab_len, dtype=np.uint32),
           "info": np.array(info, dtype=np.uint64)}
    res.update((k, None) for k in {MASK: ("attention_mask", "length", "label_length"), SENTINEL: (), INFILL: ("labels", "label_length")}[mode])
    return res


WIDTHS = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 516)


def random_rows(rows, width, seed, dtype, p_special=0.1):
    """words of random length with specials between them and a padded tail of random length"""
    rng = np.random.RandomState(seed)
    u = rng.random_sample((rows, width))
    ids = np.where(u < p_special, rng.randint(0, WORD, size=(rows, width)),
                   np.where(u < 0.5, rng.randint(CONT, N_CLASS, size=(rows, width)), rng.randint(WORD, CONT, size=(rows, width))))
    ids[np.arange(width)[None, :] >= rng.randint(width // 2, width + 1, size=rows)[:, None]] = PAD
    return np.ascontiguousarray(ids.astype(dtype))


def seam_rows(width, dtype):
    """five rows: single-token words to the last column; a row that begins with '##' columns; [SEP] inside what a span covers, on
    both sides of the 256-column step; a fully padded row; one word from end to end"""
    ids = np.full((5, width), WORD + 1, dtype=dtype)
    ids[1, :3] = CONT
    ids[2, [7, width // 2 - 2, width // 2 + 1]] = SEP
    ids[3] = PAD
    ids[4, 1:] = CONT + 2
    return ids


@functools.lru_cache(maxsize=None)
def cases(dtype):
    """[(name, ids, keywords of spec)]: the shapes and thresholds of tests/test_gpu_denoise.py"""
    third, few = {"start_below": int(0.3 * ONE), "len_below": [ONE // 2, 3 * (ONE // 4)]}, {"start_below": ONE // 50, "len_below": [0] * 31}
    out = [("width %d" % w, random_rows(5, w, w, dtype), third) for w in WIDTHS]
    out += [("rows %d" % n, random_rows(n, 3, n, dtype), third) for n in (1, 65)]  # 65: one more than a wavefront holds, one lane a row
    out += [("seams %d %d" % (start >> 30, len(lens)), seam_rows(516, dtype), {"start_below": start, "len_below": lens})
            for start in (0, ONE, int(0.3 * ONE)) for lens in ([], [0] * 31)]
    out.append(("spans of 32 units across the steps", random_rows(5, 516, 9, dtype, 0.02), few))
    five = np.array([[WORD, SEP, WORD, CONT, SEP, WORD, SEP, WORD, SEP, WORD + 1, PAD]], dtype=dtype)
    out.append(("five runs, two sentinels", five, {"start_below": ONE, "len_below": [], "n_sentinel": 2}))
    out.append(("labels cut at 3", random_rows(5, 65, 1, dtype), dict(third, label_width=3)))
    return out
