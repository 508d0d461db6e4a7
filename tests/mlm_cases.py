"""The project's own NumPy model of masked-LM batches (include/swt.h, swt_mlm_mask) and the builders of its test
cases.  The reference has no masking: this file holds the semantics, and the kernel equals it bit for bit because the draws
are Philox4x32-10 by position -- a function of (seed, epoch, row, column) and nothing else."""
import numpy as np

IGNORE = -100
ONE = 1 << 32
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)
COUNTS = ("n_eligible", "n_selected", "n_masked", "n_random", "n_kept")


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Random123) over arrays (or scalars) of counters, on uint64 -> (x0, x1, x2, x3) as uint64 below 2^32"""
    c = [np.asarray(x, dtype=np.uint64) & MASK32 for x in (c0, c1, c2, c3)]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]  # 32 x 32 bits: no overflow of 64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK32]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return tuple(c)


def philox_scalar(counter, key):
    """the same in plain Python integers: what the NumPy form is checked against"""
    c, k = [int(x) for x in counter], [int(x) for x in key]
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + W0) & 0xFFFFFFFF, (k[1] + W1) & 0xFFFFFFFF]
    return c


def thresholds(probability=0.15, mask_share=0.8, random_share=0.1):
    """what the Python layer makes of its floats: (select_below, mask_below, random_below)"""
    mask_below = int(mask_share * 4294967296.0)
    return int(probability * 4294967296.0), mask_below, mask_below + int(random_share * 4294967296.0)


def spec(n_class, mask_id, probability=0.15, whole_word=True, seed=0, epoch=0, mask_share=0.8, random_share=0.1):
    s, m, r = thresholds(probability, mask_share, random_share)
    return {"n_class": n_class, "mask_id": mask_id, "select_below": s, "mask_below": m, "random_below": r, "seed": seed, "epoch": epoch,
            "whole_word": whole_word}


def classes(ids, cls_tab, n_class):
    idx = ids.astype(np.int64)
    inside = (idx >= 0) & (idx < n_class)
    cls = np.full(ids.shape, 2, dtype=np.uint8)
    cls[inside] = np.minimum(np.asarray(cls_tab, dtype=np.uint8)[idx[inside]], 2)
    return cls


def heads(cls, whole_word):
    """per column the column of its head (-1: none at or before it); meaningful on eligible columns"""
    rows, width = cls.shape
    if whole_word:
        left = np.concatenate([np.full((rows, 1), 2, dtype=np.uint8), cls[:, :-1]], axis=1)
        head = (cls == 0) | ((cls == 1) & (left == 2))
    else:
        head = cls < 2
    col = np.broadcast_to(np.arange(width, dtype=np.int64), cls.shape)
    return np.maximum.accumulate(np.where(head, col, -1), axis=1) if width else col.copy()


def expected_mlm(ids, cls_tab, rand_ids, s):
    """ids [rows, width] int32 or int64 -> dict: input_ids, labels (as ids), selected uint8, info uint64[5] and the five counts"""
    ids = np.asarray(ids)
    rows, width = ids.shape
    cls = classes(ids, cls_tab, s["n_class"])
    eligible = cls < 2
    h = heads(cls, s["whole_word"])
    row = np.broadcast_to(np.arange(rows, dtype=np.int64)[:, None], ids.shape)
    col = np.broadcast_to(np.arange(width, dtype=np.int64), ids.shape)
    k0, k1 = s["seed"] & 0xFFFFFFFF, s["seed"] >> 32
    x0 = philox(np.where(eligible, h, 0), row, s["epoch"], 0, k0, k1)[0]
    _, x1, x2, _ = philox(col, row, s["epoch"], 0, k0, k1)
    selected = eligible & (x0 < np.uint64(s["select_below"]))
    masked = selected & (x1 < np.uint64(s["mask_below"]))
    random = selected & ~masked & (x1 < np.uint64(s["random_below"]))
    out = ids.copy()
    out[masked] = s["mask_id"]
    if random.any():
        rand_ids = np.asarray(rand_ids, dtype=np.uint64)
        out[random] = rand_ids[((x2[random] * np.uint64(rand_ids.size)) >> np.uint64(32)).astype(np.int64)].astype(ids.dtype)
    labels = np.where(selected, ids, np.asarray(IGNORE, dtype=ids.dtype)).astype(ids.dtype)
    info = np.array([eligible.sum(), selected.sum(), masked.sum(), random.sum(), (selected & ~masked & ~random).sum()], dtype=np.uint64)
    res = {"input_ids": out, "labels": labels, "selected": selected.astype(np.uint8), "info": info}
    res.update((name, int(x)) for name, x in zip(COUNTS, info))
    return res


def expected_mlm_loop(ids, cls_tab, rand_ids, s):
    """the same column by column in plain Python: what expected_mlm is checked against"""
    ids = np.asarray(ids)
    out, labels, selected = ids.copy(), np.full_like(ids, IGNORE), np.zeros(ids.shape, dtype=np.uint8)
    info = [0] * 5
    key = (s["seed"] & 0xFFFFFFFF, s["seed"] >> 32)
    for r in range(ids.shape[0]):
        head, left = None, 2
        for c in range(ids.shape[1]):
            i = int(ids[r, c])
            k = min(int(cls_tab[i]), 2) if 0 <= i < s["n_class"] else 2
            if k < 2:
                if not s["whole_word"] or k == 0 or left == 2:
                    head = c
                info[0] += 1
                if philox_scalar((head, r, s["epoch"], 0), key)[0] < s["select_below"]:
                    _, x1, x2, _ = philox_scalar((c, r, s["epoch"], 0), key)
                    selected[r, c], labels[r, c] = 1, i
                    info[1] += 1
                    if x1 < s["mask_below"]:
                        out[r, c] = s["mask_id"]; info[2] += 1
                    elif x1 < s["random_below"]:
                        out[r, c] = int(rand_ids[(x2 * len(rand_ids)) >> 32]); info[3] += 1
                    else:
                        info[4] += 1
            left = k
    return {"input_ids": out, "labels": labels, "selected": selected, "info": np.array(info, dtype=np.uint64)}


# ---- case builders.  The toy vocabulary: ids 0..4 are class 2 ([PAD] [UNK] [CLS] [SEP] [MASK]), 5..19 start a word, 20..39 continue one
N_CLASS, PAD, UNK, CLS, SEP, MASK_ID = 40, 0, 1, 2, 3, 4
WORD, CONT = 5, 20


def toy_tables():
    cls_tab = np.array([2] * 5 + [0] * 15 + [1] * 20, dtype=np.uint8)
    return cls_tab, np.flatnonzero(cls_tab < 2).astype(np.uint32)


def random_rows(rows, width, seed, dtype=np.int32, p_cont=0.5, p_special=0.1, pad_tail=True):
    """rows of words of random length with specials between them and a padded tail of random length"""
    rng = np.random.RandomState(seed)
    u = rng.random_sample((rows, width))
    ids = np.where(u < p_special, rng.randint(0, 5, size=(rows, width)),
                   np.where(u < p_special + p_cont, rng.randint(CONT, N_CLASS, size=(rows, width)), rng.randint(WORD, CONT, size=(rows, width))))
    if pad_tail:
        fill = rng.randint(0, width + 1, size=rows)
        ids[np.arange(width)[None, :] >= fill[:, None]] = PAD
    return np.ascontiguousarray(ids.astype(dtype))


def long_word_rows(width, length, dtype=np.int32):
    """four rows: a word of `length` continuation tokens behind its first token, starting at columns 0..3 (cut by the width), the
    rest single-token words"""
    ids = np.full((4, width), WORD + 1, dtype=dtype)
    for r in range(4):
        ids[r, r] = WORD
        ids[r, r + 1:r + 1 + length] = CONT + (np.arange(max(0, min(length, width - r - 1))) % 20)
    return ids
