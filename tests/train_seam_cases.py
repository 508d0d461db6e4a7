"""Inputs that cross the internal limits of the device trainer (csrc/swt_bpe_train.hip), the CPU-side properties that show
a limit is crossed, and a plain recount model.  A plain module: tests/test_train_seam_inputs.py (no GPU) checks the inputs
against the oracle alone, tests/test_gpu_train_seams.py runs them on the device.

Every builder is deterministic (fixed seeds) and returns (sym uint32, word_off uint64, freq uint32) for
BpeTrainer.from_words / OracleBPETrainer.from_words, or a list of sentences for the WordPiece trainer.

Symbols: the planted corpora use code points as opaque ids.  FILL0.. are filler symbols, every one used once (pairs of
count = the word's frequency, never a winner before the planted pairs are gone); PLANT0.. are the planted pairs' symbols.

Slots: until the stream is squeezed a symbol stays in the slot of its first character and a merge leaves a hole in the slot
of its right symbol, so the slot of a symbol inside its word is the number of initial symbols before it (sym_lengths,
slot_offsets below).  The cases that rely on slot positions keep at least 70 % of the slots live to their last merge: the
host squeezes only below that (and the device test asserts stats()["squeezes"] == 0 for them).
"""
import numpy as np

SYM_BASE = 0x110000
SLICES = (1, 2, 7, 64, 5, 300)

# the trainer's limits, restated (csrc/swt_bpe_train.hip, csrc/swt_train.h)
K_STAGE = 24
K_TIE_SLOTS = 512
K_TIE_WORDS = 16
K_MAX_BATCH = 16
K_TIE_SET = 256
K_CAND_TARGET = 1024
K_CAND_HIGH = 2048
K_CAND_CAP = 8192
K_BIG_MERGE = 8192
K_BIG_WORDS = 128
K_AGG_SLOTS = 1536
K_SEG_START = 4096
K_SEG_OF = 65536
K_WP_STEP_LIST = 16384

FILL0 = 0x2000
PLANT0 = 0x100


def csr(words, freqs):
    off = np.zeros(len(words) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(w) for w in words])
    sym = np.fromiter((s for w in words for s in w), dtype=np.uint32, count=int(off[-1]))
    return sym, off, np.asarray(freqs, dtype=np.uint32)


def text_words(strings, freqs):
    return csr([[ord(c) for c in s] for s in strings], freqs)


class _Fill:
    """fresh symbols, each handed out once"""

    def __init__(self, start=FILL0):
        self.next = start

    def __call__(self, n=1):
        out = list(range(self.next, self.next + n))
        self.next += n
        return out


# ---------------------------------------------------------------------------------------------------------------- builders

def long_words():
    """kStage: words of 23, 24, 25, 47, 48, 49 and 73 slots over 2-4 letters among short words; runs of one letter that
    collapse into a single symbol (a window of holes only); unmerged filler keeps the stream above the squeeze threshold"""
    rng = np.random.default_rng(24)
    words, freqs = [], []
    for alpha in ("ab", "abc", "abcd"):
        for n in (23, 24, 25, 47, 48, 49, 73):
            for rep in range(2):
                words.append("".join(alpha[i] for i in rng.integers(0, len(alpha), size=n)))
                freqs.append(int(rng.integers(1, 4)))
    for n in (24, 25, 48, 49, 73):  # periodic: the winning pair on both sides of slot 24 and of slot 48
        words.append(("ab" * 40)[:n]); freqs.append(3)
        words.append(("abc" * 30)[:n]); freqs.append(2)
    for head, run in (("cbd" * 5, 32), ("dcb" * 7, 52), ("", 64), ("bcd", 70)):  # the run ends up as one symbol
        words.append(head + "a" * run); freqs.append(5)
    for n in range(2, 7):
        for rep in range(8):
            words.append("".join("abcd"[i] for i in rng.integers(0, 4, size=n)))
            freqs.append(int(rng.integers(1, 4)))
    sym, off, freq = text_words(words, freqs)
    fill = _Fill()
    extra = [fill(2) for _ in range(2600)]  # pairs of count 1: never merged here, never squeezed away
    s2, o2, f2 = csr(extra, [1] * len(extra))
    return np.concatenate([sym, s2]), np.concatenate([off, o2[1:] + off[-1]]), np.concatenate([freq, f2])


def tie_staging():
    """fast_tie_kernel stages 512 slots per 16 words of a wave.  Groups of 16 words: a word of 500-530 slots takes every place
    0..15 in turn among short words, so the others start inside, straddle or lie beyond the staged slots; one word of 1,100
    slots.  The tied pairs (count 2 each: once in a long or short word, once in the last group) sit at the head, the middle
    and the tail of the words, so their first positions are found in staged slots and in the stream."""
    rng = np.random.default_rng(512)
    fill = _Fill()
    words, freqs, planted = [], [], []
    nxt = [PLANT0]

    def plant():
        p = (nxt[0], nxt[0] + 1)
        nxt[0] += 2
        planted.append(p)
        return list(p)

    def word(n, where):  # n slots, a planted pair at each fraction in `where`
        w = fill(n)
        for fr in where:
            at = min(n - 2, int(fr * (n - 2)))
            w[at:at + 2] = plant()
        return w

    for place in range(17):
        big = 1100 if place == 16 else 500 + (place * 2) % 31
        for i in range(K_TIE_WORDS):
            if i == place % K_TIE_WORDS:
                words.append(word(big, (0.0, 0.5, 0.97, 1.0)))
            else:
                n = int(rng.integers(3, 40))
                words.append(word(n, () if i % 3 else ((1.0,) if i % 2 else (0.0,))))
            freqs.append(1)
    order = rng.permutation(len(planted))  # the second occurrences, in another order
    for i in order:
        words.append(list(planted[i]))
        freqs.append(1)
    return csr(words, freqs)


def _occ_word(fill, P, Q, k, lead, trail, sep):
    w = fill(1) if lead else []
    for i in range(k):
        w += [P, Q]
        if i + 1 < k and sep:
            w += fill(1)
    return w + (fill(1) if trail else [])


def delta_overflow(tied):
    """kEmitCap / kFlushBatch: words with 2, 3, 4, 5 and 8 occurrences of the winning pair (P, Q) between distinct neighbours
    (with and without a neighbour in front, behind and in between), frequencies 2..13, and the overlapping forms aaaa, aaaaa,
    ababab.  tied: a second pair (U, V), in words of its own, ties with (P, Q) -- the fast path merges both in one step and a
    batch parks the pair's own delta too."""
    fill = _Fill()
    P, Q, U, V = PLANT0, PLANT0 + 1, PLANT0 + 2, PLANT0 + 3
    words, freqs = [], []
    f = 2
    for k in (2, 3, 4, 5, 8):
        for lead, trail, sep in ((1, 1, 1), (0, 1, 1), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 0)):
            words.append(_occ_word(fill, P, Q, k, lead, trail, sep))
            freqs.append(f)
            f = f + 1 if f < 13 else 2
    total = sum(f * sum(1 for i in range(len(w) - 1) if w[i] == P and w[i + 1] == Q) for w, f in zip(words, freqs))
    a, b = ord("a"), ord("b")
    for w, fr in (([a] * 4, 3), ([a] * 5, 2), ([a, b] * 3, 4), ([a] * 11, 2), ([a, b] * 7 + [a], 3)):
        words.append(w); freqs.append(fr)
    if tied:
        words.append([U, V]); freqs.append(total - 7)
        words.append(fill(1) + [U, V] + fill(1)); freqs.append(7)
    return csr(words, freqs)


def plateau(n, shared=False, head=0):
    """n pairs (p_i, q_i) tie at the maximum (count 4) and share no symbol: each is in [x_i p_i q_i y_i] (frequency 2) and in
    [p_i q_i] (frequency 2), the first kind in one random order and the second in another, ids in a third.  Behind them a
    plateau at count 2 of the 2n pairs (x_i, m_i), (m_i, y_i) -- they share m_i.  shared: the words are chains
    [p_i q_i r_i] instead, (p_i, q_i) and (q_i, r_i) tie and share q_i from the first step on.
    head: a pair in front of the plateau with `head` distinct neighbours of count 1 (the candidate-list cases)."""
    rng = np.random.default_rng(1000 + n + (7 if shared else 0))
    fill = _Fill()
    ids = PLANT0 + rng.permutation(3 * n)
    words, freqs = [], []
    if head:
        H = PLANT0 + 3 * n
        for _ in range(head):
            words.append(fill(1) + [H, H + 1] + fill(1)); freqs.append(1)
    a_order, b_order = rng.permutation(n), rng.permutation(n)
    for i in a_order:
        p, q, r = (int(x) for x in ids[3 * i:3 * i + 3])
        if shared:
            words.append([p, q, r]); freqs.append(4)
        else:
            words.append(fill(1) + [p, q] + fill(1)); freqs.append(2)
    if not shared:
        for i in b_order:
            words.append([int(ids[3 * i]), int(ids[3 * i + 1])]); freqs.append(2)
    return csr(words, freqs)


def list_grows():
    """the candidate list grows past kCandHigh inside one round trip: 4 hub pairs (A_h, B_h) in 125 words [x A_h B_h y] each
    (frequency 4, x and y used once), above 1,200 pairs of count 1.  A re-plan lists the 4 + 1,000 pairs of count >= 4 (at most
    kCandTarget; the pairs of count 1 stay below theta).  The hubs' merges make 1,000 pairs (x, m_h), (m_h, y) of count 4,
    which cross theta and are pushed; from then on every second merge makes one more, [x m y] -> [xm y] -> [xmy]."""
    fill = _Fill()
    words, freqs = [], []
    for h in range(4):
        for _ in range(125):
            words.append(fill(1) + [PLANT0 + 2 * h, PLANT0 + 2 * h + 1] + fill(1)); freqs.append(4)
    for _ in range(1200):
        words.append(fill(2)); freqs.append(1)
    return csr(words, freqs)


def big_merge(wide):
    """kBigMerge / kBigWords: (P, Q) in 20,000 words [x P Q y] of frequency 1..3.  narrow: x, y from 3 symbols, every delta
    fits the LDS sums; wide: x, y from 700 symbols each, about 2,800 distinct neighbour pairs for kAggSlots = 1,536."""
    rng = np.random.default_rng(8192 + int(wide))
    n = 20000
    P, Q = PLANT0, PLANT0 + 1
    na = 700 if wide else 3
    x = FILL0 + rng.integers(0, na, size=n)
    y = FILL0 + 1000 + rng.integers(0, na, size=n)
    sym = np.stack([x, np.full(n, P), np.full(n, Q), y], axis=1).astype(np.uint32).reshape(-1)
    off = (4 * np.arange(n + 1)).astype(np.uint64)
    return sym, off, rng.integers(1, 4, size=n).astype(np.uint32)


def random_words(seed, alpha, n_words, lo, hi, fmax):
    rng = np.random.default_rng(seed)
    lens = rng.integers(lo, hi + 1, size=n_words)
    off = np.zeros(n_words + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens)
    sym = (97 + rng.integers(0, alpha, size=int(off[-1]))).astype(np.uint32)
    return sym, off, rng.integers(1, fmax + 1, size=n_words).astype(np.uint32)


def wp_sentences(kind):
    """the same shapes as text for NaiveWP.train: long = words of 23..73 letters among short ones; overflow = words with
    2..8 occurrences of 'pq' between distinct letters; twin = runs of one letter"""
    rng = np.random.default_rng(77)
    if kind == "long":
        ws = ["".join("abc"[i] for i in rng.integers(0, 3, size=n)) for n in (23, 24, 25, 47, 48, 49, 73) for _ in range(2)]
        ws += [("ab" * 40)[:n] for n in (25, 49, 73)]
        ws += ["".join("abc"[i] for i in rng.integers(0, 3, size=int(n))) for n in rng.integers(2, 7, size=40)]
        return [" ".join(ws[i::4]) for i in range(4)] * 2
    if kind == "overflow":
        letters = "cdefghijklmnorstuvwxyz"
        ws = []
        for k in (2, 3, 4, 5, 8):
            for shift in range(3):
                w = ""
                for i in range(k):
                    w += letters[(shift * 7 + i) % len(letters)] + "pq"
                ws.append(w + letters[(shift + k) % len(letters)])
        ws += ["aaaa", "aaaaa", "ababab", "pq", "pq"]
        return [" ".join(ws), " ".join(ws[::2]), " ".join(ws[1::3])]
    assert kind == "twin"
    return [" ".join("a" * n for n in (4, 5, 11, 24, 25, 26, 49, 2, 3)), "aaaa aaaaa " + "a" * 73, "b ab ba aab"]


# ---------------------------------------------------------------------------------------------------------------- case table

class Case:
    def __init__(self, name, seam, build, merges, witness, checks=(), first_merged=SYM_BASE, no_squeeze=False):
        self.name, self.seam, self.build, self.merges, self.witness = name, seam, build, merges, witness
        self.checks = tuple(checks) or (merges // 3, 2 * merges // 3, merges)  # merges after which the histogram is compared
        self.first_merged, self.no_squeeze = first_merged, no_squeeze

    def __repr__(self):
        return self.name


GROW_CALLS = (60, 180, 300)  # the run calls of test_list_grows_inside_one_round_trip: the list passes kCandHigh in the second

CASES = [
    Case("long_words", "kStage", long_words, 60, "stage_refill", no_squeeze=True),
    Case("tie_staging", "kTieStage*64", tie_staging, 170, "tie_beyond_512", no_squeeze=True),
    Case("overflow_single", "kEmitCap,kFlushBatch", lambda: delta_overflow(False), 60, "deltas_single"),
    Case("overflow_tied", "kEmitCap,kFlushBatch", lambda: delta_overflow(True), 60, "deltas_batch"),
    Case("plateau_15", "kMaxBatch", lambda: plateau(15), 40, "tied_eq"),
    Case("plateau_16", "kMaxBatch", lambda: plateau(16), 40, "tied_eq"),
    Case("plateau_17", "kMaxBatch", lambda: plateau(17), 45, "tied_eq"),
    Case("plateau_33", "kMaxBatch", lambda: plateau(33), 80, "tied_eq"),
    Case("plateau_255", "kTieSet", lambda: plateau(255), 400, "tied_eq"),
    Case("plateau_256", "kTieSet", lambda: plateau(256), 400, "tied_eq"),
    Case("plateau_257", "kTieSet", lambda: plateau(257), 400, "tied_eq"),
    Case("plateau_600", "kTieSet", lambda: plateau(600), 700, "tied_eq"),
    Case("plateau_shared_40", "kMaxBatch (dangerous pairs)", lambda: plateau(40, shared=True), 80, "tied_shared"),
    Case("cand_2100", "kCandHigh, list dry", lambda: plateau(2100, head=3000), 60, "cand_list"),
    Case("cand_8300", "kCandCap, list dry", lambda: plateau(8300, head=3000), 40, "cand_list"),
    Case("cand_grow", "kCandHigh (pushes in mid trip)", list_grows, 300, "cand_grow", checks=GROW_CALLS),
    Case("big_narrow", "kBigMerge,kBigWords", lambda: big_merge(False), 12, "big", checks=(1, 6, 12)),
    Case("big_wide", "kBigMerge,kBigWords,kAggSlots", lambda: big_merge(True), 30, "big", checks=(1, 15, 30)),
    Case("squeeze_resize", "squeeze_stream, table_resize", lambda: random_words(70, 6, 4000, 2, 9, 3), 500, "squeeze"),
    Case("seg_of_65536", "seg_of", long_words, 60, "seg_of", first_merged=SYM_BASE + 65530, no_squeeze=True),
    Case("seg_start_4096", "seg_start", lambda: random_words(4096, 26, 3000, 3, 8, 2), 5400, "steps", checks=(5400,)),
]
BY_NAME = {c.name: c for c in CASES}

REUSE = ("long_words", "overflow_tied", "plateau_17")  # the corpora of the id-reuse test (30 merges)
SHARDED = ("long_words", "overflow_single", "overflow_tied", "plateau_17", "plateau_257", "cand_8300")
SHARDED_CUTS = {"2": (0.4,), "2_first_empty": (0.0,), "3_middle_empty": (0.3, 0.3), "3_last_empty": (0.5, 1.0)}  # fractions of the words
# cand_8300 takes the sharded runner through its other branch: after the first merge 8,300 pairs tie, more than kCandCap / 2,
# so the re-plan lists nothing (theta = 0) and the rest of the run is generic steps inside the fast runner.  One cut shows it.
SHARDED_ONLY = {"cand_8300": ("2",)}
# the forced one-merge-per-step form (SWT_DIST_GENERIC=1): the smallest inputs with ties, with and without an empty rank
SHARDED_GENERIC = tuple((n, c) for n in ("plateau_17", "overflow_tied") for c in ("2", "3_middle_empty"))
WP_KINDS = ("long", "overflow", "twin")


# ---------------------------------------------------------------------------------------------------------------- CPU model

def pair_keys(sym, off):
    """(keys uint64, word index) of every adjacent pair inside a word of a hole-free stream"""
    sym = np.asarray(sym, dtype=np.uint64)
    off = np.asarray(off, dtype=np.int64)
    n = sym.size
    if n < 2:
        return np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.int64)
    word = np.searchsorted(off, np.arange(n), side="right") - 1
    inside = word[:-1] == word[1:]
    keys = ((sym[:-1] << np.uint64(32)) | sym[1:])[inside]
    return keys, word[:-1][inside]


def recount(sym, off, freq):
    """the pair histogram of a stream, counted from scratch: {left << 32 | right: count}"""
    keys, word = pair_keys(sym, off)
    want = {}
    for k, f in zip(keys.tolist(), np.asarray(freq, dtype=np.int64)[word].tolist()):
        want[k] = want.get(k, 0) + f
    return want


def sym_lengths(merge_ids):
    """initial symbols under every merged id: {id: n}; ids not in it are initial symbols (1)"""
    n = {}
    for l, r, m in np.asarray(merge_ids).tolist():
        n[m] = n.get(l, 1) + n.get(r, 1)
    return n


def slot_offsets(sym, off, lens):
    """the slot of every symbol inside its word, while the stream has not been squeezed"""
    ln = np.array([lens.get(int(s), 1) for s in sym], dtype=np.int64)
    start = np.cumsum(ln) - ln
    off = np.asarray(off, dtype=np.int64)
    word = np.searchsorted(off, np.arange(sym.size), side="right") - 1
    first = start[np.minimum(off[:-1], max(sym.size - 1, 0))] if sym.size else start
    return start - first[word], ln, word


def walk_deltas(seq, pairs):
    """deltas walk_word sends for one word when the step merges `pairs` (K = len(pairs)); 0 merges -> 0"""
    seq = [int(s) for s in seq]
    pairs = {(int(l), int(r)) for l, r in pairs}
    n = merged = 0
    have = cov = False
    i = 0
    while i < len(seq):
        if i + 1 < len(seq) and (seq[i], seq[i + 1]) in pairs:
            n += (2 if have else 0) + (1 if len(pairs) > 1 else 0)
            have = cov = True
            merged += 1
            i += 2
        else:
            n += 2 if (have and cov) else 0
            have, cov = True, False
            i += 1
    return n if merged else 0


class RecountModel:
    """bpe.py:88-111 with a full recount per merge, and merged ids given by the caller (so an id may be reused): the pair
    with the highest count wins, ties go to the pair met first in the stream; a merge replaces left to right"""

    def __init__(self, sym, off, freq):
        off = np.asarray(off, dtype=np.int64)
        self.words = [[int(s) for s in sym[off[w]:off[w + 1]]] for w in range(off.size - 1)]
        self.freq = [int(f) for f in freq]

    def best(self):
        cnt = {}
        for w, f in zip(self.words, self.freq):
            for a, b in zip(w[:-1], w[1:]):
                cnt[(a, b)] = cnt.get((a, b), 0) + f
        if not cnt:
            return None
        top = max(cnt.values())
        return next((k + (top,)) for k, v in cnt.items() if v == top)  # dicts keep the order of first insertion

    def apply(self, l, r, m):
        for w in self.words:
            if len(w) < 2:
                continue
            out, i = [], 0
            while i < len(w):
                if i + 1 < len(w) and w[i] == l and w[i + 1] == r:
                    out.append(m)
                    i += 2
                else:
                    out.append(w[i])
                    i += 1
            w[:] = out

    def run(self, n, first_merged):
        log = []
        for i in range(n):
            b = self.best()
            if b is None:
                break
            self.apply(b[0], b[1], first_merged + i)
            log.append(b)
        return log

    def export(self):
        return csr(self.words, self.freq)


def oracle_walk(oracle, case, upto=None):
    """the oracle, one merge at a time: yields (k, (l, r, m, count), stream before merge k, merges 0..k) (ids from SYM_BASE)"""
    sym, off, freq = case.build()
    orc = oracle.OracleBPETrainer.from_words(sym, off, freq)
    for k in range(upto if upto is not None else case.merges):
        before = orc.export()[:2]
        if orc.run(10 ** 9, 1) < 1:
            return
        ids, cnt = orc.merge_ids()
        yield k, (int(ids[k][0]), int(ids[k][1]), int(ids[k][2]), int(cnt[k])), before, ids


_REF = {}


def reference(oracle, case):
    """the oracle's run of a case, computed once: merges (l, r, m), counts, the stream after each of case.checks, and the
    number of pairs that tie at the top of the input's histogram"""
    if case.name not in _REF:
        sym, off, freq = case.build()
        orc = oracle.OracleBPETrainer.from_words(sym, off, freq)
        states, done = {}, 0
        for c in sorted(set(case.checks) | {case.merges}):
            done += orc.run(10 ** 9, c - done)
            s, o, _ = orc.export()
            states[c] = (s.copy(), o.copy())
        ids, cnt = orc.merge_ids()
        for a in (sym, off, freq, ids, cnt):
            a.setflags(write=False)
        h0 = recount(sym, off, freq)
        top = max(h0.values())
        _REF[case.name] = {"input": (sym, off, freq), "ids": ids, "counts": cnt, "states": states,
                           "tied0": sum(1 for v in h0.values() if v == top)}
    return _REF[case.name]
