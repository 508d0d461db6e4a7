"""The inputs of tests/test_gpu_train_seams.py, checked without a GPU: for every case of tests/train_seam_cases.py the
oracle alone shows that the input crosses the seam it names, the sizes are what the case table says, and the recount model
of the id-reuse test agrees with the oracle where no id is reused.

Cases as printed by test_case_crosses_its_seam (-s); '@k' is the merge at which the oracle first shows the property:

long_words kStage words 2696 symbols 7789 merges 60
    pair on both sides of slot 24 @0; pair on both sides of slot 48 @0; word of more than 72 slots @0; window
    begins on a hole @1; window of holes to the word's end @43; live slots after the last merge: 76 % @60
tie_staging kTieStage*64 words 435 symbols 15213 merges 170
    live slots after the last merge: 98 % @170
overflow_single kEmitCap,kFlushBatch words 35 symbols 408 merges 60
    8 deltas @0; 6 deltas @0; 4 deltas @0; 12 deltas+ @0; 10 deltas @0; 2 deltas @1; twin run of 4 @3; twin run of
    5 @3
overflow_tied kEmitCap,kFlushBatch words 37 symbols 414 merges 60
    10 deltas @0; 8 deltas @0; 6 deltas @0; 12 deltas+ @0; 11 deltas @0; 9 deltas @0; 1 deltas @0; 5 deltas @0; 4
    deltas @1; 2 deltas @2; twin run of 4 @4; twin run of 5 @4
plateau_15 kMaxBatch words 30 symbols 90 merges 40
    tied at merge 0: 15 @0; tied pairs share no symbol @0; first-position order is not key order @0
plateau_16 kMaxBatch words 32 symbols 96 merges 40
    tied at merge 0: 16 @0; tied pairs share no symbol @0; first-position order is not key order @0
plateau_17 kMaxBatch words 34 symbols 102 merges 45
    tied at merge 0: 17 @0; tied pairs share no symbol @0; first-position order is not key order @0
plateau_33 kMaxBatch words 66 symbols 198 merges 80
    tied at merge 0: 33 @0; tied pairs share no symbol @0; first-position order is not key order @0
plateau_255 kTieSet words 510 symbols 1530 merges 400
    tied at merge 0: 255 @0; tied pairs share no symbol @0; first-position order is not key order @0
plateau_256 kTieSet words 512 symbols 1536 merges 400
    tied at merge 0: 256 @0; tied pairs share no symbol @0; first-position order is not key order @0
plateau_257 kTieSet words 514 symbols 1542 merges 400
    tied at merge 0: 257 @0; tied pairs share no symbol @0; first-position order is not key order @0
plateau_600 kTieSet words 1200 symbols 3600 merges 700
    tied at merge 0: 600 @0; tied pairs share no symbol @0; first-position order is not key order @0
plateau_shared_40 kMaxBatch (dangerous pairs) words 40 symbols 120 merges 80
    tied at merge 0: 80 @0; tied pairs share a symbol @0; first-position order is not key order @0
cand_2100 kCandHigh, list dry words 7200 symbols 24600 merges 60
    tied at merge 0: 1 @0; tied pairs share no symbol @0; tied at merge 1: 2100 @1; pairs below the plateau: 10200
    @1
cand_8300 kCandCap, list dry words 19600 symbols 61800 merges 40
    tied at merge 0: 1 @0; tied pairs share no symbol @0; tied at merge 1: 8300 @1; pairs below the plateau: 22600
    @1
cand_grow kCandHigh (pushes in mid trip) words 1700 symbols 4400 merges 300
    listed at the first re-plan: 1004 (theta 4, 1200 pairs below) @0; listed or pushed before merge 60: 2032 @60; list
    past kCandHigh by pushes @93
big_narrow kBigMerge,kBigWords words 20000 symbols 80000 merges 12
    words of the first merge: 20000 @0; distinct old neighbour pairs: 6 @0; distinct keys (old + new) per 256
    consecutive words, least: 12 @0
big_wide kBigMerge,kBigWords,kAggSlots words 20000 symbols 80000 merges 30
    words of the first merge: 20000 @0; distinct old neighbour pairs: 1400 @0; distinct keys (old + new) per 256
    consecutive words, least: 828 @0
squeeze_resize squeeze_stream, table_resize words 4000 symbols 22073 merges 500
    live slots after the last merge: 38 % @500
seg_of_65536 seg_of words 2696 symbols 7789 merges 60
    pair on both sides of slot 24 @0; pair on both sides of slot 48 @0; word of more than 72 slots @0; window
    begins on a hole @1; window of holes to the word's end @43; live slots after the last merge: 76 % @60
seg_start_4096 seg_start words 3000 symbols 16493 merges 5400
"""
import numpy as np
import pytest

from tests import train_seam_cases as T


def _words(sym, off):
    off = np.asarray(off, dtype=np.int64)
    return [sym[off[w]:off[w + 1]] for w in range(off.size - 1)]


def _has_pair(seq, l, r):
    return bool(((seq[:-1] == l) & (seq[1:] == r)).any()) if seq.size > 1 else False


def _tied_at_top(sym, off, freq):
    h = T.recount(sym, off, freq)
    top = max(h.values())
    return top, [k for k, v in h.items() if v == top]


def crossing(oracle, case):
    """-> {property: merge at which the oracle's run first shows it}; the caller asserts the ones the case needs"""
    seen = {}
    ref = T.reference(oracle, case)
    sym0, off0, freq = ref["input"]
    w = case.witness
    if w in ("stage_refill", "seg_of"):
        for k, (l, r, m, c), (s, o), ids in T.oracle_walk(oracle, case):
            slot, ln, word = T.slot_offsets(s, o, T.sym_lengths(ids[:k]))
            hit = np.flatnonzero((s[:-1] == l) & (s[1:] == r) & (word[:-1] == word[1:]))
            for wd in np.unique(word[hit]):
                at = slot[hit[word[hit] == wd]]
                lo, hi = int(o[wd]), int(o[wd + 1])
                n_slots = int(slot[hi - 1] + ln[hi - 1])
                if at.min() < T.K_STAGE <= at.max():
                    seen.setdefault("pair on both sides of slot 24", k)
                if at.min() < 2 * T.K_STAGE <= at.max():
                    seen.setdefault("pair on both sides of slot 48", k)
                if n_slots > 3 * T.K_STAGE:
                    seen.setdefault("word of more than 72 slots", k)
                if n_slots > T.K_STAGE and T.K_STAGE not in slot[lo:hi].tolist():
                    seen.setdefault("window begins on a hole", k)
                if ln[hi - 1] > T.K_STAGE:
                    seen.setdefault("window of holes to the word's end", k)
    elif w in ("deltas_single", "deltas_batch"):
        for k, (l, r, m, c), (s, o), ids in T.oracle_walk(oracle, case):
            pairs = [(l, r)]
            if w == "deltas_batch" and k == 0:
                pairs.append((T.PLANT0 + 2, T.PLANT0 + 3) if l == T.PLANT0 else (T.PLANT0, T.PLANT0 + 1))
            for seq in _words(s, o):
                d = T.walk_deltas(seq, pairs)
                if d:
                    seen.setdefault("%d deltas%s" % (min(d, 12), "+" if d >= 12 else ""), k)
                if _has_pair(seq, l, r) and l == r and seq.size in (4, 5) and len(set(seq.tolist())) == 1:
                    seen.setdefault("twin run of %d" % seq.size, k)
    elif w in ("tied_eq", "tied_shared", "cand_list"):
        top, tied = _tied_at_top(sym0, off0, freq)
        seen["tied at merge 0: %d" % len(tied)] = 0
        syms = [x for k in tied for x in (k >> 32, k & 0xFFFFFFFF)]
        seen["tied pairs share %s symbol" % ("a" if len(set(syms)) < len(syms) else "no")] = 0
        if sorted(tied) != tied:
            seen["first-position order is not key order"] = 0
        if w == "cand_list":
            s, o = T.reference(oracle, T.Case("_head_" + case.name, "", case.build, 1, "", checks=(1,)))["states"][1]
            h = T.recount(s, o, freq)
            top1, tied1 = _tied_at_top(s, o, freq)
            seen["tied at merge 1: %d" % len(tied1)] = 1
            seen["pairs below the plateau: %d" % sum(1 for v in h.values() if v < top1)] = 1
    elif w == "big":
        l, r = int(ref["ids"][0][0]), int(ref["ids"][0][1])
        words = _words(sym0, off0)
        holds = [i for i, seq in enumerate(words) if _has_pair(seq, l, r)]
        seen["words of the first merge: %d" % len(holds)] = 0
        nb = {(int(q[0]), l) for q in words} | {(r, int(q[3])) for q in words}
        seen["distinct old neighbour pairs: %d" % len(nb)] = 0
        blk = [len({(int(q[0]), l) for q in words[i:i + 256]} | {(r, int(q[3])) for q in words[i:i + 256]}) for i in range(0, len(words) - 255, 256)]
        seen["distinct keys (old + new) per 256 consecutive words, least: %d" % (2 * min(blk))] = 0
    elif w == "cand_grow":
        # what a re-plan of the input lists (whole count buckets from the top while at most kCandTarget pairs pass), then
        # every pair that reaches that threshold later: it is pushed, and nothing leaves the list before the next re-plan
        h = T.recount(sym0, off0, freq)
        by_count = sorted(set(h.values()), reverse=True)
        theta = by_count[0]
        for c in by_count[1:]:
            if sum(1 for v in h.values() if v >= c) > T.K_CAND_TARGET:
                break
            theta = c
        listed = {k for k, v in h.items() if v >= theta}
        seen["listed at the first re-plan: %d (theta %d, %d pairs below)" % (len(listed), theta, len(h) - len(listed))] = 0
        for k, (l, r, m, c), (s, o), ids in T.oracle_walk(oracle, case):
            listed |= {key for key, v in T.recount(s, o, freq).items() if v >= theta}
            if k == T.GROW_CALLS[0]:
                seen["listed or pushed before merge %d: %d" % (k, len(listed))] = k
            if len(listed) > T.K_CAND_HIGH:
                seen["list past kCandHigh by pushes"] = k
                break
    elif w == "squeeze":
        live = ref["states"][case.merges][0].size / sym0.size
        seen["live slots after the last merge: %.0f %%" % (100 * live)] = case.merges
    if case.no_squeeze:
        live = ref["states"][case.merges][0].size / sym0.size
        assert live >= 0.7, (case, live)
        seen["live slots after the last merge: %.0f %%" % (100 * live)] = case.merges
    return seen


NEEDS = {
    "stage_refill": ("pair on both sides of slot 24", "pair on both sides of slot 48", "word of more than 72 slots", "window begins on a hole",
                     "window of holes to the word's end"),
    "seg_of": ("pair on both sides of slot 24",),
    "deltas_single": ("6 deltas", "8 deltas", "10 deltas", "12 deltas+", "twin run of 4", "twin run of 5"),
    "deltas_batch": ("9 deltas", "10 deltas", "11 deltas", "12 deltas+"),
}


@pytest.mark.parametrize("case", T.CASES, ids=[c.name for c in T.CASES])
def test_case_crosses_its_seam(oracle, case):
    ref = T.reference(oracle, case)
    sym, off, freq = ref["input"]
    assert len(ref["ids"]) == case.merges, "the corpus is exhausted before the case ends"
    assert sym.size < 100_000 and int(sym.max()) < T.SYM_BASE and int(freq.min()) >= 1
    seen = crossing(oracle, case)
    print("%-18s %-30s words %6d symbols %6d merges %5d | %s" % (case.name, case.seam, off.size - 1, sym.size, case.merges,
                                                               "; ".join("%s @%d" % kv for kv in seen.items())))
    for need in NEEDS.get(case.witness, ()):
        assert need in seen, (case, need, sorted(seen))
    w = case.witness
    if w in ("tied_eq", "tied_shared", "cand_list"):
        n = int(case.name.rsplit("_", 1)[1])
        assert w == "cand_list" or "first-position order is not key order" in seen
        if w == "tied_eq":
            assert "tied at merge 0: %d" % n in seen and "tied pairs share no symbol" in seen
        elif w == "tied_shared":
            assert "tied at merge 0: %d" % (2 * n) in seen and "tied pairs share a symbol" in seen
        else:
            assert "tied at merge 0: 1" in seen and "tied at merge 1: %d" % n in seen
            assert any(k.startswith("pairs below the plateau") and int(k.split(": ")[1]) >= 3000 for k in seen)
    elif w == "big":
        n_words = off.size - 1
        assert "words of the first merge: %d" % n_words in seen and n_words >= T.K_BIG_MERGE + T.K_BIG_WORDS * 64
        nb = next(int(k.split(": ")[1]) for k in seen if k.startswith("distinct old"))
        per = next(int(k.split(": ")[1]) for k in seen if k.startswith("distinct keys"))
        if case.name == "big_wide":
            assert 2 * nb > T.K_AGG_SLOTS and per > T.K_AGG_SLOTS // 2
        else:
            assert 2 * nb <= 16
    elif w == "squeeze":
        assert ref["states"][case.merges][0].size * 10 < sym.size * 7
    elif w == "cand_grow":
        first = next(k for k in seen if k.startswith("listed at the first"))
        n0, theta = int(first.split(": ")[1].split(" ")[0]), int(first.split("theta ")[1].split(",")[0])
        assert n0 <= T.K_CAND_TARGET and theta > 1 and int(first.split(", ")[1].split(" ")[0]) >= 1000
        before = next(int(k.split(": ")[1]) for k in seen if k.startswith("listed or pushed before"))
        assert before <= T.K_CAND_HIGH, "the second run call of the device test would begin with a re-plan"
        # ... and passes it well inside the second call, which is shorter than a round trip (256 steps)
        assert T.GROW_CALLS[0] + 8 <= seen["list past kCandHigh by pushes"] <= T.GROW_CALLS[1] - 8 and T.GROW_CALLS[1] - T.GROW_CALLS[0] < 256
    elif w == "steps":
        assert case.merges > T.K_SEG_START
    elif w == "seg_of":
        assert case.first_merged - T.SYM_BASE < T.K_SEG_OF < case.first_merged - T.SYM_BASE + case.merges


def test_tie_staging_places():
    """every place of a wave's 16 words holds a 500-530 slot word once; around it the words start inside the staged 512
    slots, straddle their end or lie beyond it; tied pairs begin on both sides of slot 512 of their group"""
    sym, off, freq = T.tie_staging()
    off = off.astype(np.int64)
    n_groups = 17
    places, kinds, far = set(), set(), 0
    planted = (sym >= T.PLANT0) & (sym < T.FILL0)
    for g in range(n_groups):
        lo = off[16 * g]
        for i in range(16):
            b0, b1 = off[16 * g + i] - lo, off[16 * g + i + 1] - lo
            if b1 - b0 >= 500:
                places.add(i)
                assert b1 - b0 <= 530 or b1 - b0 == 1100
            kinds.add("inside" if b1 <= T.K_TIE_SLOTS else "straddles" if b0 < T.K_TIE_SLOTS else "beyond")
        at = np.flatnonzero(planted[lo:off[16 * g + 16]])
        far += int((at >= T.K_TIE_SLOTS).sum())
        assert (at < T.K_TIE_SLOTS).any()
    assert places == set(range(16)) and kinds == {"inside", "straddles", "beyond"} and far >= 2 * n_groups
    assert int((np.diff(off) == 1100).sum()) == 1
    h = T.recount(sym, off, freq)
    assert max(h.values()) == 2 and 2 <= sum(1 for v in h.values() if v == 2) <= T.K_TIE_SET


@pytest.mark.parametrize("name", T.REUSE + ("overflow_single", "plateau_shared_40"))
def test_recount_model_agrees_with_oracle(oracle, name):
    case = T.BY_NAME[name]
    ref = T.reference(oracle, case)
    sym, off, freq = ref["input"]
    n = min(case.merges, 45)
    model = T.RecountModel(sym, off, freq)
    log = model.run(n, T.SYM_BASE)
    assert [(l, r) for l, r, c in log] == [tuple(x) for x in ref["ids"][:n, :2].tolist()]
    assert [c for l, r, c in log] == ref["counts"][:n].tolist()
    if n == case.merges:
        s, o, _ = model.export()
        assert np.array_equal(s, ref["states"][n][0]) and np.array_equal(o, ref["states"][n][1])


def test_wordpiece_sentences_cross_the_seams(oracle):
    for kind in T.WP_KINDS:
        corpus = T.wp_sentences(kind)
        o = oracle.OracleWPTrainer(corpus)
        base = o.vocab_size
        syms, woff, _ = o.export()
        longest = int(np.diff(woff.astype(np.int64)).max())
        assert longest > (T.K_STAGE if kind != "overflow" else 12), (kind, longest)
        assert o.run(base + 40) == 40, kind
        if kind == "twin":
            ids, _ = o.merge_ids()
            assert any(l == r for l, r, m in ids.tolist())
