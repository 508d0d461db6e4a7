"""The device trainer (csrc/swt_bpe_train.hip) at its internal limits: every case of tests/train_seam_cases.py against the
CPU oracle on the pairs, the counts, the complete final stream and the whole pair histogram (a recount of the oracle's
stream weighted by the frequencies).  Exact integer equality, no tolerance.  Every case runs as ONE run() call, compared
after it, and in the odd slices (1, 2, 7, 64, 5, 300), which move the host round trips across the seam; only the sliced
run is also compared at the case's two or three intermediate points (a comparison in mid run needs a run call to end
there, and the one-call run is the one that has none).

Every case also asserts a witness that the far side of its seam ran: what the library reports (stats(), step_trace()) or a
property of the input shown from the oracle alone (tests/test_train_seam_inputs.py, whose docstring lists the cases with
their sizes and the merge at which each seam is crossed).

Value-only mutants of the trainer, built outside the tree one at a time and each run once on the MI355X against the
training tests there were before (test_gpu_parity.py::test_train_*, test_gpu_configs.py) and against this file
(72 tests).  "old" / "new": tests of either that fail.
  mutant                                         old (31 selected)                         new (72)
  drop `if (K > 1) EMIT(x, y, false)`            15 fail (plateaus, micro tie-breaks,      58 fail: every test_bpe_seam case but cand_2100, cand_8300,
                                                 5K / headline runs, sharded fast runs)    big_narrow, big_wide (one pair per step); the grow test; all
                                                                                           reuse and sharded tests.  WordPiece passes (one pair per step)
  drop the po_cov emit                           caught (6 of the first 8 had failed       70 fail: all but test_wordpiece_seams[long-fused / long-generic]
                                                 when the run reached its time limit)
  EMIT: sign flipped past kEmitCap               not run                                   26 fail: long_words, tie_staging, overflow_single, overflow_tied,
                                                                                           seg_of_65536; reuse[long_words, overflow_tied]; wordpiece[twin-*];
                                                                                           sharded[long_words, overflow_single, overflow_tied]
  big path: fw sign flipped into the LDS sums    not run                                   4 fail: big_narrow, big_wide (both runs): the summing rounds ran
  big path: fw sign flipped for left-over deltas not run                                   2 fail: big_wide (both runs), first difference at merge 7;
                                                                                           big_narrow passes: only big_wide leaves deltas without a slot
No mutant passes the new file.  DESIGN.md, "Trainer seams", has the same table with the old tests by name.
"""
import numpy as np
import pytest

from tests import train_seam_cases as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(native):
    if native.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests need an MI355X (there is no CPU fallback to test)")
    native.init(0)
    return native


def _to_device_ids(a, shift):
    a = np.asarray(a).astype(np.int64)
    return np.where(a >= T.SYM_BASE, a + shift, a)


def _hist_want(state, freq, shift):
    s, o = state
    return T.recount(_to_device_ids(s, shift), o, freq)


def _same_state(tr, state, freq, shift, where):
    gs, go, gf = tr.export()
    s, o = state
    assert np.array_equal(go, o), where
    assert np.array_equal(gs.astype(np.int64), _to_device_ids(s, shift)), where
    assert np.array_equal(gf, freq), where
    keys, cnts = tr.histogram()
    got = {int(k): int(c) for k, c in zip(keys, cnts)}
    assert len(got) == len(keys), where
    want = _hist_want(state, freq, shift)
    if got != want:
        bad = sorted(k for k in set(got) | set(want) if got.get(k) != want.get(k))[:5]
        raise AssertionError("%s: histogram differs at %s" % (where, [(hex(k), got.get(k), want.get(k)) for k in bad]))


def drive(dev, case, ref, slices):
    """run the case on the device, compare with the oracle; -> (trainer, stats() before the first and after every run call).
    slices None: ONE run call, compared after it; otherwise the slices, compared after each of case.checks as well."""
    sym, off, freq = ref["input"]
    ids, cnt = ref["ids"], ref["counts"]
    shift = case.first_merged - T.SYM_BASE
    tr = dev.BpeTrainer.from_words(sym, off, freq)
    n = case.merges
    marks = (n,) if slices is None else tuple(sorted(set(case.checks) | {n}))
    ls, rs, cs, stats = [], [], [], [tr.stats()]
    i = 0
    while len(ls) < n:
        stop = min(m for m in marks if m > len(ls))
        ask = stop - len(ls) if slices is None else min(slices[i % len(slices)], stop - len(ls))
        l, r, c = tr.run(ask, case.first_merged + len(ls))
        assert len(l) == ask, (case, slices, len(ls), ask, len(l))
        ls += l.tolist(); rs += r.tolist(); cs += c.tolist()
        stats.append(tr.stats())
        i += 1
        if len(ls) in marks:
            k = len(ls)
            got = np.stack([np.asarray(ls, dtype=np.int64), np.asarray(rs, dtype=np.int64)], axis=1)
            want = _to_device_ids(ids[:k, :2], shift)
            bad = np.nonzero((got != want).any(axis=1))[0]
            assert bad.size == 0, (case, slices, "first difference at merge", int(bad[0]), got[bad[0]].tolist(), want[bad[0]].tolist())
            assert np.array_equal(np.asarray(cs, dtype=np.uint64), cnt[:k]), (case, slices)
            _same_state(tr, ref["states"][k], freq, shift, (case, slices, k))
    return tr, stats


def step_sizes(tr):
    """merges per step, from the trace: the merges of one step log the same live-symbol count"""
    live = tr.step_trace()[:, 3]
    cut = np.flatnonzero(np.diff(live) != 0) + 1
    return np.diff(np.concatenate([[0], cut, [live.size]])).tolist()


def witness(case, tr, stats, slices, ref):
    st = stats[-1]
    slots = [x["table_slots"] for x in stats]
    tracerows = tr.step_trace()
    assert len(tracerows) == case.merges
    n_cand = tracerows[:, 2].astype(np.int64)
    if case.no_squeeze:
        assert st["squeezes"] == 0, "the stream was squeezed: the slot positions the case relies on moved"
    assert not (st["flags"] & 1), "the inverted index was abandoned"
    w = case.witness
    if w in ("tied_eq", "tied_shared"):
        n = int(case.name.rsplit("_", 1)[1]) * (2 if w == "tied_shared" else 1)
        assert int(tracerows[0][1]) == n, "pairs tied at the first merge"
        if slices is None and w == "tied_eq":
            sizes = step_sizes(tr)
            if n <= T.K_MAX_BATCH:
                assert sizes[0] == n
            elif n <= T.K_TIE_SET:
                assert sizes[0] == T.K_MAX_BATCH and max(sizes) == T.K_MAX_BATCH, "the plateau was not cut at kMaxBatch"
                if n <= 64:  # one trip of the tie scan covers every word: the rest follows in full steps
                    assert sizes[:-(-n // 16)] == [16] * (n // 16) + ([n % 16] if n % 16 else [])
            else:
                assert sizes[:n - T.K_TIE_SET] == [1] * (n - T.K_TIE_SET), "a plateau wider than the tie set takes one merge per step"
                assert max(sizes) > 1, "batching resumes once the plateau fits the set"
    elif w == "deltas_batch" and slices is None:
        assert step_sizes(tr)[0] == 2, "(P, Q) and (U, V) were not merged in one step"
    elif w == "deltas_single":
        assert int(tracerows[0][1]) == 1
    elif w == "cand_list":
        n = int(case.name.rsplit("_", 1)[1])
        assert int(tracerows[1][1]) == n, "pairs tied behind the first merge"
        assert st["replans"] >= 2, "the list did not run dry after the first merge"
        if n <= T.K_CAND_CAP // 2:  # (a wider plateau is not listed: theta = 0, full-table argmax)
            assert int(tracerows[:, 2].max()) > T.K_CAND_HIGH, "the candidate list never passed kCandHigh"
    elif w == "squeeze":
        assert st["squeezes"] >= 1, "the stream was never squeezed"
        assert slots[-1] > slots[0 if slices is None else 1], "the pair table was not resized (sliced: between two run calls)"
    elif w == "steps":
        assert st["steps"] > T.K_SEG_START
    elif w == "seg_of":
        # what the device holds, not what the case asked for: symbols on both sides of id 65,536 in its stream, index entries
        # logged for them, and the index still in use (the flag is checked above)
        gs = tr.export()[0].astype(np.int64) - T.SYM_BASE
        assert ((gs >= 0) & (gs < T.K_SEG_OF)).any() and (gs >= T.K_SEG_OF).any(), "no merged id beyond 65,536 in the device's stream"
        assert st["index_entries"] > 0
    elif w == "tie_beyond_512":
        # the tie scan ran over the staged words at the first merge, with a plateau the LDS set holds (use_set)
        n_tied = int(tracerows[0][1])
        assert 2 <= n_tied <= T.K_TIE_SET, n_tied
        assert n_tied == ref["tied0"], "the device saw another plateau than the recount of the input"
        assert stats[1]["tie_words"] > 0, "no tie scan covered a word"
    elif w == "big":
        # swt_bpe_train_stats' entries_scanned is the apply launches' n_ent, summed.  The first merge's list is the pair's
        # list of initial words (no tags: every entry matches), so every full row of 256 entries gives its workgroup 256
        # words in one trip: n_ent >= kBigMerge and 256 >= kBigWords make `big` true in n_ent / 256 trips at least.
        n_words = ref["input"][1].size - 1
        if slices is not None:  # the first call is one merge
            assert stats[1]["entries_scanned"] - stats[0]["entries_scanned"] == n_words >= T.K_BIG_MERGE + 256
        else:
            assert st["entries_scanned"] >= n_words >= T.K_BIG_MERGE + 256
        assert 256 >= T.K_BIG_WORDS
    elif w == "cand_grow":
        assert int(n_cand.max()) > T.K_CAND_HIGH, "pushes never took the list past kCandHigh"
        first = int(np.flatnonzero(n_cand > T.K_CAND_HIGH)[0])
        assert first > 4 and n_cand[first - 1] <= T.K_CAND_HIGH, "the list was listed long, not pushed long"


@pytest.mark.parametrize("sliced", [False, True], ids=["one_call", "slices"])
@pytest.mark.parametrize("case", T.CASES, ids=[c.name for c in T.CASES])
def test_bpe_seam(dev, oracle, case, sliced):
    ref = T.reference(oracle, case)
    assert len(ref["ids"]) == case.merges
    slices = T.SLICES if sliced else None
    tr, stats = drive(dev, case, ref, slices)
    try:
        witness(case, tr, stats, slices, ref)
    finally:
        tr.close()


def test_list_grows_inside_one_round_trip(dev, oracle):
    """cand_grow in three run calls: the second (120 merges, fewer than a round trip's 256 steps) begins with a list below
    kCandHigh, so the host does not re-plan, and pushes take it past 2,048 while the steps of that one trip are running:
    block_argmax and the tie launch take their strided loops, with pushes arriving.  No re-plan from the first call's end
    to the second's; the list only grows; the merges, counts, stream and histogram are the oracle's."""
    case = T.BY_NAME["cand_grow"]
    ref = T.reference(oracle, case)
    sym, off, freq = ref["input"]
    tr = dev.BpeTrainer.from_words(sym, off, freq)
    try:
        done, replans = 0, []
        for stop in T.GROW_CALLS:
            l, r, c = tr.run(stop - done, T.SYM_BASE + done)
            assert np.array_equal(np.stack([l, r], axis=1), ref["ids"][done:stop, :2]) and np.array_equal(c, ref["counts"][done:stop]), stop
            done = stop
            _same_state(tr, ref["states"][stop], freq, 0, ("cand_grow", stop))
            replans.append(tr.stats()["replans"])
        a, b = T.GROW_CALLS[0], T.GROW_CALLS[1]
        n_cand = tr.step_trace()[:, 2].astype(np.int64)
        print("cand_grow: replans after each call", replans, "n_cand at merges", a, b - 1, "=", int(n_cand[a]), int(n_cand[b - 1]))
        assert replans[1] == replans[0], "the host re-planned between the first call's end and the second's"
        assert n_cand[a] <= T.K_CAND_HIGH < n_cand[b - 1], (int(n_cand[a]), int(n_cand[b - 1]))
        assert (np.diff(n_cand[a:b]) >= 0).all() and int((n_cand[a:b] > T.K_CAND_HIGH).sum()) >= 2, "the list was rebuilt in mid call"
        assert replans[2] > replans[1], "a list past kCandHigh is re-planned at the next round trip"
    finally:
        tr.close()


# ---------------------------------------------------------------------------------------------------------------- id reuse

@pytest.mark.parametrize("name", T.REUSE)
def test_reused_ids_stepwise_and_run(dev, oracle, name):
    """a merged id that already names a live symbol (kFlagIndexBroken: applies scan every word, the tie scans read the
    stream): 30 merges against the recount model, through best()/apply() and through run()"""
    sym, off, freq = T.reference(oracle, T.BY_NAME[name])["input"]
    base = sorted(set(sym.tolist()))
    # stepwise: merges 0..4 take fresh ids, then every id names a live symbol -- an initial one, or an earlier merge's
    tr = dev.BpeTrainer.from_words(sym, off, freq)
    model = T.RecountModel(sym, off, freq)
    for i in range(30):
        l, r, c, tied, pos = tr.best()
        want = model.best()
        assert (l, r, c) == want, (name, i)
        live = sorted({s for w in model.words for s in w})
        m = T.SYM_BASE + i if i < 5 else (live[(i * 7) % len(live)] if i % 2 else T.SYM_BASE + (i % 5))
        tr.apply(l, r, m)
        model.apply(l, r, m)
        if i % 10 == 9:
            _same_state(tr, model.export()[:2], freq, 0, (name, "stepwise", i))
    assert tr.stats()["flags"] & 1
    tr.close()
    # run(): the second call starts at ids the first one made, the third at initial symbols
    tr = dev.BpeTrainer.from_words(sym, off, freq)
    model = T.RecountModel(sym, off, freq)
    done = 0
    for ask, first in ((6, T.SYM_BASE), (9, T.SYM_BASE + 2), (15, base[0])):
        l, r, c = tr.run(ask, first)
        want = model.run(ask, first)
        assert list(zip(l.tolist(), r.tolist(), c.tolist())) == want, (name, done)
        done += ask
        _same_state(tr, model.export()[:2], freq, 0, (name, "run", done))
    assert tr.stats()["flags"] & 1
    tr.close()


# ---------------------------------------------------------------------------------------------------------------- WordPiece

@pytest.mark.parametrize("generic", [False, True], ids=["fused", "generic"])
@pytest.mark.parametrize("kind", T.WP_KINDS)
def test_wordpiece_seams(swt, dev, oracle, monkeypatch, kind, generic):
    """the long-word, delta-overflow and twin-pair shapes through NaiveWP.train (apply_body is shared): merge order, final
    stream and frequencies against OracleWPTrainer, with the fused step kernel and with the generic four launches"""
    if generic:
        monkeypatch.setenv("SWT_WP_GENERIC", "1")
    else:
        monkeypatch.delenv("SWT_WP_GENERIC", raising=False)
    corpus = T.wp_sentences(kind)
    base = oracle.OracleWPTrainer(corpus).vocab_size
    for extra in (5, 40):
        o = oracle.OracleWPTrainer(corpus)
        o.run(base + extra)
        m = swt.NaiveWP()
        m.train(list(corpus), base + extra)
        assert [tuple(p) for p in m._merge_order] == [tuple(p) for p in o.merges_list], (kind, extra)
        # the host's whole condition for the fused step, beside the variable: every live pair listed, a list of at most
        # kWpStepList entries (one launch sequence per merge either way)
        st = m._trainer.stats()
        assert st["theta"] == 1 and 0 < st["candidates"] <= T.K_WP_STEP_LIST and st["steps"] >= extra, (kind, extra, st)
        syms, woff, freq = o.export()
        got = m.corpus_as_symbols
        assert len(got) == len(woff) - 1
        for w in range(len(got)):
            assert got[w][0] == [o.symbol(int(x)) for x in syms[int(woff[w]):int(woff[w + 1])]] and got[w][1] == int(freq[w]), (kind, w)


# ---------------------------------------------------------------------------------------------------------------- sharded

def _rank0_live_before(sym, off, n_words0, ids):
    """live symbols in the first n_words0 words before every merge of `ids` (l, r, m): the recount model on rank 0's words"""
    model = T.RecountModel(sym[:int(off[n_words0])], off[:n_words0 + 1], [1] * n_words0)
    live = []
    for l, r, m in np.asarray(ids).tolist():
        live.append(sum(len(w) for w in model.words))
        model.apply(l, r, m)
    return live


_SHARDED_FAST = [pytest.param(n, c, False, id="%s-%s" % (n, c)) for n in T.SHARDED for c in T.SHARDED_ONLY.get(n, tuple(T.SHARDED_CUTS))]
_SHARDED_GENERIC = [pytest.param(n, c, True, id="%s-%s-generic" % (n, c)) for n, c in T.SHARDED_GENERIC]


@pytest.mark.parametrize("name,cut,generic", _SHARDED_FAST + _SHARDED_GENERIC)
def test_sharded_seams(dev, oracle, monkeypatch, name, cut, generic):
    """the same words cut into 2 and 3 contiguous ranges (one of them empty) through the loop-back communicator: the fast
    form, and for the smallest tied inputs the forced one-merge-per-step form as well"""
    monkeypatch.setenv("SWT_DIST_GENERIC", "1" if generic else "0")
    cuts = T.SHARDED_CUTS[cut]
    case = T.BY_NAME[name]
    ref = T.reference(oracle, case)
    sym, off, freq = ref["input"]
    n_words = off.size - 1
    edges = [0] + [int(c * n_words) for c in cuts] + [n_words]
    comm = dev.Dist.loopback(len(edges) - 1)
    trainers = []
    try:
        for lo, hi in zip(edges[:-1], edges[1:]):
            o = off[lo:hi + 1] - off[lo]
            trainers.append(dev.BpeTrainer.from_words(sym[int(off[lo]):int(off[hi])], o, freq[lo:hi]))
        comm.shard_begin(trainers)
        l, r, c = comm.run(trainers, case.merges, T.SYM_BASE)
        got = np.stack([l, r], axis=1)
        bad = np.nonzero((got != ref["ids"][:, :2]).any(axis=1))[0] if len(l) == case.merges else np.array([len(l)])
        assert bad.size == 0, (name, cuts, "first difference at merge", int(bad[0]))
        assert np.array_equal(c, ref["counts"])
        s_want, o_want = ref["states"][case.merges]
        h_want = T.recount(s_want, o_want, freq)
        for t, lo, hi in zip(trainers, edges[:-1], edges[1:]):
            gs, go, gf = t.export()
            assert np.array_equal(go, o_want[lo:hi + 1] - o_want[lo]), (name, cuts, lo)
            assert np.array_equal(gs, s_want[int(o_want[lo]):int(o_want[hi])]), (name, cuts, lo)
            assert np.array_equal(gf, freq[lo:hi]), (name, cuts, lo)
            keys, cnts = t.histogram()  # every rank keeps the histogram of the whole corpus
            assert {int(k): int(v) for k, v in zip(keys, cnts)} == h_want, (name, cuts, lo)
        # the fast form carried several merges in one step (K > 1 in fast_apply_sharded_kernel).  Every trainer's trace is
        # rank 0's log, whose last column is rank 0's live symbols when the step began.  Rows that differ there belong to
        # different steps; rows that agree belong to one step if that step's first pair occurs in rank 0's words, because
        # the step then took symbols from rank 0 and every later step logs fewer.
        if generic:
            # every step size is 1: row k logs rank 0's live symbols before merge k itself, where a step of several merges
            # logs the count it began with in all its rows.  (step_sizes() cannot say it: two rows agree here whenever the
            # merge between them left rank 0's words alone, so the rows are held against the recount model of those words.)
            live = trainers[0].step_trace()[:, 3].astype(np.int64).tolist()
            want = _rank0_live_before(sym, off, edges[1], ref["ids"])
            assert want[0] > want[-1] and live == want, (name, cut, live[:8], want[:8])
        elif name == "cand_8300":
            for t in trainers:  # the re-plan behind the first merge listed nothing: generic steps inside the fast runner
                st = t.stats()
                assert st["theta"] == 0 and st["replans"] >= 2, (name, cut, st)
        elif edges[1] > 0 and name in ("overflow_tied", "plateau_17", "plateau_257"):
            row = 1 if name == "plateau_257" else 0  # a plateau wider than the tie set opens with a single merge
            key = (int(ref["ids"][row][0]) << 32) | int(ref["ids"][row][1])
            assert key in T.pair_keys(sym[:int(off[edges[1]])], off[:edges[1] + 1])[0].tolist(), "rank 0 does not hold the step's first pair"
            sizes = step_sizes(trainers[0])
            assert sizes[:row] == [1] * row and sizes[row] > 1, (name, cuts, sizes[:4])
    finally:
        for t in trainers:
            t.close()
        comm.close()
