"""Sentence-pair batches on the device (csrc/swt_batch.hip): swt_batch_pair_plan / swt_batch_pair_rows, host and `_dev` forms, and
encode_batch(texts, text_pairs=...) of the four classes, against the Python model of tests/pair_cases.py (itself held to the
`tokenizers` wheel's recorded output by tests/test_pair_cases.py).  Every output is pre-filled with garbage and fenced by
sentinel bytes; the `_dev` runs use torch tensors on a side stream."""
import ctypes as C

import numpy as np
import pytest

from tests import batch_cases as B
from tests import pair_cases as P
from tests.test_gpu_model_batches import GARBAGE, Fenced, _to_numpy, _tokenizer
from tests.test_gpu_model_batches import run as run_single

pytestmark = pytest.mark.gpu

FIRST, SECOND, LONGEST = P.ONLY_FIRST, P.ONLY_SECOND, P.LONGEST_FIRST
COLUMNS = {"ids": "input_ids", "mask": "attention_mask", "type": "token_type_ids", "special": "special_tokens_mask", "seq": "sequence_ids",
           "spans": "offset_mapping", "word": "word_ids", "sample": "sample", "len": "length"}


@pytest.fixture(scope="module")
def dev(native):
    if native.device_count() < 1:
        pytest.fail("no HIP device")
    native.init(0)
    return native


@pytest.fixture(scope="module")
def caps(dev):
    return dev.batch_pair_capacity()


def run(dev, form, ids, off_a, off_b, s, strategy, cmap=None, pay=None, rows_cap=None, front=32, extras=True, want=None):
    """swt_batch_pair_plan + swt_batch_pair_rows in one form -> (rc, dict of the rows written, raw bodies).  cmap = (map or None,
    n_map, flagged).  extras: out_type, out_special, out_seq, out_sample, out_len and info are given.  want: the model's result;
    the plan is held to its row_base, status, longest and refused.  The outputs have room for rows_cap rows (default: the rows
    needed); what lies behind the rows written must still be garbage."""
    table, n_map, flagged = (None, 1 << 31, False) if cmap is None else cmap
    n_rows = int(off_a.size) - 1
    spec = P.native_spec(dev, s)
    width, idb = s["width"], 8 if s["ids64"] else 4
    lib = dev.lib()
    if form == "host":
        row_base, status, pinfo = dev.batch_pair_plan(off_a, off_b, spec, strategy)
    else:
        import torch
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt).copy()).cuda()
        stream = torch.cuda.Stream()
        d_a, d_b = up(off_a, np.int64), up(off_b, np.int64)
        d_base = torch.full((n_rows + 1 + 2,), -1, dtype=torch.int64, device="cuda")
        d_status = torch.full((n_rows + 8,), 0x77, dtype=torch.uint8, device="cuda")
        d_pinfo = torch.full((5 + 2,), -1, dtype=torch.int64, device="cuda")
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            dev.check(lib.swt_batch_pair_plan_dev(d_a.data_ptr(), d_b.data_ptr(), n_rows, C.byref(spec), strategy, d_base.data_ptr(),
                                                  d_status.data_ptr(), d_pinfo.data_ptr(), stream.cuda_stream))
        stream.synchronize()
        hb, hs, hi = d_base.cpu().numpy(), d_status.cpu().numpy(), d_pinfo.cpu().numpy()
        assert (hb[n_rows + 1:] == -1).all() and (hs[n_rows:] == 0x77).all() and (hi[5:] == -1).all()
        row_base, status, pinfo = hb[:n_rows + 1].view(np.uint64), hs[:n_rows], hi[:5].view(np.uint64)
    need = int(row_base[-1])
    if want is not None:
        assert row_base.tolist() == want["row_base"].tolist() and status.tolist() == want["status"].tolist()
        assert pinfo.tolist() == [need, want["longest"], 0, want["refused"], 0]
    if rows_cap is None:
        rows_cap = need
    slots = rows_cap * width
    outs = {"ids": Fenced(slots * idb, front), "mask": Fenced(slots, front), "type": Fenced(slots * idb, front), "special": Fenced(slots, front),
            "seq": Fenced(slots, front), "spans": Fenced(slots * 8, front), "word": Fenced(slots * 4, front),
            "sample": Fenced(rows_cap * 4, front), "len": Fenced(rows_cap * 4, front), "info": Fenced(40, 32)}
    use = {k: extras for k in outs}
    use.update({"ids": True, "mask": True, "spans": pay is not None, "word": pay is not None})
    spans = word = None
    if pay is not None:
        spans, word = P.flat_payloads(pay)
    windows = s["windows"]
    order = ("ids", "mask", "type", "special", "seq", "spans", "word", "sample", "len", "info")
    if form == "host":
        p = {k: (C.c_void_p(o.host_ptr()) if use[k] else None) for k, o in outs.items()}
        types = {"mask": dev.u8p, "special": dev.u8p, "spans": dev.u32p, "word": dev.u32p, "sample": dev.u32p, "len": dev.u32p, "info": dev.u64p}
        args = [C.cast(p[k], types[k]) if k in types and p[k] is not None else p[k] for k in order]
        cast = lambda a, t: a.ctypes.data_as(t) if a is not None and a.size else None
        rc = lib.swt_batch_pair_rows(cast(ids, dev.u32p), cast(off_a, dev.u64p), cast(off_b, dev.u64p), n_rows, cast(table, dev.u32p), n_map,
                                     int(flagged), cast(spans, dev.u32p), cast(word, dev.u32p), C.byref(spec), strategy,
                                     cast(row_base, dev.u64p) if windows else None, cast(np.ascontiguousarray(status), dev.u8p), rows_cap, *args)
    else:
        pad4 = lambda a: np.concatenate([a, np.zeros(4, a.dtype)])
        d_ids = up(pad4(ids), np.int32)
        d_map = up(pad4(table), np.int32) if table is not None else None
        d_spans = up(pad4(spans.reshape(-1)), np.int32) if pay is not None else None
        d_word = up(pad4(word), np.int32) if pay is not None else None
        d_rb = up(row_base, np.int64)
        p = {k: (o.to_device(torch) if use[k] else None) for k, o in outs.items()}
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            rc = lib.swt_batch_pair_rows_dev(d_ids.data_ptr(), d_a.data_ptr(), d_b.data_ptr(), n_rows,
                                             d_map.data_ptr() if d_map is not None else None, n_map, int(flagged),
                                             d_spans.data_ptr() if pay is not None else None, d_word.data_ptr() if pay is not None else None,
                                             C.byref(spec), strategy, d_rb.data_ptr() if windows else None, d_status.data_ptr(), rows_cap,
                                             *[p[k] for k in order], stream.cuda_stream)
        stream.synchronize()
    if rc == dev.ERR_CAPACITY:
        return rc, {"info": outs["info"].body(np.uint64)}, outs
    dev.check(rc)
    done = min(need, rows_cap)
    dtypes = {"ids": np.int64 if s["ids64"] else np.int32, "mask": np.uint8, "type": np.int64 if s["ids64"] else np.int32, "special": np.uint8,
              "seq": np.int8, "spans": np.uint32, "word": np.int32, "sample": np.uint32, "len": np.uint32, "info": np.uint64}
    body = {k: outs[k].body(dtypes[k]) for k in outs}
    per_row = {"ids": width, "mask": width, "type": width, "special": width, "seq": width, "spans": 2 * width, "word": width, "sample": 1, "len": 1}
    res = {}
    for k, n in per_row.items():
        garbage = np.frombuffer(bytes([GARBAGE]) * body[k].itemsize, dtype=body[k].dtype)[0]
        if use[k]:
            assert (body[k][done * n:] == garbage).all(), "%s: a row at or beyond the capacity was written" % k
            shape = (done, width, 2) if k == "spans" else (done, width) if n > 1 or k not in ("sample", "len") else (done,)
            res[COLUMNS[k]] = body[k][:done * n].reshape(shape)
        else:
            assert (body[k] == garbage).all(), "%s was not given and was written" % k
    if extras:
        res["info"] = body["info"]
    else:
        assert (body["info"] == np.frombuffer(bytes([GARBAGE]) * 8, dtype=np.uint64)[0]).all()
    return rc, res, outs


def agree(res, want, rows=None, info=True):
    rows = want["input_ids"].shape[0] if rows is None else rows
    for k in COLUMNS.values():
        if k not in res:
            continue
        assert res[k].shape[0] == rows, k
        if not np.array_equal(res[k], want[k][:rows]):
            bad = np.argwhere(np.asarray(res[k]) != np.asarray(want[k][:rows]))[0]
            raise AssertionError("%s differs first at %s: %r != %r" % (k, bad.tolist(), res[k][tuple(bad)], want[k][:rows][tuple(bad)]))
    if info and "info" in res:
        assert res["info"].tolist() == [rows, want["longest"], want["n_unknown"], want["refused"], want["lost"]]


def both_ways(dev, form, lengths, seed, s, strategy, cmap=None, payloads=True, front=32, extras=True, cont=False):
    rows_a, rows_b, ids, off_a, off_b, pay = P.pair_stream(lengths, seed, cont=cont)
    pay = pay if payloads else None
    want = P.expected_pair_batch(rows_a, rows_b, s, strategy, cmap, pay)
    _, res, _ = run(dev, form, ids, off_a, off_b, s, strategy, cmap, pay, front=front, extras=extras, want=want)
    agree(res, want)
    return want


@pytest.mark.parametrize("form", ["host", "dev"])
def test_every_recorded_geometry(dev, golden, form):
    """the widths, strides, strategies and padding sides of tests/golden/pair_batches.json, all 81 pairs of a geometry in one
    call, windowed and truncating: the arrays of the device against the model that test_pair_cases holds to the wheel"""
    recorded = golden("pair_batches.json")
    n = recorded["n_max"] + 1
    lengths = [(na, nb) for na in range(n) for nb in range(n)]
    some_refused = 0
    for case, key in enumerate(recorded["cases"]):
        width, stride, strategy, left, specials = (int(x) for x in key.split(","))
        for windows in ([False] if strategy == LONGEST else [True, False]):
            s = P.spec(width, stride, windows, bool(left), False, 0, 1, 2 if specials else None, 3 if specials else None)
            want = both_ways(dev, form, lengths, 100 + case, s, strategy, payloads=bool(case & 1))
            some_refused += want["refused"]
            if windows:  # refused exactly where the wheel raised
                assert [int(x) for x in want["status"]] == [int(e == "E") for e in recorded["cases"][key]]
    assert some_refused > 1000


@pytest.mark.parametrize("width", [6, 9, 63, 64, 65, 129, 4 * 64 + 4])
@pytest.mark.parametrize("form", ["host", "dev"])
def test_width_seams(dev, form, width):
    """the widths at which a row's lane group doubles and one past a full wavefront step; both sides at the lengths where the
    kept lengths or the window count change, and where the spared side alone refuses the pair; with and without payloads and
    the optional outputs, 64-bit ids, left padding, and outputs 4 bytes (8 with 64-bit ids) off the alignment of the wide
    stores"""
    case = 0
    for specials in (True, False):
        cap = width - 3 * specials
        for stride in sorted({0, cap // 3, cap - 1}):
            for strategy in (SECOND, FIRST, LONGEST):
                lengths = []
                for other in sorted({0, 1, cap // 2, cap - 1, cap, cap + 1}):
                    for n in P.side_seams(cap, stride, other):
                        lengths.append((n, other) if strategy == FIRST else (other, n))
                if strategy == LONGEST:
                    lengths += [(cap // 2, cap // 2 + 1), (cap, cap), (cap + 2, 1), (1, cap + 2), (cap // 2 + 1, cap // 2 + 1)]
                for windows in ([False] if strategy == LONGEST else [True, False]):
                    case += 1
                    ids64 = bool(case & 2)
                    s = P.spec(width, stride, windows, pad_left=bool(case & 1), ids64=ids64, cls_id=2 if specials else None,
                               sep_id=3 if specials else None)
                    front = 32 if case % 3 else (40 if ids64 else 36)
                    want = both_ways(dev, form, lengths, width * 1000 + case, s, strategy, payloads=bool(case & 4), front=front,
                                     extras=case % 5 != 0)
                    assert strategy == LONGEST or want["refused"] > 0
                    assert want["input_ids"].shape[0] > len(lengths) or not windows or stride == cap - 1


@pytest.mark.parametrize("form", ["host", "dev"])
def test_mixed_batch_over_scan_groups(dev, caps, form):
    """fitting, truncated, windowed and refused pairs in one batch of more pairs than one scan group of the plan: row_base,
    status and the five counters of both calls (run() holds the plan to the model, agree() the rows)"""
    n_rows = caps[1] + 37
    rng = np.random.RandomState(n_rows)
    kinds = [(0, 0), (2, 3), (4, 5), (3, 30), (0, 25), (9, 1), (10, 4), (7, 3), (8, 9), (1, 8)]  # cap 9
    lengths = [kinds[i] for i in rng.randint(0, len(kinds), size=n_rows)]
    cmap = ((rng.permutation(4000) + 10).astype(np.uint32), 4000, False)
    cmap[0][::17] = P.NONE
    for strategy, windows, stride in ((SECOND, True, 2), (SECOND, False, 0), (FIRST, True, 0), (FIRST, False, 1), (LONGEST, False, 0)):
        s = P.spec(12, stride, windows, unk_id=77, pad_id=78, cls_id=2, sep_id=3)
        want = both_ways(dev, form, lengths, n_rows + strategy, s, strategy, cmap)
        assert want["n_unknown"] > 0 and (want["refused"] > 0) == (strategy != LONGEST)
        assert (want["lost"] > 0) == (not windows) and want["longest"] == 33
        if windows:
            assert want["input_ids"].shape[0] > n_rows + n_rows // 5


def test_capacity(dev):
    """rows_cap one short: the host form answers SWT_ERR_CAPACITY with the rows needed and writes nothing; the `_dev` form
    writes the rows below rows_cap and leaves everything behind them alone in every output (run() checks the garbage and the
    fences).  The inputs are well-formed throughout: this is the bound of the writes."""
    lengths = [(2, 3), (3, 20), (0, 0), (4, 7), (9, 2), (1, 13)]
    rows_a, rows_b, ids, off_a, off_b, pay = P.pair_stream(lengths, seed=77)
    for windows in (True, False):
        s = P.spec(8, 1, windows, cls_id=2, sep_id=3)
        want = P.expected_pair_batch(rows_a, rows_b, s, SECOND, None, pay)
        need = want["input_ids"].shape[0]
        assert want["refused"] == (2 if windows else 1) and need == (27 if windows else 6)
        rc, res, outs = run(dev, "host", ids, off_a, off_b, s, SECOND, None, pay, rows_cap=need - 1, want=want)
        assert rc == dev.ERR_CAPACITY and res["info"].tolist() == [need, 0, 0, 0, 0]
        for k in ("ids", "mask", "type", "special", "seq", "spans", "word"):
            assert (outs[k].body(np.uint8) == GARBAGE).all(), k
        for cap_rows in (need - 1, 1):
            rc, res, _ = run(dev, "dev", ids, off_a, off_b, s, SECOND, None, pay, rows_cap=cap_rows, want=want)
            assert rc == 0
            agree(res, want, rows=cap_rows, info=False)
            assert int(res["info"][0]) == cap_rows and int(res["info"][1]) == want["longest"]
        rc, res, _ = run(dev, "dev", ids, off_a, off_b, s, SECOND, None, pay, rows_cap=need + 3, want=want)  # room to spare
        agree(res, want)


@pytest.mark.parametrize("form", ["host", "dev"])
def test_map_edges(dev, form):
    """ids at n_map - 1 and n_map, an entry of 0xFFFFFFFF, SWT_BPE_CONT ids through the second half of a flagged map, the identity
    map and its bound, on both sides; info[2] counts every slot that went to unk_id -- a token of the repeated side once per
    window"""
    n_map = 50
    rng = np.random.RandomState(5)
    flat = (1000 + rng.permutation(n_map)).astype(np.uint32)
    flat[7] = P.NONE
    both = np.concatenate([flat, (2000 + rng.permutation(n_map)).astype(np.uint32)])
    both[n_map + 9] = P.NONE
    cont = 0x80000000
    edge = [n_map - 1, n_map, n_map + 1, 7, 9, 0, 0x7FFFFFFF]
    long_row = edge + [x | cont for x in edge] + [int(x) for x in rng.randint(0, n_map, size=11)]
    rows_a = [[n_map, 7], long_row[:3], [], [n_map | cont, 7 | cont, 1]]
    rows_b = [long_row, [9 | cont], [n_map - 1], edge]
    ids = np.array([x for r in rows_a + rows_b for x in r], dtype=np.uint32)
    off = np.array(np.cumsum([0] + [len(r) for r in rows_a + rows_b]), dtype=np.uint64)
    off_a, off_b = off[:5].copy(), off[4:].copy()
    for cmap in ((both, n_map, True), (flat, n_map, False), (None, n_map, False), None):
        for strategy, windows, stride in ((SECOND, False, 0), (SECOND, True, 0), (SECOND, True, 2), (FIRST, True, 1), (LONGEST, False, 0)):
            s = P.spec(10, stride, windows, unk_id=77, pad_id=78, cls_id=2, sep_id=3)
            want = P.expected_pair_batch(rows_a, rows_b, s, strategy, cmap)
            assert cmap is None or want["n_unknown"] > 0
            _, res, _ = run(dev, form, ids, off_a, off_b, s, strategy, cmap, want=want)
            agree(res, want)


@pytest.mark.parametrize("width", [6, 64, 65])
@pytest.mark.parametrize("form", ["host", "dev"])
def test_a_pair_with_an_empty_side_is_the_single_batch_of_the_other_side(dev, form, width):
    """The two instantiations of the one skeleton against each other: without specials, only_first with (n, 0) and only_second
    with (0, n), windowed and truncating, and longest_first with (n, 0) truncating, write what swt_batch_plan / swt_batch_rows
    write for the side that holds the tokens, and refuse no pair.  A two-lane group, a full group on the wide stores, and the
    element-by-element path one past it; each run is also held to its own model, row_base included."""
    stride = width // 3
    lengths = B.seam_lengths(width, width - stride) + [3 * width + 1]
    for strategy, windows in ((FIRST, True), (SECOND, True), (FIRST, False), (SECOND, False), (LONGEST, False)):
        side = int(strategy == SECOND)
        rows_a, rows_b, ids, off_a, off_b, pay = P.pair_stream([(0, n) if side else (n, 0) for n in lengths], seed=width)
        s = P.spec(width, stride, windows)
        want = P.expected_pair_batch(rows_a, rows_b, s, strategy, None, pay)
        want_single = B.expected_batch(rows_b if side else rows_a, s, None, pay[side])
        _, pair, _ = run(dev, form, ids, off_a, off_b, s, strategy, None, pay, want=want)
        _, single, _ = run_single(dev, form, ids, off_b if side else off_a, s, None, pay[side], want_rows=want_single["row_base"])
        assert np.array_equal(want["row_base"], want_single["row_base"])
        for k in ("input_ids", "attention_mask", "length", "sample", "offset_mapping", "word_ids"):
            assert np.array_equal(pair[k], single[k]), (k, strategy, windows)
        assert int(pair["info"][3]) == 0 and int(pair["info"][0]) == int(single["info"][0]) == int(want["row_base"][-1])


# ---- through the classes

PLAIN_KEYS = {"input_ids", "attention_mask", "length", "n_unknown"}


@pytest.mark.parametrize("cls", ["FastBPE", "FastWP", "NaiveBPE", "NaiveWP"])
def test_encode_batch_of_pairs(swt, dev, ref_dir, corpora, cls):
    """a handful of sentences of pan_tadeusz as questions and contexts: the result equals the model applied to the class's own ids
    and spans of each side, device on and off; a refused pair raises on both paths; the default call returns today's keys"""
    tok = _tokenizer(swt, ref_dir, cls)
    texts = [t for t in list(corpora["pan"])[:60] if t.strip()]
    if "WP" in cls:  # a text the reference does not return from has no spans: the span calls raise on it
        status = tok.encode_ids_batch(texts)[2]
        texts = [t for t, st in zip(texts, status) if not st]
    n = 12
    questions, contexts = texts[:n], [" ".join(texts[n + 2 * i:n + 2 * i + 2]) for i in range(n)]
    longest_q = int(np.argmax(np.diff(tok.encode_ids_batch(questions)[1].astype(np.int64))))
    questions[(longest_q + 1) % n], contexts[(longest_q + 2) % n] = "", ""  # an empty side each, away from the longest question
    got = tok._batch_encode_spans(questions + contexts)
    raw, off, spans, word = got[0], got[1], got[-2], got[-1]
    side = lambda lo: [[int(x) for x in raw[int(off[i]):int(off[i + 1])]] for i in range(lo, lo + n)]
    pay_of = lambda lo: ([spans[int(off[i]):int(off[i + 1])].tolist() for i in range(lo, lo + n)],
                         [word[int(off[i]):int(off[i + 1])].tolist() for i in range(lo, lo + n)])
    rows_a, rows_b, pay = side(0), side(n), (pay_of(0), pay_of(n))
    voc, sp = tok._batch_vocabulary(), tok.special_ids()
    cmap = (voc.cmap, voc.n_map, voc.flagged)
    longest_a = max(len(r) for r in rows_a)
    width = longest_a + 3 + 6  # every question leaves the context six tokens
    assert max(len(a) + len(b) for a, b in zip(rows_a, rows_b)) + 3 > width
    keys = ("input_ids", "attention_mask", "token_type_ids", "special_tokens_mask", "sequence_ids", "length", "offset_mapping", "word_ids")
    for truncation, strategy, windows, stride in (("only_second", SECOND, True, 2), ("only_second", SECOND, False, 0),
                                                  ("longest_first", LONGEST, False, 0)):
        s = P.spec(width, stride, windows, pad_id=sp["pad"], unk_id=sp["unk"], cls_id=sp["cls"], sep_id=sp["sep"])
        want = P.expected_pair_batch(rows_a, rows_b, s, strategy, cmap, pay)
        assert not want["refused"] and (want["input_ids"].shape[0] > n) == windows
        for device in (False, True):
            res = _to_numpy(tok.encode_batch(questions, text_pairs=contexts, max_length=width, stride=stride, padding="max_length",
                                             truncation=truncation, return_overflowing=windows, return_offsets=True,
                                             return_special_tokens_mask=True, device=device))
            for k in keys:
                assert np.array_equal(res[k], want[k]), (k, truncation, device)
            assert res["n_unknown"] == want["n_unknown"]
            assert ("overflow_to_sample_mapping" in res) == windows
            if windows:
                assert np.array_equal(res["overflow_to_sample_mapping"], want["sample"])
    # padding="longest", no specials, int64, left padding; token types can be declined
    s = P.spec(max(len(a) + len(b) for a, b in zip(rows_a, rows_b)), ids64=True, pad_left=True, pad_id=sp["pad"], unk_id=sp["unk"])
    want = P.expected_pair_batch(rows_a, rows_b, s, LONGEST, cmap)
    for device in (False, True):
        res = _to_numpy(tok.encode_batch(questions, text_pairs=contexts, add_special_tokens=False, padding_side="left", int64=True,
                                         return_token_type_ids=False, device=device))
        assert set(res) == PLAIN_KEYS | {"sequence_ids"} and res["input_ids"].dtype == np.int64
        for k in ("input_ids", "attention_mask", "sequence_ids", "length"):
            assert np.array_equal(res[k], want[k]), (k, device)
    # a refused pair: the longest question alone fills the row
    for device in (False, True):
        with pytest.raises(ValueError, match=r"pair \d+ \(\d+ and \d+ tokens\)"):
            tok.encode_batch(questions, text_pairs=contexts, max_length=longest_a + 3, padding="max_length", truncation="only_second", device=device)
        with pytest.raises(ValueError, match="stride"):
            tok.encode_batch(questions, text_pairs=contexts, max_length=longest_a + 5, stride=2, padding="max_length", truncation="only_second",
                             return_overflowing=True, device=device)
    # without pairs nothing changes, and the pair keywords have nothing to act on
    for device in (False, True):
        assert set(tok.encode_batch(questions, device=device)) == PLAIN_KEYS
        assert set(tok.encode_batch(questions, max_length=8, return_overflowing=True, return_offsets=True, device=device)) == \
            PLAIN_KEYS | {"overflow_to_sample_mapping", "offset_mapping", "word_ids"}
    for bad in ({"truncation": "only_first"}, {"return_token_type_ids": True}, {"return_special_tokens_mask": True}):
        with pytest.raises(ValueError):
            tok.encode_batch(questions, **bad)
    with pytest.raises(ValueError):
        tok.encode_batch(questions, text_pairs=contexts[:-1])
    with pytest.raises(ValueError):
        tok.encode_batch(questions, text_pairs=contexts, max_length=width, truncation="longest_first", return_overflowing=True)
    with pytest.raises(ValueError):
        tok.encode_batch(questions, text_pairs=contexts, truncation="shortest")
