"""The conditions that keep tests/test_gpu_counters.py from being hollow, checked without a GPU: the constants the constructions
are laid out by are the kernels', every construction reaches the seam it is named for in the models of tests/counter_cases.py,
the census model is the oracle's Counter wherever no word reaches 255 bytes (and folds into it where one does), and the
vectorised references of the equivalence rows are the Counter restatement."""
import math
import time

import numpy as np
import pytest

from tests import codepoint_cases as P
from tests import counter_cases as K

FAMILIES = list(K.CENSUS_FAMILIES)


@pytest.fixture(scope="module", autouse=True)
def started():
    """when the first test of this file began"""
    return time.monotonic()


def test_constants_are_the_kernels():
    """the seams sit where these say; if a kernel's constant moves, this fails before a case silently leaves its seam"""
    got = K.constants()
    assert got == K.EXPECTED_CONSTANTS, {k: (v, K.EXPECTED_CONSTANTS.get(k)) for k, v in got.items() if v != K.EXPECTED_CONSTANTS.get(k)}
    assert (K.TILE, K.CAP, K.CUT_ROOM, K.LONG, K.OFF_BITS, 64 - K.TAG_SHIFT, K.MIN_BITS) == (512, 1024, 4, 255, 40, 16, 10)
    assert (K.OCC_MUL, K.OCC_ADD) == (2, 16) and K.table_bits(504) == 10 and K.table_bits(505) == 11
    assert (K.MH_THREADS, K.MH_SLOTS, K.MH_PER_LANE, K.MH_PROBES, K.MH_MAX_BLOCKS) == (256, 1024, 64, 8, 2048)
    assert (K.MH_STRETCH, K.MH_BLOCK, K.MH_SECOND) == (4096, 16384, 33554432) and 1 << (32 - K.MH_SHIFT) == K.MH_SLOTS
    assert (K.TE_THREADS, K.TE_WAVE_CAP, K.TE_BLOCK_THREADS, K.TE_BLOCK_CAP) == (256, 256, 1024, 2048)
    assert (K.TE_WAVE_BLOCKS_PER_CU, K.TE_BLOCK_BLOCKS_PER_CU) == (8, 1)  # the grid caps 8 * n_cu and n_cu
    # the code-point sweep reads the same two from the same file
    assert P.constants()["kWTile"] == K.TILE and P.constants()["kWCap"] == K.CAP
    w = K._read("swt_words.hip")
    for c in ("0xcbf29ce484222325ull", "0x100000001b3ull", "h ^= h >> 29; h *= 0x9E3779B97F4A7C15ull; h ^= h >> 32;", "uint32_t idx = (uint32_t)h & mask;",
              "const uint64_t abase = cb & ~15ull;", "const bool last = avail <= (uint64_t)kWCap;", "idx = (idx + 1) & mask;"):
        assert c in w, c
    m = K._read("swt_metrics.hip")
    assert "te_hash(uint32_t c) { return c * 2654435761u; }" in m and "h = (h + 1) & (kMhSlots - 1);" in m
    from subword_tokenizers_amd import _native
    assert _native.WP_CONT == K.WP_CONT and _native.BPE_CONT == K.CONT


def test_hash_model():
    """the vectorised FNV-1a and finish against the scalar one, and the scalar one against a value worked out by hand"""
    assert K.word_hash(b"") == ((0xcbf29ce484222325 ^ (0xcbf29ce484222325 >> 29)) * 0x9E3779B97F4A7C15 % 2 ** 64) ^ \
        (((0xcbf29ce484222325 ^ (0xcbf29ce484222325 >> 29)) * 0x9E3779B97F4A7C15 % 2 ** 64) >> 32)
    words = [b"ab", b"ba", b"zz"]
    assert [int(x) for x in K.word_hash_np(np.frombuffer(b"".join(words), dtype=np.uint8).reshape(3, 2))] == [K.word_hash(w) for w in words]
    assert len({K.word_hash(w) for w in words}) == 3


def all_batches():
    return [(f, b) for f in FAMILIES for b in K.census_batches(f)]


def test_batches_are_small_lowercase_and_of_the_alphabet():
    names = set()
    for f, b in all_batches():
        size = sum(map(K.nbytes, b.sents))
        assert b.name not in names, b.name
        names.add(b.name)
        assert set("".join(b.sents)) <= K.ALPHABET, b.name
        assert all(s == P.lower(s) and not P.has_host(s) for s in b.sents), b.name  # the joined form lowers on the device
        assert size <= (70_000 if f == "contention" else 8_000), (b.name, size)
        pad = K.padded(b.sents)
        assert len(pad) > 64 and (len(pad) == len(b.sents) or pad[:len(b.sents)] == list(b.sents))
    words = {w for _f, b in all_batches() for s in b.sents for w in s.split()}
    assert not words & set(K.padding()) and len(set(K.padding())) == K.PAD_SENTENCES


def test_walk_splits_as_the_oracle_and_counts_every_word_once(oracle):
    """the model's classes give the oracle's words, and the chunk walk of the model inserts exactly those, each once, whole"""
    for f, b in all_batches():
        for sents in (b.sents, K.padded(b.sents)):
            w = K.Walk(sents)
            want = [x for s in sents for x in oracle.pretokenize(s)]
            assert [x.decode("utf-8") for _p, x in w.words()] == want, b.name
            assert [(p, e) for p, e, _how in w.counted()] == [(p, p + len(x)) for p, x in w.words()], b.name


def same_stream(a, b, what):
    assert np.array_equal(a.woff, b[1]) and np.array_equal(a.freq, b[2]) and np.array_equal(a.syms, b[0]), what


def test_census_model_is_the_oracle(oracle):
    """no word of 255 bytes: the model is OracleBPETrainer.export(); with such words its duplicate entries fold into it; its
    distinct code points are the initial vocabulary either way"""
    plain = longs = repeated = 0
    for f, b in all_batches():
        for sents in (b.sents, K.padded(b.sents)):
            orc = P.oracle_census(oracle, list(sents))
            got = orc.export()
            model = K.census_model(oracle, sents)
            if K.has_long(sents):
                longs += 1
                repeated += model.n_words > got[2].size  # a long word that occurs twice: two entries here, one there
                assert model.n_words >= got[2].size, b.name
                same_stream(K.census_model(oracle, sents, folded=True), got, b.name)
            else:
                plain += 1
                same_stream(model, got, b.name)
            assert np.array_equal(model.base, np.unique(got[0])) and orc.vocab_size == model.base.size, b.name
            assert sum(model.hist.values()) == int(((np.diff(model.woff.astype(np.int64)) - 1).clip(0) * model.freq).sum())
            wp = K.census_model(oracle, sents, wordpiece=True)
            first = np.zeros(wp.syms.size, dtype=bool)
            first[wp.woff[:-1].astype(np.int64)] = True
            assert np.array_equal(wp.syms, np.where(first, model.syms, model.syms + K.WP_CONT)) and np.array_equal(wp.freq, model.freq)
    assert plain > 30 and longs > 300 and repeated > 20


def test_every_construction_reaches_its_seam():
    """the models show the event each batch is named for; together they reach every exit of the chunk walk"""
    entered, ended, n_expect = set(), set(), 0
    for f, b in all_batches():
        assert b.expect or f == "contention" or "very end" in b.name, b.name
        w, (bits, ins) = K.holds(b)
        n_expect += len(b.expect)
        for c in w.all_chunks():
            if c["giant"]:
                entered.add(c["giant"][0])
                ended.add(c["giant"][1])
            elif not c["last"]:
                assert c["off0"] < c["cut"] - c["abase"] <= c["staged"] - K.CUT_ROOM
    assert entered == {"ws", "punct", "word"} and ended == {"first", "ws", "punct", "send"}
    assert n_expect > 500


def test_cut_sweep_is_complete():
    names = {b.name for b in K.census_batches("cut")}
    assert len(names) == len(K.CUT_OFF0) * (len(K.CUT_STRADDLERS) * (2 * len(K.CUT_BACK) + len(K.SENT_BACK)) + len(K.BRAILLE_BACK) + 3)
    cut = lane = last = 0
    for b in K.census_batches("cut"):
        c = K.Walk(b.sents).chunks(1)[0]
        cut += c["cut"] is not None
        lane += c["giant"] is not None
        last += c["last"]
    # staged - 5 and staged - 4 cut, staged - 3 and staged - 1 go to the one lane; a sentence start up to staged ends the span
    per = len(K.CUT_OFF0) * len(K.CUT_STRADDLERS)
    assert (cut, lane, last) == (per * 4 + 9 + len(K.CUT_OFF0) * len(K.BRAILLE_BACK), per * 4 + per, per * 5)


def test_collisions_meet_in_the_table():
    c = K.collisions()
    assert c["n_groups"] > 1000  # 2^20 candidates: thousands of pairs, and the three words of the chain
    for group in (c["pair"], c["triple"], c["wrap"]):
        hs = [K.word_hash(w.encode()) for w in group]
        assert len(set(group)) == len(group) and len({len(w) for w in group}) == 1
        assert len({h >> K.TAG_SHIFT for h in hs}) == 1 and len({h & 1023 for h in hs}) == 1 and len(set(hs)) == len(hs)
    assert K.word_hash(c["wrap"][0].encode()) & 1023 == 1023
    a, b = K.first_byte_pair()
    ha, hb = K.word_hash(a.encode()), K.word_hash(b.encode())
    assert a[0] != b[0] and a[1:] == b[1:] and len(a) == 6 and (ha >> K.TAG_SHIFT, ha & 1023) == (hb >> K.TAG_SHIFT, hb & 1023) and ha != hb
    for b in K.census_batches("collisions"):
        for sents in (b.sents, K.padded(b.sents)):  # the joined form's padding comes behind: the same slots, the same table
            w = K.Walk(sents)
            bits, ins = K.table_model([x for _p, x in w.words()])
            assert len(ins) <= 504 and bits == K.MIN_BITS, b.name
            K.holds(b._replace(expect=tuple(e for e in b.expect if e[0] in ("insert", "foreign", "bits"))), walk=w, table=(bits, ins))


def test_table_batches_sit_on_the_sizing_step():
    seen = set()
    for b in K.census_batches("table"):
        w = K.Walk(b.sents)
        n = len(w.words())
        seen.add((n, K.table_bits(n), len({x for _p, x in w.words()}) == n))
        assert K.padded(b.sents) == list(b.sents)
    assert seen == {(504, 10, True), (505, 11, True), (504, 10, False), (505, 11, False)}


def test_contention_batch():
    batch, late = K.contention_batch()
    w = K.Walk(batch.sents)
    words = w.words()
    assert 50_000 < w.n < 70_000 and 2000 < len(batch.sents) < 4000
    count = {}
    first = {}
    for p, x in words:
        count[x] = count.get(x, 0) + 1
        first.setdefault(x, p // K.TILE)
    assert len(count) == 300 and count[b"the"] * 2 >= len(words)
    assert len(late) >= 149 and all(first[x.encode()] >= w.n_tiles // 2 for x in late)
    assert K.table_bits(len(words)) > 14


def test_histogram_cases():
    cases = K.hist_cases()
    assert [c.ids.size for c in cases[:len(K.HIST_LENGTHS)]] == list(K.HIST_LENGTHS)
    assert set(K.HIST_LENGTHS) >= {1, 63, 64, 65, 4095, 4096, 4097, 16383, 16384, 16385}
    modelled = 0
    for c in cases:
        sym = c.ids & 0x7FFFFFFF
        assert sym.max() < c.id_cap and c.ids.dtype == np.uint32, c.name
        want, oor = K.hist_want(c.ids, c.id_cap)
        assert oor == 0 and int(want.sum()) == c.ids.size
        if c.given_up is None:
            continue
        modelled += 1
        assert c.ids.size == K.MH_STRETCH and K.hist_waves(c.ids.size) == (1, 4, 1)  # one stretch: one wave's table takes all of it
        idx = sym.astype(np.int64) + c.id_cap * (c.ids >> 31).astype(np.int64)
        used, given_up, wrapped = K.mh_stretch_model(idx)
        assert given_up >= c.given_up[0] and (given_up == 0) == (c.given_up[0] == 0), (c.name, used, given_up)
        assert c.given_up[1] is None or wrapped == c.given_up[1], (c.name, wrapped)
        if "home slot" in c.name:
            assert np.unique(K.mh_bucket(idx)).size == 1 and used == min(np.unique(idx).size, K.MH_PROBES)
            assert (idx < c.id_cap).any() and (idx >= c.id_cap).any()  # both halves of the counter array
    assert modelled == 7
    by_name = {c.name: c for c in cases}
    assert by_name["id_cap 1"].id_cap == 1 and by_name["id_cap 1,001, not a power of two"].id_cap == 1001
    c = by_name["sym == id_cap - 1 on both halves"]
    assert {int(x) for x in c.ids} >= {c.id_cap - 1, (c.id_cap - 1) | K.CONT}
    ids, cap, n_bad = K.hist_out_of_range_case()
    want, oor = K.hist_want(ids, cap)
    assert oor == n_bad == 7 and int(want.sum()) == ids.size - 7 and cap in ids and (cap | K.CONT) in ids
    # the second stretch: the grid is capped, wave 0 gets 4,096 more ids and wave 1 one
    assert K.SECOND_STRETCH_N == 2048 * 16384 + 4097
    assert K.hist_waves(K.MH_SECOND) == (2048, 8192, 1) and K.hist_waves(K.SECOND_STRETCH_N) == (2048, 8192, 2)
    assert K.SECOND_STRETCH_N - K.MH_SECOND == K.MH_STRETCH + 1


@pytest.mark.parametrize("n_cu", [256, 304, 8, 9, 10, 11, 12, 13])
def test_equivalence_wave_rows(n_cu):
    """a wave's second and third row: the kinds' period is coprime to the number of waves, the grid is at its cap, and some wave
    meets a row that probes for X (kind 1) directly behind one that inserted X (kinds 0 and 3)"""
    ra, rb, kinds, want = K.te_wave_rows(n_cu)
    n_rows = len(ra)
    blocks, n_waves = K.te_wave_geometry(n_rows, n_cu)
    assert n_rows == 2 * 32 * n_cu + 5 and (blocks, n_waves) == (8 * n_cu, 32 * n_cu)
    assert math.gcd(len(K.TE_KINDS), n_waves) == 1
    assert set(K.TE_KINDS) == {0, 1, 2, 3}
    for nth in (1, 2):  # second row of every wave, third row of waves 0 .. 4
        cur = kinds[nth * n_waves:min((nth + 1) * n_waves, n_rows)]
        prev = kinds[(nth - 1) * n_waves:][:cur.size]
        assert cur.size == (n_waves if nth == 1 else 5)
        assert np.count_nonzero(np.isin(prev, (0, 3)) & (cur == 1)) >= 1, nth
    assert K.te_wave_keys(ra, rb, n_waves) < 512  # kTeWaveSlots: an empty slot in every wave's table whatever was left in it
    assert all(min(len(a), len(b)) <= K.TE_WAVE_CAP for a, b in zip(ra, rb))
    assert max(min(len(a), len(b)) for a, b in zip(ra, rb)) == K.TE_WAVE_CAP
    # by hand: X against itself, against a disjoint row, against nothing
    assert tuple(want[0]) == (8, 8, 8, 1) and tuple(want[1]) == (7, 0, 0, 0) and tuple(want[4]) == (0, 0, 0, 0)
    assert want[kinds == 3][:, 2].min() >= 8 and (want[kinds == 1][:, 2:] == 0).all()
    for r in (0, 3, 4, 7, 11, 2, n_rows - 1):
        assert tuple(want[r]) == K.te_brute(ra[r], rb[r])


def test_equivalence_block_rows():
    """the second tile of a workgroup: the vectorised reference against the Counter one, and where the long rows lie"""
    n_cu = 8
    sa, sb, want, longs = K.te_block_rows(n_cu)
    n_rows = sa[1].size - 1
    T = K.TE_BLOCK_THREADS
    assert n_rows == T * n_cu + 1030 and -(-n_rows // T) == n_cu + 2 > n_cu  # more tiles than workgroups: n_cu at the most
    assert [(r // T, r % T) for r in longs] == [(0, 0), (0, 1), (0, T - 1), (n_cu, 0), (n_cu, T - 1), (n_cu + 1, 3)]
    assert (n_cu + 1) * T + 3 < n_rows < (n_cu + 2) * T  # the last tile is a partial one
    la, lb = np.diff(sa[1].astype(np.int64)), np.diff(sb[1].astype(np.int64))
    m = np.minimum(la, lb)
    assert sorted(np.flatnonzero(m > K.TE_WAVE_CAP)) == sorted(longs) and m[[r for r in range(n_rows) if r not in longs]].max() == 2
    for r in longs:
        assert r + 1 in longs or (la[r + 1], lb[r + 1]) == (2, 2)
    split = longs[3]
    short = (sa if la[split] <= lb[split] else sb)[0][int((sa if la[split] <= lb[split] else sb)[1][split]):][:int(m[split])]
    assert np.unique(short).size == 2 * K.TE_BLOCK_CAP and K.te_first_parts(short, 1).max() > K.TE_BLOCK_CAP
    for r in range(n_rows):
        a, b = sa[0][int(sa[1][r]):int(sa[1][r + 1])], sb[0][int(sb[1][r]):int(sb[1][r + 1])]
        assert tuple(want[r]) == K.te_brute(a, b), r
    assert want[:, 1].sum() > 100 and want[:, 2].sum() > want[:, 1].sum() and 0 < want[:, 3].sum() < n_rows


def test_this_file_is_quick(started):
    """runs last: everything above, the generators included, within a minute"""
    assert time.monotonic() - started < 60
