"""The seams of the three device Counters against plain references, exact: the training word census (csrc/swt_words.hip) against
the Python model of the device's rule in tests/counter_cases.py (which is the oracle's Counter wherever no word reaches 255 bytes:
tests/test_counter_cases.py), the token histogram (token_hist_kernel) against np.bincount, and the token-sequence equivalence
(token_equiv_wave_kernel, token_equiv_block_kernel) against the Counter restatement of tests/test_gpu_equivalence.py.  The
constructions, the models that say which seam each one reaches and what the geometry allows are in tests/counter_cases.py; that
every one reaches its seam is checked without a GPU by tests/test_counter_cases.py.  Every batch of every family runs here.

Every census batch goes through BpeTrainer.from_text, through swt_bpe_train_create_joined (with fewer than 65 sentences: 65
one-word sentences appended, the model padded alike) and through from_text_wordpiece; word offsets, frequencies, symbols, info(),
base_symbols() and histogram() are compared with the model, and where no word reaches 255 bytes the helpers of
tests/test_gpu_codepoints.py compare the same trainers with the C oracle as well.

The two large calls are test_histogram_second_stretch (33,558,529 ids, 134 MB: a wave needs more than 2,048 * 16,384 ids before
it takes a second stretch) and test_equivalence_block_second_tile (1,024 * n_cu + 1,030 rows: a workgroup needs more than
1,024 * n_cu rows before it takes a second tile).  Neither can be smaller and still reach its seam; their times, and every other
test's, are in profiles/counters.txt, the mutants that were run against this file in DESIGN.md 4.4d.

Needs a real MI355X: `-m gpu`."""
import math
import re

import numpy as np
import pytest

from tests import codepoint_cases as P
from tests import counter_cases as K
from tests.test_gpu_codepoints import census_from_text, census_joined, same_census, same_census_wp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(native):
    if native.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests need an MI355X (there is no CPU fallback to test)")
    native.init(0)
    return native


# ================================================================================================================= census

def same_stream(tr, want, what):
    """export(), info(), base_symbols() and histogram() of a trainer against a model stream, all exact"""
    gs, go, gf = tr.export()
    assert np.array_equal(go, want.woff), "%s: word offsets differ (%d / %d words)" % (what, go.size - 1, want.woff.size - 1)
    assert np.array_equal(gf, want.freq), "%s: frequencies differ, first at word %d" % (what, int(np.flatnonzero(gf != want.freq)[0]))
    if not np.array_equal(gs, want.syms):
        at = int(np.flatnonzero(gs != want.syms)[0])
        pytest.fail("%s: symbol %d differs: got %#x, want %#x" % (what, at, gs[at], want.syms[at]))
    info = tr.info()
    assert (info["n_words"], info["n_symbols"]) == (want.n_words, want.syms.size), "%s: info() %r" % (what, info)
    assert np.array_equal(tr.base_symbols(), want.base), "%s: base symbols differ" % what
    keys, cnts = tr.histogram()
    got = dict(zip(keys.tolist(), cnts.tolist()))
    assert len(got) == keys.size, "%s: a pair twice in the histogram" % what
    if got != want.hist:
        bad = sorted(k for k in set(got) | set(want.hist) if got.get(k) != want.hist.get(k))[:5]
        pytest.fail("%s: histogram differs at %s" % (what, [(hex(k), got.get(k), want.hist.get(k)) for k in bad]))


def check_census(dev, oracle, b):
    sents, pad = list(b.sents), K.padded(b.sents)
    plain, plain_pad = not K.has_long(sents), not K.has_long(pad)
    want = K.census_model(oracle, sents)
    tr = census_from_text(dev, sents)
    same_stream(tr, want, "from_text, " + b.name)
    if plain:
        same_census(tr, P.oracle_census(oracle, sents), "from_text against the oracle, " + b.name)
    tr.close()
    tr = census_joined(dev, pad)
    same_stream(tr, want if pad == sents else K.census_model(oracle, pad), "joined, " + b.name)
    if plain_pad:
        same_census(tr, P.oracle_census(oracle, pad), "joined against the oracle, " + b.name)
    tr.close()
    tr = census_from_text(dev, sents, wordpiece=True)
    same_stream(tr, K.census_model(oracle, sents, wordpiece=True), "from_text_wordpiece, " + b.name)
    if plain and want.n_words:
        same_census_wp(dev, tr, P.oracle_census(oracle, sents, True), P.oracle_census(oracle, sents), "wordpiece against the oracle, " + b.name)
    tr.close()


CUT_PARTS = 3  # the 177 batches of the cut rule in three tests: one per off0


@pytest.mark.parametrize("family,part", [(f, k) for f in K.CENSUS_FAMILIES for k in range(CUT_PARTS if f == "cut" else 1)])
def test_census_seams(dev, oracle, family, part):
    batches = K.census_batches(family)
    if family == "cut":
        batches = [b for b in batches if int(re.findall(r"off0 (\d+)", b.name)[-1]) == K.CUT_OFF0[part]]
        assert len(batches) * CUT_PARTS == len(K.census_batches(family))
    assert batches
    for b in batches:
        check_census(dev, oracle, b)


@pytest.mark.parametrize("family", K.MERGE_FAMILIES)
def test_census_merges(swt, dev, oracle, family):
    """the words of 255 bytes and more are entries of their own with frequency 1 on the device and one entry in the reference:
    the first 30 merges are the same"""
    for b in K.census_batches(family):
        max_vocab = int(K.census_model(oracle, b.sents).base.size) + 30
        tok = swt.NaiveBPE()
        tok.train(list(b.sents), max_vocab)
        orc = oracle.OracleBPETrainer(list(b.sents))
        orc.run(max_vocab)
        assert 10 <= len(orc.merges_list) <= 30, b.name  # the long words are periodic: some batches run out of pairs before 30
        assert tok.merges_list == orc.merges_list, b.name
        assert len(tok.vocab) == orc.vocab_size, b.name


# ============================================================================================================== histogram

def same_counts(got, want, what):
    if not np.array_equal(got, want):
        at = np.flatnonzero(got != want)
        pytest.fail("%s: %d counters differ, first %d: got %d, want %d" % (what, at.size, at[0], got[at[0]], want[at[0]]))


@pytest.mark.parametrize("case", [c.name for c in K.hist_cases()])
def test_histogram_cases(dev, case):
    c = next(x for x in K.hist_cases() if x.name == case)
    want, oor = K.hist_want(c.ids, c.id_cap)
    assert oor == 0 and int(want.sum()) == c.ids.size
    got, got_oor = dev.token_histogram_counts(c.ids, c.id_cap)
    assert got_oor == 0
    same_counts(got, want, case)
    same_counts(dev.token_histogram(c.ids, c.id_cap), want, case + ", the raising wrapper")


def test_histogram_out_of_range(dev):
    """sym == id_cap and beyond among valid ids: counted in out_of_range and nowhere else, the other counters as without them"""
    ids, cap, n_bad = K.hist_out_of_range_case()
    want, oor = K.hist_want(ids, cap)
    assert oor == n_bad
    got, got_oor = dev.token_histogram_counts(ids, cap)
    assert got_oor == n_bad
    same_counts(got, want, "out of range")
    valid = ids[(ids & 0x7FFFFFFF) < cap]
    same_counts(dev.token_histogram(valid, cap), want, "the same ids without the seven")
    with pytest.raises(ValueError, match="%d token ids" % n_bad):
        dev.token_histogram(ids, cap)


def test_histogram_second_stretch(dev):
    """2,048 * 16,384 + 4,097 ids: the grid is at its cap of 2,048 blocks, wave 0 clears its table and counts a second stretch of
    4,096 ids, wave 1 one of a single id"""
    assert K.hist_waves(K.SECOND_STRETCH_N) == (K.MH_MAX_BLOCKS, 4 * K.MH_MAX_BLOCKS, 2)
    ids = K.second_stretch_ids()
    assert ids.size == K.SECOND_STRETCH_N == 2048 * 16384 + 4097
    want, oor = K.hist_want(ids, K.SECOND_STRETCH_CAP)
    assert oor == 0 and int(want[0]) > 10 * int(want[K.SECOND_STRETCH_CAP // 2]) > 0  # heavy-headed
    assert np.count_nonzero(want[:K.SECOND_STRETCH_CAP]) > 50000 and np.count_nonzero(want[K.SECOND_STRETCH_CAP:]) > 50000
    got, got_oor = dev.token_histogram_counts(ids, K.SECOND_STRETCH_CAP)
    assert got_oor == 0
    same_counts(got, want, "second stretch")


# ============================================================================================================ equivalence

def test_equivalence_wave_second_row(dev):
    """2 * 32 * n_cu + 5 rows: every wave of the capped grid takes a second row and five take a third, of another kind than the
    row before; a table that is not cleared adds to `unordered` and `has_common` of the rows that probe for the eight tokens
    the row before inserted"""
    n_cu = dev.device_info()[0]
    ra, rb, kinds, want = K.te_wave_rows(n_cu)
    n_rows = len(ra)
    n_waves = K.te_wave_geometry(n_rows, n_cu)[1]
    assert n_rows == 2 * 32 * n_cu + 5 and n_waves == 32 * n_cu and math.gcd(len(K.TE_KINDS), n_waves) == 1
    for nth in (1, 2):
        cur = kinds[nth * n_waves:min((nth + 1) * n_waves, n_rows)]
        assert np.count_nonzero(np.isin(kinds[(nth - 1) * n_waves:][:cur.size], (0, 3)) & (cur == 1)) >= 1
    sa, sb = K.te_side(ra), K.te_side(rb)
    totals, rows = dev.token_equivalence(sa, sb, per_row=True)
    bad = np.flatnonzero((rows.astype(np.int64) != want).any(axis=1))
    assert bad.size == 0, [(int(i), int(kinds[i]), rows[i].tolist(), want[i].tolist()) for i in bad[:8]]
    assert [int(x) for x in totals] == want.sum(axis=0).tolist()
    weight = np.random.default_rng(5).integers(0, 2 ** 32, size=n_rows, dtype=np.uint64).astype(np.uint32)
    weight[::11] = 0
    got = dev.token_equivalence(sa, sb, weight=weight)
    assert [int(x) for x in got] == [int((weight.astype(np.int64) * want[:, c]).sum()) for c in range(4)]  # below 2^55


def test_equivalence_block_second_tile(dev):
    """1,024 * n_cu + 1,030 rows: workgroups 0 and 1 of the capped grid take a second tile; long rows at the first, second and
    last place of tile 0, at the first and last place of tile n_cu and in the last, partial tile, one of them split over passes"""
    n_cu = dev.device_info()[0]
    sa, sb, want, longs = K.te_block_rows(n_cu)
    n_rows = sa[1].size - 1
    T = K.TE_BLOCK_THREADS
    assert n_rows == T * n_cu + 1030 and -(-n_rows // T) == n_cu + 2
    assert [(r // T, r % T) for r in longs] == [(0, 0), (0, 1), (0, T - 1), (n_cu, 0), (n_cu, T - 1), (n_cu + 1, 3)]
    totals, rows = dev.token_equivalence(sa, sb, per_row=True)
    bad = np.flatnonzero((rows.astype(np.int64) != want).any(axis=1))
    assert bad.size == 0, [(int(i), rows[i].tolist(), want[i].tolist()) for i in bad[:8]]
    assert [int(x) for x in totals] == want.sum(axis=0).tolist()
    weight = np.random.default_rng(6).integers(0, 2 ** 32, size=n_rows, dtype=np.uint64).astype(np.uint32)
    weight[longs[1]] = 0
    weight[longs[3]] = 0xFFFFFFFF
    got = dev.token_equivalence(sa, sb, weight=weight)
    assert [int(x) for x in got] == [int((weight.astype(np.int64) * want[:, c]).sum()) for c in range(4)]  # below 2^55
