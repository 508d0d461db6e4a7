"""The literal merge rounds of bpe_lane_kernel (csrc/swt_bpe_encode.hip: literal_rounds for a word in LDS, walker_rounds for a
word longer than a chunk) under their three merge rules.  profiles/merge_rule.txt names the test that drives each combination
of loop, rule and table; this file holds the ones no other test reaches:

  * FastBPE's rank order on an UNPACKED table in the LDS loop -- the proper unpacked table of test_gpu_parity never leaves the
    one-occurrence rounds on its text, and every improper table elsewhere is packed;
  * the three rules where they must agree, on a table that is improper AND unpacked: BPE-dropout at drop_below = 0 equals the
    plain encode id for id (test_gpu_dropout holds that for an improper packed and a proper unpacked table), and NaiveBPE's
    list order equals both on a list whose order cannot matter.

Every case is held to the plain-Python model of tests/dropout_cases.py at drop_below = 0, which is the literal loop of
bpe.py:210-238.  Needs an MI355X."""
import pytest

from tests import dropout_cases as D
from tests.test_naive_bpe_encode import RisingFloor, splitter
from tests.test_gpu_dropout import GIANT_ASCII, GIANT_WIDE, LONG33, LONG100, Case, same, table_info

pytestmark = pytest.mark.gpu

SHIFT = 0x10000  # merged symbols numbered from here: an index of at least 0xFFFF does not fit a packed value
LONG32 = "ab" * 16
# words of 2, 32, 33 and 100 symbols, one just longer than a chunk in ASCII and one in multi-byte letters
WORDS = ["ab", LONG32, LONG33, LONG100, "aaaaaaa", "abcabc", "xyxyx", "qqqqq", "żółżół", GIANT_ASCII, GIANT_WIDE]
DIRECT = ["ab " + LONG32 + " " + LONG33, "", LONG100 + " aaaaaaa abcabc xyxyx", "qqqqq żółżół ab"]  # the single workgroup
TILED = D.short_sentences(24, 1800, seed=21) + [" ".join(WORDS), "", GIANT_ASCII + " ab", LONG33 + "," + LONG100] + D.short_sentences(12, 900, seed=22)


@pytest.fixture(scope="module")
def dev(native):
    if native.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests need an MI355X (there is no CPU fallback to test)")
    native.init(0)
    return native


@pytest.fixture(scope="module")
def split(swt):
    return swt.SubwordTokenizer._split


@pytest.fixture(scope="module")
def unpacked(swt, dev):
    out = {"proper": Case(swt, dev, D.PROPER, SHIFT), "improper": Case(swt, dev, D.IMPROPER, SHIFT)}
    assert [table_info(dev, out[k].tok, 1) for k in ("proper", "improper")] == [0, 0]  # neither is packed
    assert [table_info(dev, out[k].tok, 2) for k in ("proper", "improper")] == [1, 0]
    return out


def plain(c, texts):
    text, off = c.dev.pack_and_lower(texts)
    return c.tok._table.encode(text, off, flags=c.dev.BPE_NO_DEDUP)


@pytest.mark.parametrize("name", ["proper", "improper"])
@pytest.mark.parametrize("texts", [DIRECT, TILED], ids=["single workgroup", "tiles"])
def test_rank_order_on_an_unpacked_table(unpacked, split, texts, name):
    """proper: the words beyond 32 symbols take the literal rounds; improper: every word does.  The merged symbol comes from
    merged_of_rank[]."""
    c = unpacked[name]
    n_bytes = sum(len(t.encode()) for t in texts)
    assert (len(texts) <= 64 and n_bytes <= 1024) == (texts is DIRECT)
    same(plain(c, texts), c.want(split, texts, 0), "%s unpacked table, %d bytes" % (name, n_bytes))


@pytest.mark.parametrize("texts", [DIRECT, TILED], ids=["single workgroup", "tiles"])
def test_dropout_at_zero_is_the_plain_encode_on_an_improper_unpacked_table(unpacked, texts):
    c = unpacked["improper"]
    same(c.got(texts, 0), plain(c, texts), "drop_below 0 against swt_bpe_encode")


def test_list_order_agrees_where_the_order_cannot_matter(swt, dev, unpacked, split):
    """the proper list with one pair repeated at its end: not order-equivalent, so NaiveBPE takes the ordered kernel and follows
    the pair's chain, but the repeat finds nothing left to merge -- list order (the rising-floor model) and rank order (the
    model at drop_below = 0, which the unpacked table is held to above) spell the same words"""
    merges = D.PROPER + [D.PROPER[0]]
    naive = swt.NaiveBPE()
    naive.merges_list = list(merges)
    assert not naive._ensure_naive_table().order_equivalent()
    floor, pre = RisingFloor(merges), splitter()
    want = [floor.tokenize(t, pre) for t in TILED]
    assert want == D.tokenize(D.Table(D.PROPER), split, TILED, 0)
    assert naive.tokenize_batch(TILED) == want
    c = unpacked["proper"]
    same(c.got(TILED, 0), c.want(split, TILED, 0), "drop_below 0, proper unpacked table")
