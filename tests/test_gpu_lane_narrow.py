"""The NARROW form of the FastBPE running-text kernel (csrc/swt_bpe_encode.hip: bpe_lane_kernel<.., Narrow>, csrc/swt_bpe_narrow.h)
against the C oracle, ids and offsets exact.

A packed table below 32 k symbols keeps 16-bit symbol codes in LDS, stages 640 bytes a chunk (CAP) and takes tiles of 512 bytes
(TILE) in the library's own geometry -- by the library's own choice from one chip-full of 384-byte tiles up, so the small
texts here ask for it at every size (SWT_OPT_LANE_NARROW = 2).  Every test that means to run the narrow kernel asserts that the
library chose it -- swt_debug_bpe_table_info 7 (the policy: 2 = every running-text call, 1 = from the floor up, 0 = none)
before the call, and 11 after it: the kernel the launch itself took, written where the launch picks it (1 narrow, 0 wide) -- since
a call that fell back to the wide kernel would give the same arrays.  A code point outside the
table's alphabet is FOREIGN: it has no code, never merges, and must come out as its code point.  Everything is generated from a
fixed seed; nothing here reads a file outside the repository.  Needs a real MI355X: `-m gpu`."""
import ctypes
import random

import numpy as np
import pytest

from tests.test_gpu_lane_spans import IMPROPER, fill, make, nbytes
from tests.test_gpu_lane_taper import boundaries, cut, tile_map

pytestmark = pytest.mark.gpu

CAP = 640    # staged bytes per chunk of the narrow kernel: kNarrowCap
TILE = 512   # its largest tile: kNarrowTile
OPT_LANE_NARROW = 7   # SWT_OPT_LANE_NARROW (include/swt.h): 0 the library's choice, 1 never, 2 at every size and under a set taper
CONT = 0x80000000
FOREIGN = ("é", "ж", "😀")  # U+00E9 (below U+0400: the class copy's range), U+0436, U+1F600 (four bytes)


@pytest.fixture(scope="module")
def dev(native):
    if native.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests need an MI355X (there is no CPU fallback to test)")
    native.init(0)
    return native


def info(dev, h, which):
    fn = dev.lib().swt_debug_bpe_table_info
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]
    return fn(h._h, which)


def run(dev, tok, orc, texts, narrow=2, ask=True, ran=None):
    """one batch on the direct path in tiles (not the single workgroup) against the oracle; the kernel is the one the test means:
    narrow = what swt_debug_bpe_table_info 7 must say, ran = what 11 must say after the call (the narrow kernel unless narrow is
    0).  ask: the call asks for the narrow kernel at every size (and the handle
    goes back to the library's choice); otherwise the handle is taken as the test set it"""
    h = tok._table
    total = sum(nbytes(t) for t in texts)
    assert total > 1024 or len(texts) > 64
    oids, ooff = orc.tokenize_batch_ids(texts)
    h.set_option(dev.OPT_DEDUP, dev.DEDUP_NEVER)
    try:
        if ask:
            h.set_option(OPT_LANE_NARROW, 2)
        assert info(dev, h, 7) == narrow
        ids, off = tok.encode_ids_batch(texts)
        assert info(dev, h, 11) == ((1 if narrow else 0) if ran is None else ran), "the launch took the other kernel"
    finally:
        if ask:
            h.set_option(OPT_LANE_NARROW, 0)
        h.set_option(dev.OPT_DEDUP, dev.DEDUP_AUTO)
    assert np.array_equal(off, ooff), "offsets differ (%d sentences, %d bytes)" % (len(texts), total)
    assert np.array_equal(ids, oids), "ids differ (%d sentences, %d bytes)" % (len(texts), total)
    return ids, off


def tiled(texts):
    """65 sentences at least, so that a text of 1,024 bytes or less is not the single workgroup's"""
    return [""] * max(0, 65 - len(texts)) + texts


@pytest.fixture(scope="module")
def pre(swt, oracle, dev):
    """the first 8,000 pretrained merges (the benchmark's table) with words of its own corpus"""
    from subword_tokenizers_amd import synth

    tok, orc = make(swt, oracle, synth.pretrained_merges()[:8000])
    assert info(dev, tok._table, 8) == 1 and info(dev, tok._table, 7) == 1 and info(dev, tok._table, 9) == 45
    sents = synth.sentences_open(3000, 640512)
    words = sorted({w.lower() for s in sents for w in s.split() if w.isalpha()})
    short = [w for w in words if 2 <= len(w) <= 8][:400]
    multibyte = [w for w in words if nbytes(w) > len(w) and nbytes(w[0]) == 2][:100]
    cat = "".join(w for w in words if len(w) >= 6)
    return tok, orc, short, multibyte, cat


def test_chunk_and_tile_seams(dev, pre):
    """texts and sentence starts at CAP - 1 .. CAP + 1, 2 CAP +- 1 and TILE +- 1 bytes; a word across the cut; a word longer than
    a chunk (the one-lane walker); a word of 33 symbols (literal_rounds)"""
    tok, orc, short, multibyte, cat = pre
    rng = random.Random(640)
    sizes = (CAP - 1, CAP, CAP + 1, 2 * CAP - 1, 2 * CAP, 2 * CAP + 1, TILE - 1, TILE, TILE + 1)
    w33, w32, giant = cat[100:133], cat[200:232], cat[300:300 + CAP + 90]
    assert len(w33) == 33 and nbytes(giant) > CAP
    for n in sizes:
        # one sentence of n bytes: tile 0 owns it whole, in one chunk or in two
        run(dev, tok, orc, tiled([fill(short + multibyte, n, rng)]))
        # a sentence start ON byte n, in a text of three chunks
        for words in (short, short + multibyte):
            run(dev, tok, orc, [fill(words, n, rng), fill(words, 3 * CAP - n, rng)])
            run(dev, tok, orc, [fill(words, 7, rng), fill(words, n - 7, rng), fill(words, 5, rng), fill(words, 2 * CAP, rng)])
        # one word across the byte: it begins 1, 2, or all but one of its bytes before it
        for word in (cat[40:52], multibyte[0], w33):
            for back in (1, 2, nbytes(word) - 1):
                if n - back > 0:
                    run(dev, tok, orc, tiled([fill(short, n - back, rng) + word + " " + fill(short, CAP, rng)]))
    for lead in (0, 10, TILE - 3, CAP - 1, CAP + 5):
        run(dev, tok, orc, tiled([fill(short, lead, rng) + giant + " " + fill(short, 300, rng), fill(short, 90, rng)]))
        run(dev, tok, orc, tiled([fill(short, lead, rng) + w33 + " " + w32 + " " + w33 + w32 + " " + fill(short, 700, rng)]))
    # many tiles, sentences of every length, the library's own geometry (tiles of TILE bytes)
    sents, left = [], 40 * TILE + 77
    while left > 0:
        n = min(left, rng.choice((40, 90, 130, 260, 700, 1500)))
        sents.append(fill(short + multibyte + [w33, giant], n, rng) if n > CAP + 100 else fill(short + multibyte, n, rng))
        left -= n
    h = tok._table
    try:
        h.set_option(OPT_LANE_NARROW, 2)
        n_tiles, segs = tile_map(dev, h, 40 * TILE + 77)
        assert segs == [(0, 0, TILE)] and n_tiles == 41
        run(dev, tok, orc, sents, ask=False)
        # the library's own choice: the wide kernel's tiles under one chip-full of them (here a chip of 5 slots), the narrow
        # kernel's from there up
        h.set_option(OPT_LANE_NARROW, 0)
        h.set_option(dev.OPT_LANE_SLOTS, 5)
        assert info(dev, h, 7) == 1
        for n, tile in ((5 * 384 - 1, 384), (5 * 384, TILE), (5 * 384 + 1, TILE)):
            assert tile_map(dev, h, n)[1][0] == (0, 0, tile)  # (the narrow kernel's tiles taper from its floor up)
            run(dev, tok, orc, cut(fill(short + multibyte, n, rng).encode("utf-8"), range(60, n, 211)), narrow=1, ask=False, ran=1 if tile == TILE else 0)
    finally:
        h.set_option(OPT_LANE_NARROW, 0)
        h.set_option(dev.OPT_LANE_SLOTS, 0)


def test_foreign_code_points(dev, pre):
    """letters outside the alphabet in three ranges: alone, at the start, in the middle and at the end of a word, beside a
    merging pair, in a word of more than 32 symbols, as the last symbol before a cut, and at every place of a 64-byte block"""
    tok, orc, short, multibyte, cat = pre
    rng = random.Random(7)
    for f in FOREIGN:
        cp = ord(f)
        # the emitted id IS the code point
        ids, off = run(dev, tok, orc, tiled([f, f + " " + f, "ie" + f, f + "ie " + f + f]))
        ids = [int(x) for x in ids]
        ie = ids[-6]
        assert ie >= 0x110000 and ie & CONT == 0
        assert ids == [cp, cp, cp, ie, cp | CONT, cp, ie | CONT, cp, cp | CONT]
        words = [f, f + "nie", "nie" + f, "ni" + f + "e", "ie" + f + "ie", f + f, "po" + f + f + "cz", f + "a", "z" + f,
                 cat[500:520] + f + cat[520:535], f + cat[600:633], cat[700:733] + f, cat[800:815] + f + cat[815:831] + f + "ie"]
        assert max(len(w) for w in words) > 33
        # every word at every offset of a 64-byte block: a run of k bytes in front
        for w in words[:9]:
            run(dev, tok, orc, ["x" * k + " " + w + " ie" for k in range(66)])
        for n in (CAP - 1, CAP, CAP + 1, TILE, 2 * CAP + 1, 3000):
            run(dev, tok, orc, tiled([fill(short + words * 6, n, rng)]))
            # the last symbol before the cut: the word that ends on byte n - 1 ends with the foreign letter
            for w in ("nie" + f, f, cat[900:933] + f):
                run(dev, tok, orc, tiled([fill(short, n - nbytes(w) - 1, rng) + w + " " + fill(short + words, CAP, rng)]))
    mixed = ["".join(rng.choice(["ie", "na", "cz", "po"] + list(FOREIGN)) for _ in range(rng.choice((2, 5, 17, 40)))) for _ in range(300)]
    sents = cut(fill(short + mixed, 30 * TILE + 3, rng).encode("utf-8"), range(100, 30 * TILE, 331))
    run(dev, tok, orc, sents)


def synthetic(n_merges, alphabet):
    """all pairs (x, y) of the alphabet, then (xy, z): short strings, every merged symbol a new one, a proper table"""
    merges = [(x, y) for x in alphabet for y in alphabet]
    for x in alphabet:
        for y in alphabet:
            if len(merges) >= n_merges:
                break
            merges += [(x + y, z) for z in alphabet]
    assert len(merges) >= n_merges
    return merges[:n_merges]


def test_eligibility_edge(swt, oracle, dev):
    """letters + merges = 0x7FFD exactly takes the narrow kernel, one merge more the wide one, and so does a table that is not
    packed; all three agree with the oracle on one text"""
    alphabet = [chr(ord("a") + i) for i in range(26)] + list("ąćęłńóśźżαβγδε")
    a = len(alphabet)
    assert a == 40
    rng = random.Random(0x7FFD)
    words = ["".join(rng.choice(alphabet[:6] + alphabet[30:33]) for _ in range(rng.choice((1, 2, 3, 4, 7, 12, 35)))) for _ in range(200)]
    words += ["ab" + f + "abc" for f in FOREIGN] + ["q" * 40, "zzz", "εεε"]
    texts = cut(fill(words, 5 * TILE + 9, rng).encode("utf-8"), range(90, 5 * TILE, 207))
    for n, narrow, packed in ((0x7FFD - a, True, True), (0x7FFE - a, False, True), (65600, False, False)):
        tok, orc = make(swt, oracle, synthetic(n, alphabet))
        h = tok._table
        assert info(dev, h, 3) == n and info(dev, h, 1) == (1 if packed else 0)
        assert info(dev, h, 8) == (1 if narrow else 0) and info(dev, h, 9) == (a if narrow else 0)
        run(dev, tok, orc, texts, narrow=2 if narrow else 0)


def test_improper_table(swt, oracle, dev):
    """a table that is not proper: every word goes through literal_rounds, with 16-bit symbols and foreign letters among them"""
    tok, orc = make(swt, oracle, IMPROPER)
    assert info(dev, tok._table, 2) == 0 and info(dev, tok._table, 8) == 1
    rng = random.Random(512640)
    short = ["ab", "abc", "aaa", "aaaa", "cd", "xy", "abcabc", "bc", "aab", "xyxy", "żół", "żółżół", "óż", "łłł"]
    longs = ["abc" * 12, "a" * 40, "abcd" * 9, "aab" * 14, "abc" * 230]
    for f in FOREIGN + ("q",):
        foreign = [f, "ab" + f, f + "abc", "a" + f + "a", "aa" + f + "aab" + f, "abc" * 6 + f + "abc" * 6, f + "aab" * 12, "żó" + f + "ł"]
        ids, _ = run(dev, tok, orc, tiled([f + " ab" + f]))
        assert [int(x) for x in ids][0] == ord(f) and [int(x) for x in ids][-1] == ord(f) | CONT
        for n in (CAP - 1, CAP + 1, 2 * CAP, 4000):
            run(dev, tok, orc, tiled([fill(short + longs[:4] + foreign, n, rng)]))
        for w in foreign:
            run(dev, tok, orc, ["c" * k + " " + w + " ab" for k in range(66)])
    run(dev, tok, orc, cut(fill(short + longs, 20 * TILE, rng).encode("utf-8"), range(60, 20 * TILE, 173)))


def test_tapered_narrow_tiles(dev, pre):
    """SWT_OPT_LANE_NARROW = 2 with a set taper: the tiles fall from 512 over 256 and 192 to 128 bytes, every size occurs, and
    the arrays are those of tiles of one size; without it a set taper counts from 384, on the narrow kernel all the same (4,991
    bytes are more than a chip-full of tiles when the chip has 3 slots)"""
    tok, orc, short, multibyte, cat = pre
    h = tok._table
    rng = random.Random(512256)
    seen = set()
    try:
        h.set_option(OPT_LANE_NARROW, 2)
        for taper, slots in ((4, 1), (8, 2), (8, 3), (16, 5), (256 + 8, 3)):
            h.set_option(dev.OPT_LANE_TAPER, taper)
            h.set_option(dev.OPT_LANE_SLOTS, slots)
            n = TILE * (taper & ~256) * slots // 8 + 1300
            n_tiles, segs = tile_map(dev, h, n)
            assert segs[0] == (0, 0, TILE) and len(boundaries(n_tiles, segs)) == n_tiles
            seen.update(tb for _, _, tb in segs)
            text = fill(short + multibyte + [cat[50:83]], n, rng).encode("utf-8")
            edges = [fb for fb, _, _ in segs[1:]]
            a = run(dev, tok, orc, cut(text, range(70, n, 149)), ask=False)
            b = run(dev, tok, orc, cut(text, [e - 1 for e in edges] + [n // 3]), ask=False)
            h.set_option(dev.OPT_LANE_TAPER, 1)
            assert tile_map(dev, h, n) == ((n + TILE - 1) // TILE, [(0, 0, TILE)])
            for got, pts in ((a, range(70, n, 149)), (b, [e - 1 for e in edges] + [n // 3])):
                one = run(dev, tok, orc, cut(text, pts), ask=False)
                assert np.array_equal(one[0], got[0]) and np.array_equal(one[1], got[1])
        assert seen == {TILE, 256, 192, 128}, seen
        h.set_option(OPT_LANE_NARROW, 0)
        h.set_option(dev.OPT_LANE_TAPER, 8)
        h.set_option(dev.OPT_LANE_SLOTS, 3)
        assert tile_map(dev, h, 4991)[1][0] == (0, 0, 384)
        run(dev, tok, orc, cut(fill(short, 4991, rng).encode("utf-8"), range(70, 4991, 149)), narrow=1, ask=False)
        h.set_option(OPT_LANE_NARROW, 1)
        assert tile_map(dev, h, 4991)[1][0] == (0, 0, 384)
        run(dev, tok, orc, cut(fill(short, 4991, rng).encode("utf-8"), range(70, 4991, 149)), narrow=0, ask=False)
        for bad in (-1, 3):
            with pytest.raises(Exception):
                h.set_option(OPT_LANE_NARROW, bad)
    finally:
        h.set_option(OPT_LANE_NARROW, 0)
        h.set_option(dev.OPT_LANE_TAPER, 0)
        h.set_option(dev.OPT_LANE_SLOTS, 0)
    assert info(dev, h, 7) == 1


def test_naive_order_stays_on_the_wide_kernel(swt, dev):
    """a list that is not order-equivalent through swt_bpe_encode_naive*: the ordered form of the wide kernel, against the Python
    encode_word loop, foreign letters included -- on a table whose FastBPE order would take the narrow kernel"""
    tok = swt.NaiveBPE()
    tok.merges_list = list(IMPROPER) + [("a", "b"), ("ab", "ab")]
    h = tok._ensure_naive_table()
    assert not h.order_equivalent() and info(dev, h, 8) == 1
    rng = random.Random(33)
    short = ["ab", "abc", "aaa", "aaaa", "cd", "xy", "abcabc", "bc", "aab", "xyxy", "abab", "ababab", "abéab", "жab", "ab😀"]
    h.set_option(dev.OPT_DEDUP, dev.DEDUP_NEVER)
    try:
        for n in (CAP + 1, 2 * CAP - 1, 5000):
            words = fill(short, n, rng).split()
            sents = [" ".join(words[i:i + 11]) + " " for i in range(0, len(words), 11)]
            want = [sum((tok.encode_word(w) for w in s.split()), []) for s in sents]
            assert tok.tokenize_batch(tiled(sents)) == [[]] * max(0, 65 - len(sents)) + want, n
            assert info(dev, h, 11) == 0  # the ordered form is a wide kernel
    finally:
        h.set_option(dev.OPT_DEDUP, dev.DEDUP_AUTO)


def test_single_workgroup_and_dedup_calls(dev, pre):
    """the two forms that stay on the wide kernel: a 600-byte call of three sentences (one workgroup), and the unique-word pass of
    the dedup path at about 100 KB -- on a handle whose running text takes the narrow kernel"""
    tok, orc, short, multibyte, cat = pre
    h = tok._table
    assert info(dev, h, 7) == 1
    rng = random.Random(600)
    foreign = ["ie" + f + "na" for f in FOREIGN]
    texts = [fill(short + foreign, 250, rng), fill(short + multibyte, 200, rng), fill(short + foreign, 150, rng)]
    assert sum(nbytes(t) for t in texts) == 600
    oids, ooff = orc.tokenize_batch_ids(texts)
    ids, off = tok.encode_ids_batch(texts)
    assert np.array_equal(ids, oids) and np.array_equal(off, ooff)
    sents = cut(fill(short + multibyte + foreign + [cat[50:83]], 100 * 1024, rng).encode("utf-8"), range(80, 100 * 1024, 157))
    oids, ooff = orc.tokenize_batch_ids(sents)
    try:
        for mode in (dev.DEDUP_ALWAYS, dev.DEDUP_NEVER):
            h.set_option(dev.OPT_DEDUP, mode)
            ids, off = tok.encode_ids_batch(sents)
            assert np.array_equal(ids, oids) and np.array_equal(off, ooff), mode
        assert info(dev, h, 11) == 0  # 100 KB on the direct path: under the floor of the library's choice, the wide kernel
    finally:
        h.set_option(dev.OPT_DEDUP, dev.DEDUP_AUTO)
