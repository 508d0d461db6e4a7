"""The seams of TAPERING tiles on the FastBPE / NaiveBPE direct path (csrc/swt_bpe_encode.hip: lane_map, csrc/swt_tilemap.h) against the C
oracle, ids and offsets exact.

The running-text form of bpe_lane_kernel takes its tile from plan[t] and plan[t + 1]; the plan is cut by a tile map whose tiles
fall from 384 over 256 and 192 to 128 bytes towards the end of the text (the tile at byte x is the largest size that is no more
than the bytes still to come / (c x wave slots)).  SWT_OPT_LANE_TAPER sets c (v = 8 c), SWT_OPT_LANE_SLOTS pretends the chip has
1, 2, 3 or 5 slots, so that texts of 1.1 to 8 KB walk through every size with one to a few tiles each.  Every text is built to an
exact byte count, the map of that count is read back from the library (swt_debug_bpe_tile_map), and the seams are put where it
says the size changes.  Every call is repeated with tiles of one size (taper 1), which must give the same arrays.
Everything is generated from a fixed seed; nothing here reads a file outside the repository.  Needs a real MI355X: `-m gpu`."""
import ctypes
import random

import numpy as np
import pytest

from tests.test_gpu_lane_spans import IMPROPER, fill, make, nbytes

pytestmark = pytest.mark.gpu

TAPERS = (4, 8, 16)   # c = 0.5, 1, 2
SLOTS = (1, 2, 3, 5)
SIZES = (384, 256, 192, 128)


@pytest.fixture(scope="module")
def dev(native):
    if native.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests need an MI355X (there is no CPU fallback to test)")
    native.init(0)
    return native


def tile_map(dev, h, n_bytes):
    """(tiles, [(first byte, first tile, tile bytes)]) of a running-text call of n_bytes under the handle's options"""
    fn = dev.lib().swt_debug_bpe_tile_map
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
    m = (ctypes.c_uint64 * 13)()
    assert fn(h._h, n_bytes, m) == 0
    return int(m[0]), [(int(m[1 + 3 * k]), int(m[2 + 3 * k]), int(m[3 + 3 * k])) for k in range(4) if m[3 + 3 * k]]


def boundaries(n_tiles, segs):
    out = []
    for k, (fb, ft, tb) in enumerate(segs):
        end = segs[k + 1][1] if k + 1 < len(segs) else n_tiles
        out += [fb + (t - ft) * tb for t in range(ft, end)]
    return out


class Setting:
    """taper and slots on a handle; the handle goes back to its defaults"""

    def __init__(self, dev, h):
        self.dev, self.h = dev, h

    def __enter__(self):
        self.h.set_option(self.dev.OPT_DEDUP, self.dev.DEDUP_NEVER)
        return self

    def set(self, taper, slots):
        self.h.set_option(self.dev.OPT_LANE_TAPER, taper)
        self.h.set_option(self.dev.OPT_LANE_SLOTS, slots)

    def __exit__(self, *exc):
        self.set(0, 0)
        self.h.set_option(self.dev.OPT_DEDUP, self.dev.DEDUP_AUTO)


def cut(text, points):
    """bytes -> sentences (str) cut behind the first space at or after each point: their bytes joined are the text"""
    sents, pos = [], 0
    for p in sorted(points):
        i = text.find(b" ", p) + 1
        if i > pos:
            sents.append(text[pos:i])
            pos = i
    sents.append(text[pos:])
    assert b"".join(sents) == text
    return [s.decode("utf-8") for s in sents]


def seam_text(n, edges, straddler, back, words, rng):
    """n bytes exactly; `straddler` begins `back` bytes before every edge it fits at"""
    out = b""
    sb = straddler.encode("utf-8") + b" "
    for p in edges:
        start = p - back
        if start < len(out) or start + len(sb) > n:
            continue
        out += fill(words, start - len(out), rng).encode("utf-8") + sb
    out += fill(words, n - len(out), rng).encode("utf-8")
    assert len(out) == n
    return out


def run(dev, st, tok, orc, texts, taper, slots, seen=None):
    """one batch under (taper, slots) and under tiles of one size against the oracle; returns the map it ran under"""
    total = sum(nbytes(t) for t in texts)
    assert total > 1024 or len(texts) > 64  # not the single-workgroup call
    oids, ooff = orc.tokenize_batch_ids(texts)
    got = []
    for tp in (taper, 1):
        st.set(tp, slots)
        ids, off = tok.encode_ids_batch(texts)
        assert np.array_equal(off, ooff), "offsets differ (taper %d, slots %d, %d sentences, %d bytes)" % (tp, slots, len(texts), total)
        assert np.array_equal(ids, oids), "ids differ (taper %d, slots %d, %d sentences, %d bytes)" % (tp, slots, len(texts), total)
        got.append((ids, off))
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])
    st.set(taper, slots)
    n_tiles, segs = tile_map(dev, tok._table, total)
    if seen is not None:
        seen.update(tb for _, _, tb in segs)
    return n_tiles, segs


def seam_suite(dev, tok, orc, short, longs, multibyte, seed):
    rng = random.Random(seed)
    h = tok._table
    seen, most_segs, second_chunks = set(), 0, 0
    stradd = [(longs[0], b) for b in (1, 2, nbytes(longs[0]) - 1)] + [(multibyte[0], b) for b in (1, 2, nbytes(multibyte[0]) - 1)] + \
             [(multibyte[0][0], 1)]  # a two-byte character alone: the edge between its bytes
    assert nbytes(multibyte[0][0]) == 2
    with Setting(dev, h) as st:
        for taper in TAPERS:
            for slots in SLOTS:
                k8 = taper * slots  # c x slots in eighths
                for n in (min(8192, max(1100, 384 * k8 // 8 + 997)), min(8192, max(1100, 384 * k8 // 8 + 997 + 211))):
                    st.set(taper, slots)
                    n_tiles, segs = tile_map(dev, h, n)
                    most_segs = max(most_segs, len(segs))
                    bnd = boundaries(n_tiles, segs)
                    assert len(bnd) == n_tiles and bnd[0] == 0 and bnd[-1] < n
                    edges = [fb for fb, _, _ in segs[1:]]
                    for i, (word, back) in enumerate(stradd):
                        text = seam_text(n, edges, word, back, short + multibyte, rng)
                        # sentence boundaries elsewhere, short sentences
                        pts, p = [], 0
                        while p < n:
                            p += rng.choice((40, 90, 130, 260))
                            pts.append(p)
                        assert run(dev, st, tok, orc, cut(text, pts), taper, slots, seen) == (n_tiles, segs)
                        if i % 3 == 0:
                            # a sentence that starts in one segment and ends two segments later (or at the end of the text)
                            a = segs[0][0] + 50
                            b = segs[2][0] + segs[2][2] + 9 if len(segs) > 2 else n - 40
                            run(dev, st, tok, orc, cut(text, [20, a, b] + [q for q in pts if q > b]), taper, slots)
                        if i % 3 == 1:
                            # tiles without a sentence start on both sides of every size change
                            pts2 = []
                            for k in range(1, len(segs)):
                                pts2 += [segs[k][0] - 2 * segs[k - 1][2] - 30, segs[k][0] + 2 * segs[k][2] + 5]
                            run(dev, st, tok, orc, cut(text, [q for q in pts2 if 0 < q < n]), taper, slots)
                        if i % 3 == 2 and segs[-1][2] == 128 and n - segs[-1][0] > 700:
                            # a sentence longer than a chunk (512 B) that begins in a 128-byte tile: a second chunk in the taper
                            a = segs[-1][0] + 20
                            second_chunks += 1
                            run(dev, st, tok, orc, cut(text, [q for q in pts if q < a - 140] + [a - 1, a + 560]), taper, slots)
        assert seen == set(SIZES) and most_segs == 4 and second_chunks >= 3, (seen, most_segs, second_chunks)

        # a segment of exactly zero tiles (a size the map skips), and a last tile of one byte
        found_skip = found_one = None
        for taper in TAPERS:
            for slots in SLOTS:
                st.set(taper, slots)
                for n in range(1100, 2600):
                    n_tiles, segs = tile_map(dev, h, n)
                    sizes = [tb for _, _, tb in segs]
                    if found_skip is None and len(segs) >= 2 and any(SIZES.index(b) - SIZES.index(a) > 1 for a, b in zip(sizes, sizes[1:])):
                        found_skip = (taper, slots, n)
                    if found_one is None and len(segs) >= 2 and boundaries(n_tiles, segs)[-1] == n - 1:
                        found_one = (taper, slots, n)
                if found_skip and found_one:
                    break
        assert found_skip and found_one
        for taper, slots, n in (found_skip, found_one):
            text = fill(short + multibyte + longs, n, rng).encode("utf-8")
            run(dev, st, tok, orc, cut(text, range(70, n, 97)), taper, slots)
            run(dev, st, tok, orc, cut(text, [n // 2]), taper, slots)

        # a text shorter than 128 x c x slots: every tile is the smallest
        n_tiles, segs = run(dev, st, tok, orc, cut(fill(short + longs, 1200, rng).encode("utf-8"), range(50, 1200, 61)), 16, 5)
        assert segs == [(0, 0, 128)] and n_tiles == 10
        # 1,025 bytes in one sentence, just over the single-workgroup limit; 65 sentences of 3 bytes
        for taper, slots in ((4, 1), (8, 2), (16, 5)):
            run(dev, st, tok, orc, [fill(short + longs[:1] + multibyte, 1025, rng)], taper, slots)
            run(dev, st, tok, orc, [fill(short, 3, rng) for _ in range(65)], taper, slots)
        # 3,000 empty sentences in front of 2 KB of text: more than 256 sentences per tile, the binary-search plan_kernel
        for taper, slots in ((4, 1), (8, 1), (4, 2)):
            body = cut(fill(short + multibyte, 2048, rng).encode("utf-8"), range(100, 2048, 83))
            n_tiles, segs = run(dev, st, tok, orc, [""] * 3000 + body, taper, slots)
            assert (3000 + len(body)) // 256 > n_tiles and len(segs) >= 2
            run(dev, st, tok, orc, body[:3] + [""] * 3000 + body[3:], taper, slots)


def test_taper_seams_improper_table(swt, oracle, dev):
    """a hand-made improper table: every word goes through literal_rounds"""
    tok, orc = make(swt, oracle, IMPROPER)
    short = ["ab", "abc", "aaa", "aaaa", "cd", "xy", "abcabc", "bc", "aab", "xyxy"]
    longs = ["abc" * 9, "a" * 31, "abcd" * 9, "aab" * 14]
    multibyte = ["żół", "żółżół", "óż", "łłł"]
    seam_suite(dev, tok, orc, short, longs, multibyte, 128384)


@pytest.mark.parametrize("n_merges", [8000, None])
def test_taper_seams_pretrained(swt, oracle, dev, n_merges):
    """the pretrained merges at 8,000 (packed table values) and in full"""
    from subword_tokenizers_amd import synth

    merges = synth.pretrained_merges()
    tok, orc = make(swt, oracle, merges if n_merges is None else merges[:n_merges])
    sents = synth.sentences_open(4000, 2424)
    words = sorted({w.lower() for s in sents for w in s.split() if w.isalpha()})
    short = [w for w in words if 2 <= len(w) <= 8][:400]
    multibyte = [w for w in words if nbytes(w) > len(w) and nbytes(w[0]) == 2][:100]
    cat = "".join(w for w in words if len(w) >= 6)
    longs = [cat[i * 37: i * 37 + n] for i, n in enumerate((25, 30, 32, 33, 41))]
    seam_suite(dev, tok, orc, short, longs, multibyte, 85128)


def test_taper_naive_bpe_ordered_form(swt, dev):
    """NaiveBPE shares the direct path and gets the same map: the ordered form of the kernel (a list with a repeated pair) under
    tapering tiles against tiles of one size and against the Python encode_word loop"""
    tok = swt.NaiveBPE()
    tok.merges_list = list(IMPROPER) + [("a", "b"), ("ab", "ab")]
    h = tok._ensure_naive_table()
    assert not h.order_equivalent()
    rng = random.Random(192256)
    short = ["ab", "abc", "aaa", "aaaa", "cd", "xy", "abcabc", "bc", "aab", "xyxy", "abab", "ababab"]
    with Setting(dev, h) as st:
        for taper, slots, n in ((4, 1, 1189), (8, 3, 2400), (16, 5, 4837), (16, 5, 1200)):
            words = fill(short, n, rng).split()
            sents, i = [], 0
            while i < len(words):
                k = rng.choice((3, 9, 25, 80))
                sents.append(" ".join(words[i:i + k]) + " ")
                i += k
            want = [sum((tok.encode_word(w) for w in s.split()), []) for s in sents]
            got = []
            for tp in (taper, 1):
                st.set(tp, slots)
                got.append(tok.encode_ids_batch(sents))
                assert tok.tokenize_batch(sents) == want, (tp, slots, n)
            assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])


def test_taper_options_are_validated(swt, dev):
    tok = swt.FastBPE()
    tok.merges_list = [("a", "b")]
    tok._build_table()
    h = tok._table
    default = tile_map(dev, h, 5000000)
    for bad in (-1, 65, 255, 256, 257, 256 + 65, 1000):
        with pytest.raises(Exception):
            h.set_option(dev.OPT_LANE_TAPER, bad)
    for bad in (-1, (1 << 20) + 1):
        with pytest.raises(Exception):
            h.set_option(dev.OPT_LANE_SLOTS, bad)
    assert tile_map(dev, h, 5000000) == default  # a refused value changes nothing
    for ok in (1, 2, 64, 258, 320):
        h.set_option(dev.OPT_LANE_TAPER, ok)
    h.set_option(dev.OPT_LANE_SLOTS, 1 << 20)
    h.set_option(dev.OPT_LANE_SLOTS, 3)
    h.set_option(dev.OPT_LANE_TAPER, 8)
    assert tile_map(dev, h, 5000000) != default
    # c x slots = 3: ten tiles of 384 (1,151 bytes are left: under 1,152), two of 256 (639: under 768), one of 192 (447: under 576)
    assert tile_map(dev, h, 4991) == (17, [(0, 0, 384), (3840, 10, 256), (4352, 12, 192), (4544, 13, 128)])
    h.set_option(dev.OPT_LANE_TAPER, 1)
    assert tile_map(dev, h, 5000) == ((5000 + 383) // 384, [(0, 0, 384)])
    h.set_option(dev.OPT_LANE_TAPER, 8)
    h.set_option(dev.OPT_LANE_SPAN, 2)  # a span keeps its tiles of one size
    assert tile_map(dev, h, 5000) == ((5000 + 767) // 768, [(0, 0, 768)])
    h.set_option(dev.OPT_LANE_SPAN, 0)
    h.set_option(dev.OPT_LANE_TAPER, 0)
    h.set_option(dev.OPT_LANE_SLOTS, 0)
    assert tile_map(dev, h, 5000000) == default  # 0 restores the library's choice
