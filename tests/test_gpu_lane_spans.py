"""The seams of a SPAN of the FastBPE direct path (csrc/swt_bpe_encode.hip) against the C oracle, ids and offsets exact.

A wave of bpe_lane_kernel's running-text form takes K consecutive 384-byte tiles as one span and walks it in 512-byte chunks; plan,
scan and gather work per span.  The library's own K is 1 (profiles/lane_spans.txt: longer spans measured slower); SWT_OPT_LANE_SPAN
sets it, and every construction here runs under K = 1, 2, 3, 4 and 8 and under the library's own choice.  The inputs put a seam wherever a span can break: a sentence longer
than a span and than several chunks, a multi-byte character and a word across a tile boundary inside a span and across the span
boundary, tiles without a sentence start inside a span and at its end, a tile count that is no multiple of K (the last span
shorter), and batches of one and of 65 sentences just above the single-workgroup limit (1,024 bytes / 64 sentences).
Everything is generated from a fixed seed; nothing here reads a file outside the repository.  Needs a real MI355X: `-m gpu`."""
import ctypes
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CAP = 512     # staged bytes per chunk: SWT_LANE_CAP (tests/test_gpu_lane_pipeline.py pins both against the source)
TILE = 384    # bytes of sentence starts per tile: SWT_LANE_TILE
SPANS = (1, 2, 3, 4, 8, 0)  # 0 last: the library's own choice, which is also what the handle is left with

# not proper: (ab, c) ranks BELOW the merge that makes ab, and (aa, a) below (a, a): every word goes through literal_rounds
IMPROPER = [("ab", "c"), ("a", "b"), ("aa", "a"), ("a", "a"), ("c", "d"), ("x", "y"), ("b", "c"), ("ż", "ó"), ("żó", "ł")]


@pytest.fixture(scope="module")
def dev(native):
    if native.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests need an MI355X (there is no CPU fallback to test)")
    native.init(0)
    return native


def make(swt, oracle, merges):
    tok = swt.FastBPE()
    tok.merges_list = list(merges)
    tok._build_table()
    return tok, oracle.OracleBPE(tok.merges_list)


def nbytes(t):
    return len(t.encode("utf-8"))


def check(dev, tok, orc, texts):
    """the direct path under every span length against the oracle"""
    total = sum(nbytes(t) for t in texts)
    assert total > 1024 or len(texts) > 64  # not the single-workgroup call
    oids, ooff = orc.tokenize_batch_ids(texts)
    h = tok._table
    try:
        h.set_option(dev.OPT_DEDUP, dev.DEDUP_NEVER)
        for k in SPANS:
            h.set_option(dev.OPT_LANE_SPAN, k)
            ids, off = tok.encode_ids_batch(texts)
            assert np.array_equal(off, ooff), "offsets differ (span %d, %d sentences, %d bytes)" % (k, len(texts), total)
            assert np.array_equal(ids, oids), "ids differ (span %d, %d sentences, %d bytes)" % (k, len(texts), total)
    finally:
        h.set_option(dev.OPT_LANE_SPAN, 0)
        h.set_option(dev.OPT_DEDUP, dev.DEDUP_AUTO)


def fill(words, n_bytes, rng):
    """words separated by single spaces, n_bytes of UTF-8 exactly (ends with a space; 'q' runs make up the remainder)"""
    out = []
    left = n_bytes
    while left > 0:
        w = rng.choice(words)
        b = nbytes(w) + 1
        if b > left:
            w = "q" * (left - 1)
            b = left
        out.append(w)
        left -= b
    return " ".join(out) + " " if out else ""


def span_batches(rng, short, longs, multibyte):
    """lists of sentences; byte positions are absolute in the batch, so each list is encoded on its own"""
    batches = []
    mb = multibyte[0]
    lw = longs[0]
    for k in (1, 2, 3, 4, 8):
        span = k * TILE
        # a word and a multi-byte character across every tile boundary of three spans (the boundaries inside a span and the
        # two between spans), the sentence boundaries elsewhere: pieces of TILE bytes whose last word straddles the boundary
        for straddler in (lw, mb, mb[0]):
            for back in (1, 2, nbytes(straddler) - 1):
                if back < 1:
                    continue
                text = ""
                while nbytes(text) < 3 * span:
                    t_end = (nbytes(text) // TILE + 1) * TILE
                    text += fill(short, t_end - nbytes(text) - back, rng) + straddler + " "
                sents, pos = [], 0
                for cut in (150, 500, span + 7, 2 * span - 90, 2 * span + 300):
                    i = text.find(" ", cut) + 1
                    if i > pos:
                        sents.append(text[pos:i])
                        pos = i
                sents.append(text[pos:])
                batches.append(sents)
        # a sentence longer than a span and longer than several chunks, after short ones and before short ones; its start in
        # the first, a middle and the last tile of a span
        for lead in (10, TILE + 5, span - 9, span + 1):
            batches.append([fill(short, lead, rng), fill(short + longs, 2 * span + 3 * CAP + 11, rng), fill(short, 60, rng),
                            fill(short, 2 * span, rng)] + [fill(short, 90, rng) for _ in range(9)])
        # tiles without a sentence start: inside a span (a sentence of 2.5 tiles from the span's first tile), a whole span of
        # them, and at the end of the last span (the batch ends with a sentence of several tiles)
        batches.append([fill(short, 20, rng), fill(short, 2 * TILE + TILE // 2, rng)] + [fill(short, 70, rng) for _ in range(12)] +
                       [fill(short, 2 * span + 40, rng), fill(short, 33, rng), fill(short + longs, 3 * TILE + 1, rng)])
        # the tile count around a multiple of K: the last span full, one tile short, one tile over, and a last span of one byte
        for tiles in (2 * k, 2 * k + 1, 3 * k - 1, 3 * k):
            for d in (-1, 0, 1):
                total = max(tiles * TILE + d, 1100)
                sents, left = [], total
                while left > 0:
                    n = min(left, rng.choice((40, 90, 130, 260, 700)))
                    sents.append(fill(short + multibyte, n, rng))
                    left -= n
                batches.append(sents)
    # one sentence and 65 sentences just above the single-workgroup limit (1,024 bytes and 64 sentences)
    for n in (1025, 1026, 1040, 1024 + TILE, 3 * CAP):
        batches.append([fill(short + longs[:1] + multibyte, n, rng)])
    batches.append([fill(short, 3, rng) for _ in range(65)])
    batches.append([fill(short + multibyte, 16, rng) for _ in range(64)] + [""])
    batches.append([""] * 30 + [fill(short, 9, rng) for _ in range(35)])
    batches.append([fill(short, 15, rng) for _ in range(64)] + [fill(short + longs, 2000, rng)])
    return batches


def test_span_seams_improper_table(swt, oracle, dev):
    """a hand-made improper table: every word of every span goes through literal_rounds"""
    tok, orc = make(swt, oracle, IMPROPER)
    lib = dev.lib()
    lib.swt_debug_bpe_table_info.restype = ctypes.c_int
    lib.swt_debug_bpe_table_info.argtypes = [ctypes.c_void_p, ctypes.c_int]
    assert lib.swt_debug_bpe_table_info(tok._table._h, 2) == 0  # not proper
    short = ["ab", "abc", "aaa", "aaaa", "cd", "xy", "abcabc", "bc", "aab", "xyxy"]
    longs = ["abc" * 9, "a" * 31, "abcd" * 9, "aab" * 14]
    multibyte = ["żół", "żółżół", "óż", "łłł"]
    rng = random.Random(384512)
    for sents in span_batches(rng, short, longs, multibyte):
        check(dev, tok, orc, sents)


@pytest.mark.parametrize("n_merges", [8000, None])
def test_span_seams_pretrained(swt, oracle, dev, n_merges):
    """the pretrained merges at 8,000 (packed table values) and in full, on the constructed seams and on running text"""
    from subword_tokenizers_amd import synth

    merges = synth.pretrained_merges()
    tok, orc = make(swt, oracle, merges if n_merges is None else merges[:n_merges])
    rng = random.Random(85384)
    sents = synth.sentences_open(4000, 2424)
    words = sorted({w.lower() for s in sents for w in s.split() if w.isalpha()})
    short = [w for w in words if 2 <= len(w) <= 8][:400]
    multibyte = [w for w in words if nbytes(w) > len(w)][:100]
    cat = "".join(w for w in words if len(w) >= 6)
    longs = [cat[i * 37: i * 37 + n] for i, n in enumerate((25, 30, 32, 33, 41))]
    for batch in span_batches(rng, short, longs, multibyte):
        check(dev, tok, orc, batch)
    # running text: sentences as they come (a tile count that is no multiple of any K but 1), joined thirty at a time (every
    # sentence longer than a span of eight), and one sentence of half the text first
    check(dev, tok, orc, sents)
    check(dev, tok, orc, [" ".join(sents[i:i + 30]) for i in range(0, len(sents), 30)])
    check(dev, tok, orc, [" ".join(sents[:2000])] + sents[2000:])


def test_span_option_is_validated(swt, dev):
    tok = swt.FastBPE()
    tok.merges_list = [("a", "b")]
    tok._build_table()
    for bad in (-1, 17, 384):
        with pytest.raises(Exception):
            tok._table.set_option(dev.OPT_LANE_SPAN, bad)
    tok._table.set_option(dev.OPT_LANE_SPAN, 16)
    tok._table.set_option(dev.OPT_LANE_SPAN, 0)
