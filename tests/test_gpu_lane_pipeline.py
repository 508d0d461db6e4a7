"""The seams between the chunks of a bpe_lane_kernel tile (csrc/swt_bpe_encode.hip) against the C oracle, ids and offsets exact.

The kernel takes one 512-byte chunk of its tile after the other (a form that overlapped them is described in
profiles/lane_pipeline.txt).  The inputs put a seam wherever chunking can break: a long word last in
its chunk, chunks that are finished at once or have nothing to merge, a word longer than a chunk between two ordinary chunks,
sentence boundaries and multi-byte characters at the cut, tiles of exactly K chunks and of one byte more.  Where a chunk is cut
depends on the 16-byte alignment of its first byte and on the word boundaries before byte 512, so every construction is swept
over a range of paddings: some padding puts the interesting word last in its chunk, the next one first in the following chunk.
Everything is generated from a fixed seed and the pretrained merges (synth.pretrained_merges); nothing here reads a file outside
the repository.  Needs a real MI355X: `-m gpu`."""
import os
import random
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CAP = 512     # staged bytes per chunk: SWT_LANE_CAP of csrc/swt_bpe_encode.hip
TILE = 384    # bytes of sentence starts per tile: SWT_LANE_TILE


def test_constants_are_the_kernels():
    """the seams below sit where these two say; if the kernel's constants move, this file has to move with them"""
    src = open(os.path.join(ROOT, "subword-tokenizers_amd", "csrc", "swt_bpe_encode.hip"), encoding="utf-8").read()
    assert int(re.search(r"#define SWT_LANE_CAP (\d+)", src).group(1)) == CAP
    assert int(re.search(r"#define SWT_LANE_TILE (\d+)", src).group(1)) == TILE


# proper: every pair ranks above the merges that make its symbols; long words take many rounds (the chain ab, cd, abcd, ...)
PROPER = [("a", "b"), ("c", "d"), ("ab", "cd"), ("e", "e"), ("ee", "e"), ("abcd", "ab"), ("x", "y"), ("xy", "xy"),
          ("ab", "ab"), ("d", "a"), ("ż", "ó"), ("żó", "ł"), ("b", "c"), ("abcdab", "cd"), ("y", "x"), ("abcd", "abcd"),
          ("abcdabcd", "abcdabcd")]
# not proper: (ab, c) ranks BELOW the merge that makes ab, and (aa, a) below (a, a): every word goes through literal_rounds
IMPROPER = [("ab", "c"), ("a", "b"), ("aa", "a"), ("a", "a"), ("c", "d"), ("x", "y"), ("b", "c")]


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


def check(dev, tok, orc, texts):
    """the direct path (the running-text form of the kernel) and the dedup path (its unique-word form) against the oracle"""
    assert sum(len(t.encode("utf-8")) for t in texts) > 1024 or len(texts) > 64  # not the single-workgroup call
    oids, ooff = orc.tokenize_batch_ids(texts)
    h = tok._table
    try:
        for mode in (dev.DEDUP_NEVER, dev.DEDUP_ALWAYS):
            h.set_option(dev.OPT_DEDUP, mode)
            ids, off = tok.encode_ids_batch(texts)
            assert np.array_equal(off, ooff), "offsets differ (dedup mode %d)" % mode
            assert np.array_equal(ids, oids), "ids differ (dedup mode %d)" % mode
    finally:
        h.set_option(dev.OPT_DEDUP, dev.DEDUP_AUTO)


def fill(words, n_bytes, rng):
    """words separated by single spaces, n_bytes of UTF-8 exactly (ends with a space; 'q' runs make up the remainder)"""
    out = []
    left = n_bytes
    while left > 0:
        w = rng.choice(words)
        b = len(w.encode("utf-8")) + 1
        if b > left:
            w = "q" * (left - 1)
            b = left
        out.append(w)
        left -= b
    return " ".join(out) + " " if out else ""


def long_words(unit, lengths):
    return [(unit * (n // len(unit) + 1))[:n] for n in lengths]


def seam_texts(rng, short, longs, multibyte, giant_unit):
    """short: words of 2-8 symbols that merge; longs: words of 25-32 and of 33+ symbols; multibyte: words of 2-byte characters"""
    singles = ["q", "r", "s", "t"]  # no merge has them: single-symbol words, nothing for the rounds
    texts = []
    pads = list(range(0, 48, 3)) + [64, 127, 128, 129, 191]
    for pad in pads:
        for lw in longs:
            # a long word LAST in chunk k (a pipeline would still be merging it when chunk k+1 -- short words only, done in two or
            # three rounds -- is split, and again when chunk k+2 wants a buffer); the same word once more at the tile's end
            head = fill(short, CAP - 32 - pad - len(lw.encode("utf-8")), rng)
            texts.append(head + lw + " " + fill(short[:2], CAP - 24, rng) + fill(short, CAP + 40, rng) + lw)
            # ... with nothing at all for the rounds in chunk k+1, and with fewer multi-symbol words than the threshold in chunk k
            texts.append(fill(singles, CAP - 32 - pad - len(lw.encode("utf-8")), rng) + lw + " " + fill(singles, CAP + 60, rng) + fill(short, 300, rng) + lw)
        # a chunk whose words all finish before the threshold, then a dense one
        texts.append(fill(singles, 400 + pad, rng) + " ".join(short[:5]) + " " + fill(short, 2 * CAP, rng))
        # a giant word (longer than the chunk) between two ordinary chunks, with long words merging before it
        giant = (giant_unit * (2 * CAP))[: CAP + 100 + pad]
        texts.append(fill(short, 300 + pad, rng) + longs[0] + " " + giant + " " + fill(short, CAP, rng) + longs[-1] + " " + giant)
        # multi-byte characters across the cut
        texts.append(fill(multibyte, 470 + pad, rng) + fill(multibyte + short, 3 * CAP, rng))
    # a sentence boundary exactly at a chunk cut: runs of sentences whose lengths walk round the chunk size
    for pad in range(0, 34):
        texts += [fill(short, CAP - 17 + pad, rng), fill(short + longs[:1], CAP - 16, rng), fill(short, 7 + pad, rng)]
    # tiles of exactly K chunks, and of K chunks + 1 byte: one sentence each (a tile is whole sentences), in tile units and in chunks
    for k in (2, 4):
        for unit in (TILE, CAP, CAP - 16):
            for d in (-1, 0, 1):
                texts.append(fill(short + longs[:1], k * unit + d, rng))
                texts.append(fill(short, k * unit + d - len(longs[1].encode("utf-8")), rng) + longs[1])
    return texts


def test_pipeline_seams_handmade_tables(swt, oracle, dev):
    """the proper table (one occurrence of the best pair per round) and the improper one (every word through literal_rounds)"""
    short = ["ab", "cd", "abcd", "xyxy", "eee", "abab", "abcdabcd", "da", "xyx"]
    longs = long_words("abcd", (25, 28, 31, 32)) + long_words("abcd", (33, 40, 64)) + ["e" * 32, "xy" * 16, "xy" * 17]
    multibyte = ["żół", "żółżół", "óż", "łłł"]
    for merges in (PROPER, IMPROPER):
        tok, orc = make(swt, oracle, merges)
        rng = random.Random(20240607)
        texts = seam_texts(rng, short, longs, multibyte, "abcdabcdab")
        check(dev, tok, orc, texts)
        rng.shuffle(texts)  # other neighbours, other alignments
        check(dev, tok, orc, texts)
        check(dev, tok, orc, [" ".join(texts[:40])] + texts[40:])  # one sentence of ~100 chunks first


@pytest.mark.parametrize("n_merges", [8000, None])
def test_pipeline_seams_pretrained(swt, oracle, dev, n_merges):
    """the pretrained merges at 8,000 (packed table values) and in full, on constructed seams and on running text in long sentences"""
    from subword_tokenizers_amd import synth

    merges = synth.pretrained_merges()
    tok, orc = make(swt, oracle, merges if n_merges is None else merges[:n_merges])
    rng = random.Random(85000)
    sents = synth.sentences_open(3000, 4242)
    words = sorted({w.lower() for s in sents for w in s.split() if w.isalpha()})
    short = [w for w in words if 2 <= len(w) <= 8][:400]
    multibyte = [w for w in words if len(w.encode("utf-8")) > len(w)][:100]
    cat = "".join(w for w in words if len(w) >= 6)
    longs = [cat[i * 37: i * 37 + n] for i, n in enumerate((25, 27, 30, 32, 33, 41, 70))]
    texts = seam_texts(rng, short, longs, multibyte, cat[:257])
    check(dev, tok, orc, texts)
    # running text: sentences as they come, then joined ten at a time (every tile spans several chunks), then one sentence of all
    check(dev, tok, orc, sents)
    check(dev, tok, orc, [" ".join(sents[i:i + 10]) for i in range(0, len(sents), 10)])
    check(dev, tok, orc, [" ".join(sents[:1500])] + sents[1500:])
