"""The split's lane masks and the narrow table's hash pair of the FastBPE running-text kernel (csrc/swt_bpe_encode.hip: lane_split,
lane_ballot / lane_bit / lanes_below, slot_value; csrc/swt_bpe_narrow.h: narrow_hash) against the C oracle, ids and offsets exact.

The split forms every mask of a 64-byte block from one vector compare and combines them as scalars: the bytes inside the chunk as
one range compare, the class masks from the class bits where they lie, the symbols that have a successor by a carry through the
bit-reversed masks, a word's first symbol from the word list.  What can go wrong there is a lane at an edge: device text at every
offset from 16-byte alignment, a staged end at every residue of 64, words that begin or end in lanes 0, 62 and 63, a pair across a
block boundary (also behind a FOREIGN symbol, and not across a sentence start), sentence starts on the first and the last byte of
a block, a block of whitespace only, a multi-byte character whose bytes run past the staged ones, runs of punctuation.  The mask
cases run through the narrow kernel and once more through the wide one, which compiles the same split.

The table of the 16-bit codes has a hash pair of its own: both slots from one multiply chain, addresses as a scalar base and a
32-bit offset.  Its cases: every ordered pair of 90 letters as a merge (every pair of the text hits, every pair of a round
misses; the builder doubles that table twice), a table whose merged codes are read from memory (the Seq = false kernel), an
improper table (literal_rounds), and a word longer than a chunk, which the one-lane walker merges over the WIDE table.

Every call through run() asks for the kernel it means and asserts that the launch took it (swt_debug_bpe_table_info 11).  All
texts are built from a fixed seed; nothing here reads a file outside the repository.  Needs a real MI355X: `-m gpu`."""
import random

import numpy as np
import pytest

from tests.test_gpu_lane_keys import REPEATED
from tests.test_gpu_lane_narrow import CAP, FOREIGN, OPT_LANE_NARROW, dev, info, pre, run, tiled  # noqa: F401  (dev, pre: fixtures)
from tests.test_gpu_lane_spans import IMPROPER, fill, make, nbytes

pytestmark = pytest.mark.gpu


def both(dev, tok, orc, texts):
    """the narrow kernel, then the wide one over the same split"""
    out = run(dev, tok, orc, texts)
    h = tok._table
    try:
        h.set_option(OPT_LANE_NARROW, 1)
        run(dev, tok, orc, texts, narrow=0, ask=False)
    finally:
        h.set_option(OPT_LANE_NARROW, 0)
    return out


def test_device_text_alignment(dev, pre):
    """the device call with its text 0..15 bytes past a 16-byte boundary: the chunks are staged from the aligned address below"""
    import torch

    tok, orc, short, multibyte, cat = pre
    rng = random.Random(0xD1E7)
    texts = tiled([fill(short + multibyte, 700, rng), fill(short, 90, rng), fill(short + multibyte, 2 * CAP + 33, rng)])
    oids, ooff = orc.tokenize_batch_ids(texts)
    text, off = dev.pack_and_lower(texts)
    n = int(text.size)
    h = tok._table
    d_off = torch.from_numpy(off.astype(np.int64)).cuda()
    d_out = torch.zeros(n + 64, dtype=torch.int32, device="cuda")
    d_out_off = torch.zeros(len(texts) + 1, dtype=torch.int64, device="cuda")
    d_n = torch.zeros(1, dtype=torch.int64, device="cuda")
    h.set_option(dev.OPT_DEDUP, dev.DEDUP_NEVER)
    try:
        for narrow in (2, 1):
            h.set_option(OPT_LANE_NARROW, narrow)
            for shift in range(16):
                d_text = torch.zeros(n + 96, dtype=torch.uint8, device="cuda")
                assert d_text.data_ptr() % 16 == 0
                d_text[shift:shift + n] = torch.from_numpy(text).cuda()
                d_out.zero_()
                h.encode_dev(d_text.data_ptr() + shift, n, d_off.data_ptr(), len(texts), d_out.data_ptr(), d_out_off.data_ptr(), d_n.data_ptr())
                torch.cuda.synchronize()
                assert info(dev, h, 11) == (1 if narrow == 2 else 0), "the launch took the other kernel"
                assert int(d_n.item()) == oids.size, "shift %d" % shift
                assert np.array_equal(d_out_off.cpu().numpy().astype(np.uint64), ooff), "offsets differ at shift %d" % shift
                assert np.array_equal(d_out[:oids.size].cpu().numpy().view(np.uint32), oids), "ids differ at shift %d" % shift
    finally:
        h.set_option(OPT_LANE_NARROW, 0)
        h.set_option(dev.OPT_DEDUP, dev.DEDUP_AUTO)


def test_staged_end_at_every_residue(dev, pre):
    """texts of CAP + 40 .. CAP + 103 bytes: the last chunk's staged bytes end at every lane of a block, in a word and behind one"""
    tok, orc, short, multibyte, cat = pre
    rng = random.Random(0xD1E8)
    for r in range(64):
        body = fill(short + multibyte, CAP + 40 + r, rng)
        both(dev, tok, orc, tiled([body]))
        run(dev, tok, orc, tiled([body[:-1] + "x"]))  # the text ends with a letter, not a space


def test_words_at_the_edge_lanes(dev, pre):
    """words that begin or end in lanes 0, 62 and 63 of a block (the text opens the call, so byte k of it is lane k % 64 of block
    k // 64), and pairs that straddle a block boundary"""
    tok, orc, short, multibyte, cat = pre
    rng = random.Random(0xD1E9)
    two = [w for w in short if len(w) == 2][:40]
    words = [cat[3000:3002], cat[3100:3105], cat[3200:3212], "a", multibyte[0]]
    for edge in (64, 128, 576):
        sents = []
        for w in words:
            starts = {edge - 2, edge - 1, edge}                                      # begins in lane 62, 63, 0
            starts |= {edge - nbytes(w) - 2, edge - nbytes(w) - 1, edge - nbytes(w)}  # ends in lane 61 (a space in 62), 62, 63
            starts |= {edge + 1 - nbytes(w), edge - nbytes(w) // 2}                   # ends in lane 0; the boundary in its middle
            for start in sorted(s for s in starts if s >= 0):
                sents.append(fill(two, start, rng) + w + " " + fill(two, 40, rng))
        for s in sents:
            both(dev, tok, orc, tiled([s]))


def test_pairs_across_a_block_boundary(dev, pre):
    """the pair of lane 63 and the next block's first symbol: in one word it merges, behind a FOREIGN symbol it is not looked up,
    and where a sentence starts on the boundary there is no pair at all"""
    tok, orc, short, multibyte, cat = pre
    rng = random.Random(0xD1EA)
    two = [w for w in short if len(w) == 2][:40]
    for edge in (64, 192, 576):
        lead = fill(two, edge - 1, rng)
        assert nbytes(lead) == edge - 1
        both(dev, tok, orc, tiled([lead + "ie ", lead + "nie " + fill(two, 30, rng)]))
        for f in FOREIGN:
            k = nbytes(f)
            # the FOREIGN symbol's lead byte in lane 63, and its last byte in lane 63
            both(dev, tok, orc, tiled([fill(two, edge - 1, rng) + f + "ie ", fill(two, edge - k, rng) + f + "ie " + fill(two, 30, rng),
                                       fill(two, edge - k - 1, rng) + "n" + f + "ie " + f]))
        # a sentence that ends with a letter in lane 63, the next begins in lane 0: "i" | "e" must not merge
        first = fill(two, edge - 2, rng) + "ni"
        assert nbytes(first) == edge
        ids, off = both(dev, tok, orc, [""] * 63 + [first, "e ie", fill(two, 2 * CAP, rng)])
        assert int(ids[int(off[64])]) == ord("e")


def test_sentence_starts_on_block_edges(dev, pre):
    """sentences that start on the first and on the last byte of a block, after a space and after a letter"""
    tok, orc, short, multibyte, cat = pre
    rng = random.Random(0xD1EB)
    two = [w for w in short if len(w) == 2][:40]
    for at in (63, 64, 127, 128, 575, 576, 639):
        for last in (" ", "w"):
            head = fill(two, at - 1, rng) + last
            assert nbytes(head) == at
            both(dev, tok, orc, [""] * 63 + [head, "ie " + fill(short, 100, rng), fill(short + multibyte, CAP, rng)])
            both(dev, tok, orc, [""] * 62 + [head, "", "nie", fill(short, CAP + 7, rng)])


def test_whitespace_blocks_and_punctuation_runs(dev, pre):
    """a block that holds whitespace only (every word ends, no symbol), and runs of punctuation marks -- each a word of one
    symbol -- inside a block and across its boundary"""
    tok, orc, short, multibyte, cat = pre
    rng = random.Random(0xD1EC)
    two = [w for w in short if len(w) == 2][:40]
    for lead in (0, 1, 63, 64, 100):
        for gap in (64, 65, 127, 128, 200):
            both(dev, tok, orc, tiled([fill(two, lead, rng)[:-1] + " " * gap + "nie " + fill(two, 300, rng)]))
    both(dev, tok, orc, tiled([" " * 700 + "ie"]))
    both(dev, tok, orc, tiled([" " * 1100]))
    for lead in (0, 50, 60, 62, 63, 64):
        for run_ in ("!" * 8, "?!" * 5, "..." + "nie" + "...", "(nie)(ie)", "," * 70, "nie," * 20, "-" + "ie" + "-" * 3 + "nie"):
            both(dev, tok, orc, tiled([fill(two, lead, rng) + run_ + " " + fill(two, 100, rng), fill(two, lead, rng)[:-1] + run_]))


def test_sequence_past_the_staged_bytes(dev, pre):
    """a character of two, three and four bytes whose lead byte is among the last staged bytes of a chunk and whose other bytes are
    not: the chunk is cut before it and the next one stages it whole"""
    tok, orc, short, multibyte, cat = pre
    rng = random.Random(0xD1ED)
    for ch in ("é", "ж", "€", "😀"):
        for back in range(1, nbytes(ch)):
            for before, after in (("", ""), ("ni", "e"), ("", "ie")):
                # the lead byte is byte CAP - back of the text, which opens the call
                both(dev, tok, orc, tiled([fill(short, CAP - back - len(before), rng) + before + ch + after + " " + fill(short, 200, rng)]))


LETTERS = ([chr(c) for c in range(ord("a"), ord("z") + 1)] + [chr(c) for c in range(0x430, 0x450)] + [chr(c) for c in range(0x3B1, 0x3CA)]
           + [chr(c) for c in range(0x561, 0x568)])


def test_square_table(swt, oracle, dev):
    """every ordered pair of 90 letters is a merge: each pair of the text is found, each pair of a merged symbol misses.  The
    structured keys make the builder double the table twice (2^16 slots for 8,100 pairs)"""
    assert len(LETTERS) == 90 and all(c.isalpha() and c.lower() == c for c in LETTERS)
    tok, orc = make(swt, oracle, [(a, b) for a in LETTERS for b in LETTERS])
    h = tok._table
    assert info(dev, h, 8) == 1 and info(dev, h, 9) == 90 and info(dev, h, 12) == 1 and info(dev, h, 13) == 16
    rng = random.Random(0x5A5A)
    words = ["".join(rng.choice(LETTERS) for _ in range(rng.choice((1, 2, 3, 4, 5, 8, 9, 16, 31, 32, 33, 40)))) for _ in range(300)]
    words += [a + "é" + b for a in LETTERS[:5] for b in LETTERS[40:44]]  # FOREIGN in the middle: its neighbours have no pair
    run(dev, tok, orc, tiled(words[:120]))
    for n in (CAP - 1, CAP + 1, 3000):
        run(dev, tok, orc, tiled([fill(words, n, rng)]))
    ids, _ = run(dev, tok, orc, tiled(["abc " + LETTERS[89] + LETTERS[0]]))
    assert [int(x) for x in ids] == [tok._syms.intern("ab"), ord("c") | 0x80000000, tok._syms.intern(LETTERS[89] + LETTERS[0])]


def test_tables_with_other_kernels(swt, oracle, dev, pre):
    """the kernel of a table whose merged codes come from memory (Seq = false), an improper table (every word through literal_rounds),
    and a word longer than a chunk, which the one-lane walker merges over the wide table of the ids"""
    rng = random.Random(0xD1EE)
    tok, orc = make(swt, oracle, REPEATED)
    assert info(dev, tok._table, 8) == 1 and info(dev, tok._table, 12) == 0
    words = ["abc", "abcd", "abcabc", "aabc", "abcdabcd", "bcbc", "abcddd", "ddabcdd", "abd", "dddd", "abcd" * 8, "abc" * 11, "abécd"]
    run(dev, tok, orc, tiled(words))
    run(dev, tok, orc, tiled([fill(words, 2 * CAP + 1, rng)]))
    tok, orc = make(swt, oracle, IMPROPER)
    assert info(dev, tok._table, 8) == 1 and info(dev, tok._table, 2) == 0
    words = ["ab", "abc", "aaa", "aaaa", "cd", "xy", "abcabc", "aab", "xyxy", "żół", "żółżół", "abc" * 11, "a" * 33, "abéc"]
    run(dev, tok, orc, tiled(words))
    run(dev, tok, orc, tiled([fill(words, 2 * CAP + 1, rng)]))
    tok, orc, short, multibyte, cat = pre
    giant = cat[300:300 + CAP + 90]
    assert nbytes(giant) > CAP
    for lead in (0, 63, CAP - 1):
        run(dev, tok, orc, tiled([fill(short, lead, rng) + giant + " " + fill(short, 300, rng), fill(short, 90, rng)]))
