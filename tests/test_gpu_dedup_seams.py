"""The seams of the FastBPE word-dedup path (csrc/swt_dedup.hip: wordref_kernel<kDedupBpe>, ureg_kernel, refcount_kernel,
refwrite_kernel, and lane_kernel<1> over the unique words with the plan ureg_kernel writes) against the C oracle: ids and offsets
exact, under the handmade table of tests/dedup_seam_cases.py and the pretrained merges.  The constructions, the model that says
which seam each one reaches and the paragraph on what the geometry allows are in tests/dedup_seam_cases.py; that every one
reaches its seam is checked without a GPU by tests/test_dedup_seam_cases.py.  Every batch of every family runs here: none is left out.

That the path under test ran is asserted, not supposed: profile level 3 brackets exactly the wordref_kernel launch of dedup_front,
so a forced-dedup call leaves one bracket and a DEDUP_NEVER call none (counted()).  The DEDUP_NEVER leg is there for the message
of a failure only: it tells whether the direct path disagrees with the oracle as well.

test_unaligned_device_text hands swt_bpe_encode_dev and swt_wp_encode_dev a text pointer at 0, 1, 7, 8 and 15 bytes behind an
aligned address, 64 bytes of 'q' directly behind byte n_bytes inside the same allocation, and sixteen consecutive lengths whose
last word ends the text: the byte-wise branch of the staging guard (g + 16 <= n_bytes && aligned) of wordref_kernel, the lane
kernel and wp_encode_kernel then runs with a tail, and a reader that went past n_bytes would lengthen the last word.

What the geometry allows (worked out from the kernels, so nobody looks for more; the walk itself is described in
tests/dedup_seam_cases.py).  A tabled word has two bytes at least, so a span of n bytes lists at most n / 2 words and
span_base >> 1 never reaches the next tile's list: 512 distinct two-byte words in 1,024 bytes (sentence starts are their only
boundaries) fill a list to its last entry, from an even and from an odd span_base.  Every sentence of a tile starts at most 1,024
bytes behind the tile's first one, so it has at most 1,024 of the tile's words before it: whatever a giant sentence's tile holds
(tile_words above 1,536: refwrite_kernel's later chunks), the sentence offsets of a tile are all written in the first chunk trip
of refwrite_kernel, and a sentence behind a giant one, empty or not, opens a later tile: no sentence reaches the `run` branch of a
later trip.  A cut lies at most 1,532 bytes behind abase, so a word of 1,533 - off0 bytes or more at cb takes the one-lane path.
A one-symbol word at cb is always followed by a boundary the cut can take, so the one-lane path's `nchar == 1` branch is reached
by a punctuation character alone.  A span end that is a sentence start at abase + 1,536 or before makes the chunk the last one
(no cut: everything staged is used); one byte later the chunk is cut.  The byte compare decides only between words of one length,
one tag and one probe sequence: the compare family takes pairs that differ at one byte and share tag and home slot of a
sixteen-slot table (SWT_OPT_DEDUP_TABLE_BITS 4); for the top byte of the last eight bytes the hash takes in (words of 16, 24 and
40 bytes, last byte) no such pair exists, so there the compare never decides.  A multi-byte character that the staged end clips
is decoded from the bytes that are there: U+2800 (E2 A0 80) behind two bytes reads as U+00A0, white space; the four bytes of room
of the cut rule keep such a false boundary from becoming a cut ("a word around U+2800" in the chunk end sweep).

Measured on an MI355X, this layout, `--durations=0`, the three seam and parity files in one run: the slowest case of
tests/test_gpu_wp_seams.py took 0.44 s (test_fast_wp_seams[c-align 0-19-0]); here the slowest was
test_dedup_seams[handmade-chunk end 1, off0 0-0] with 0.21 s (the first test of the file: it loads the library), then the parts of
the giant family with 0.09 .. 0.16 s (its words go through one lane in global memory), lengths 0.10 .. 0.12 s, the chunk end
sweeps 0.04 .. 0.09 s each (0.03 s of it generating the 143 batches), test_unaligned_device_text 0.04 .. 0.08 s, everything else
0.05 s or less (scan: a text of 1 MiB per case; counter: 608,000 bytes); the module's fixture (both tables) 1.85 s once.  Unsplit,
the giant family took 0.43 s and the chunk end sweep 0.46 s, above that bound.  The C oracle takes 0.4 s for all batches per table.

What the sweep defends, measured once per library on an MI355X with one one-line change to swt_dedup.hip each (value changes
only: a constant of a comparison, a dropped term of a sum; every one read beforehand to keep all indexes inside their buffers),
this file up to its first failure and the BPE dedup tests from before it (test_gpu_parity.py -k dedup):
  kDdMaxProbes = 1                       healed by design (a word that finds no slot at once gets its own and is encoded like a
                                         new one): passes everything, as read
  the tail compare of the coherent       fails here at "compare: words of 17 bytes that differ at byte 16, table bits 4" (ids: the
  path from byte 17                      second word gets the first one's tokens); the old tests pass
  the cut rule's `staged - 3u` as        fails here at "chunk end 1: a word around U+2800 at end -4, off0 0" (ids: the word is cut
  `staged`                               in two at the false white space); the old tests pass
  `L.nwb[rel >> 6]` dropped from         fails here at the first batch of the file (offsets: every batch has a sentence start behind
  sent_word                              the first 64-byte block with words before it) and in four old tests
  refwrite_kernel's rest loop            fails here at the first batch of the file (ids: its filler holds "bdbdbd", six tokens
  from 4                                 under the handmade table) and in three old tests
Not run, because nothing in the code shows that they stay inside their buffers: ureg_kernel's plan2 loop writing only its first
boundary (the entries it leaves out keep whatever the buffer held, and lane_kernel<1> takes them as indexes of unique words), and
`wlen <= l0` as `wlen < l0` (one-byte words in the table: more list entries than span / 2, more unique words than n_bytes / 2).

Needs a real MI355X: `-m gpu`."""
import json
import os

import numpy as np
import pytest

from tests import dedup_seam_cases as D

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev(native):
    if native.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests need an MI355X (there is no CPU fallback to test)")
    native.init(0)
    return native


@pytest.fixture(scope="module")
def tables(swt, oracle, dev, ref_dir):
    """name -> (FastBPE, its oracle)"""
    with open(os.path.join(ref_dir, "resources/pretrained/FastBPE", "merges.json"), encoding="utf-8") as f:
        pretrained = [tuple(m) for m in json.load(f)]
    out = {}
    for name, merges in (("handmade", D.HANDMADE), ("pretrained", pretrained)):
        tok = swt.FastBPE()
        tok.merges_list = list(merges)
        tok._build_table()
        out[name] = (tok, oracle.OracleBPE(tok.merges_list))
    return out


def counted(dev, handle, mode, call):
    """call() under SWT_OPT_DEDUP = mode -> its result; asserts the dedup pipelines that ran: one under DEDUP_ALWAYS, none
    under DEDUP_NEVER"""
    handle.set_option(dev.OPT_DEDUP, mode)
    dev.profile_enable(3)
    try:
        dev.profile_read()
        got = call()
        _, n = dev.profile_read()
    finally:
        dev.profile_enable(0)
        handle.set_option(dev.OPT_DEDUP, dev.DEDUP_AUTO)
    assert n == (1 if mode == dev.DEDUP_ALWAYS else 0), "%d dedup pipelines ran under SWT_OPT_DEDUP %d" % (n, mode)
    return got


def differs(got, want):
    if not np.array_equal(got[1], want[1]):
        return "offsets"
    return None if np.array_equal(got[0], want[0]) else "ids"


def check(dev, tok, orc, table, b):
    want = orc.tokenize_batch_ids(b.sents)
    h = tok._table
    h.set_option(dev.OPT_DEDUP_TABLE_BITS, b.bits)
    h.set_option(dev.OPT_UNIQUE_TILE, b.utile)
    try:
        dedup = counted(dev, h, dev.DEDUP_ALWAYS, lambda: tok.encode_ids_batch(b.sents))
        direct = counted(dev, h, dev.DEDUP_NEVER, lambda: tok.encode_ids_batch(b.sents))
    finally:
        h.set_option(dev.OPT_DEDUP_TABLE_BITS, 0)
        h.set_option(dev.OPT_UNIQUE_TILE, 0)
    bad = differs(dedup, want)
    assert bad is None, "%s differ on the dedup path (the direct path: %s): %s table, %s: %d sentences, %d bytes" % (
        bad, differs(direct, want) or "as the oracle", table, b.name, len(b.sents), sum(map(D.nbytes, b.sents)))


@pytest.mark.parametrize("table,family,part", [(t, f, k) for t in ("handmade", "pretrained") for f, k in D.CASES])
def test_dedup_seams(dev, tables, table, family, part):
    tok, orc = tables[table]
    batches = D.part(family, part)
    assert batches
    for b in batches:
        check(dev, tok, orc, table, b)


def test_small_calls_reach_the_dedup(dev, tables):
    """a call of at most 1,024 bytes and 64 sentences goes over the pinned host block, and under DEDUP_ALWAYS still through the
    dedup (check() asserts the bracket); these are such calls"""
    small = [b for f in ("small", "one symbol") for b in D.batches(f)
             if sum(map(D.nbytes, b.sents)) <= D.DIRECT_BYTES and len(b.sents) <= D.DIRECT_SENTS]
    assert len(small) >= 3
    for b in small:
        check(dev, *tables["handmade"], "handmade", b)


# ------------------------------------------------------------------------------------------------- unaligned, unpadded device text

OFFSETS = (0, 1, 7, 8, 15)
TAIL = 64


def texts_ending_in_a_word(corpus, first_len, lengths=16):
    """[(sentences, their bytes, offsets)] of first_len, first_len + 1, .. bytes; the last word ends the text"""
    out = []
    for n in range(first_len, first_len + lengths):
        sents, left = [], n
        for s in corpus:
            s = s.lower()
            if D.nbytes(s) + 8 > left:
                break
            sents.append(s)
            left -= D.nbytes(s)
        sents.append("koniec " + "a" * (left - 7))
        raw = [s.encode("utf-8") for s in sents]
        off = np.concatenate([[0], np.cumsum([len(r) for r in raw])]).astype(np.uint64)
        assert int(off[-1]) == n
        out.append((sents, np.frombuffer(b"".join(raw), dtype=np.uint8), off))
    return out


def encode_at(torch, handle, text, off, shift, wp):
    """the text `shift` bytes behind an aligned address, 'q' before and directly behind it; -> (ids, offsets[, statuses])"""
    n, n_sent = int(text.size), off.size - 1
    buf = torch.full((shift + n + TAIL,), ord("q"), dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf[shift:shift + n] = torch.from_numpy(text.copy()).cuda()
    d_off = torch.from_numpy(off.view(np.int64).copy()).cuda()
    d_out = torch.empty(n + 64, dtype=torch.int32, device="cuda")
    d_out_off = torch.empty(n_sent + 1, dtype=torch.int64, device="cuda")
    d_status = torch.zeros(n_sent + 8, dtype=torch.uint8, device="cuda")
    d_n = torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    if wp:
        handle.encode_dev(buf.data_ptr() + shift, n, d_off.data_ptr(), n_sent, d_out.data_ptr(), d_out_off.data_ptr(),
                          d_status.data_ptr(), d_n.data_ptr(), 0)
    else:
        handle.encode_dev(buf.data_ptr() + shift, n, d_off.data_ptr(), n_sent, d_out.data_ptr(), d_out_off.data_ptr(), d_n.data_ptr(), 0, 0)
    torch.cuda.synchronize()
    k = int(d_n.item())
    assert bytes(buf[shift + n:].cpu().numpy()) == b"q" * TAIL and bytes(buf[:shift].cpu().numpy()) == b"q" * shift
    got = (d_out[:k].cpu().numpy().view(np.uint32), d_out_off.cpu().numpy().view(np.uint64))
    return got + ((d_status[:n_sent].cpu().numpy(),) if wp else ())


@pytest.mark.parametrize("encoder,first_len", [("bpe", 1500), ("bpe", 600), ("wp", 2600), ("wp", 600)])
def test_unaligned_device_text(swt, oracle, dev, tables, corpora, ref_dir, encoder, first_len):
    torch = pytest.importorskip("torch")
    wp = encoder == "wp"
    if wp:
        tok = swt.FastWP()
        tok.load_resources(os.path.join(ref_dir, "resources/pretrained/FastWordPiece"))
        orc, handle = oracle.OracleWP(tok._tokens), tok._trie
    else:
        tok, orc = tables["pretrained"]
        handle = tok._table
    for sents, text, off in texts_ending_in_a_word(corpora["pan"], first_len):
        want = orc.tokenize_batch_ids(sents)
        for shift in OFFSETS:
            for mode in (dev.DEDUP_ALWAYS, dev.DEDUP_NEVER):
                got = counted(dev, handle, mode, lambda: encode_at(torch, handle, text, off, shift, wp))
                tag = "%s, %d bytes at an address = %d mod 16, SWT_OPT_DEDUP %d" % (encoder, text.size, shift, mode)
                if wp:
                    assert np.array_equal(got[2], want[2][:len(sents)]), "statuses differ: " + tag
                assert np.array_equal(got[1], want[1]), "offsets differ: " + tag
                assert np.array_equal(got[0], want[0]), "ids differ: " + tag
