"""The seams of the host-call layer (csrc/swt_tile.hip: host_encode, host_encode_from_device) under the four host-buffer entry
points: swt_bpe_encode, swt_bpe_encode_naive, swt_wp_encode, swt_wp_encode_naive.  A call takes one of three paths by its size
alone:

  pinned     up to the encoder's single-launch limits (1,024 bytes for BPE, 2,048 for WordPiece, 64 sentences for both): the kernel
             reads and writes pinned host memory
  one-copy   up to kSmallCallBytes = 65,536 bytes and kSmallCallSents = 4,096 sentences: one block up, one block down
  large      beyond: plain copies through the handle's staging buffers

The batches below stand on both sides of every one of those limits.  Ids, offsets and statuses are exact against what the other
tests of each encoder use: the C oracle (FastBPE, FastWP), the rising-floor model of tests/test_naive_bpe_encode.py on a table
that is not order-equivalent (NaiveBPE), MaxMatch (NaiveWP).  The capacity test calls the C functions with room for one id less
than the call makes, once per path: SWT_ERR_CAPACITY, and the count, the offsets and the statuses are all there already.

The texts are made from a fixed seed out of letters the vocabularies know, plus a rare ".z": FastWP refuses a sentence with it
(status 1; the WordPiece vocabulary has no "z" and no "e", and a letter without an edge at the root never returns behind
punctuation), so the statuses are not all zero.  Nothing outside the repository is read.  Needs a real MI355X: `-m gpu`."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

from tests.test_gpu_naive_wp import model_batch
from tests.test_gpu_wp_seams import handmade_vocab
from tests.test_naive_bpe_encode import RisingFloor, splitter
from tests.test_naive_wp_encode import MaxMatch

pytestmark = pytest.mark.gpu

SMALL_BYTES, SMALL_SENTS = 65536, 4096   # kSmallCallBytes, kSmallCallSents (csrc/swt_common.h)
# (bytes, sentences) of a batch
CASES = [(SMALL_BYTES - 1, 300), (SMALL_BYTES, 300), (SMALL_BYTES + 1, 300),      # one-copy | large, by bytes
         (20000, SMALL_SENTS), (20000, SMALL_SENTS + 1),                           # one-copy | large, by sentences
         (1024, 3), (1025, 3), (2048, 3), (2049, 3), (500, 64), (500, 65)]         # pinned | one-copy, for BPE and for WordPiece
CAPACITY_CASES = {"pinned": (1024, 3), "one-copy": (SMALL_BYTES, 300), "large": (SMALL_BYTES + 1, 300)}

WORDS = ["ab", "abc", "abcd", "cd", "xy", "aaaa", "a", "b", "dab", "xyxy", "abab", "żół", "żółżół", "óż", "łłł", "ee", "eee",
         "abcdabcd", "ż", "aab", "aaab", "abcab"]
SEPARATORS = [" "] * 8 + [". ", ", ", " - ", "  "]

# proper (any trained table looks like this): FastBPE
PROPER = [("a", "b"), ("c", "d"), ("ab", "cd"), ("e", "e"), ("ee", "e"), ("abcd", "ab"), ("x", "y"), ("xy", "xy"), ("ab", "ab"),
          ("d", "a"), ("ż", "ó"), ("żó", "ł"), ("b", "c"), ("abcdab", "cd")]
# (ab, c) below the merge that makes ab, (aa, a) below (a, a), (a, b) listed twice: list order and lowest rank first differ
NOT_ORDER_EQUIVALENT = [("ab", "c"), ("a", "b"), ("aa", "a"), ("a", "a"), ("c", "d"), ("x", "y"), ("b", "c"), ("ż", "ó"),
                        ("a", "b"), ("żó", "ł")]


def sentence(rng, want):
    """a sentence of exactly `want` UTF-8 bytes"""
    parts, left = [], want
    while left:
        w = ".z" if rng.random() < 1 / 1500 else rng.choice(WORDS)
        if len(w.encode("utf-8")) > left:
            w = "a"
        parts.append(w)
        left -= len(w.encode("utf-8"))
        sep = rng.choice(SEPARATORS)
        if len(sep) < left:
            parts.append(sep)
            left -= len(sep)
    return "".join(parts)


@functools.lru_cache(maxsize=None)
def batch(n_bytes, n_sent):
    """(sentences, their UTF-8 bytes, their offsets): n_sent sentences of uneven length (some empty), n_bytes bytes together"""
    rng = random.Random(n_bytes * 8191 + n_sent)
    sents, left = [], n_bytes
    for i in range(n_sent):
        want = left
        if i < n_sent - 1:
            mean = left // (n_sent - i)
            want = min(left, rng.randint(mean // 2, mean + (mean + 1) // 2))
        sents.append(sentence(rng, want))
        left -= want
    raw = [s.encode("utf-8") for s in sents]
    off = np.zeros(n_sent + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in raw])
    assert int(off[-1]) == n_bytes and all(s == s.lower() for s in sents)
    return sents, np.frombuffer(b"".join(raw), dtype=np.uint8), off


@pytest.fixture(scope="module")
def dev(native):
    if native.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests need an MI355X (there is no CPU fallback to test)")
    native.init(0)
    return native


class Encoder:
    """one of the four: the C entry point, its handle, and what its other tests take for the truth"""

    def __init__(self, kind, swt, oracle):
        self.kind, self.status = kind, kind.endswith("wp")
        if kind == "fast_bpe":
            tok = swt.FastBPE()
            tok.merges_list = list(PROPER)
            tok._build_table()
            orc = oracle.OracleBPE(tok.merges_list)
            self.entry, self.handle = "swt_bpe_encode", tok._table
            self.expected = lambda sents: orc.tokenize_batch_ids(sents) + (None,)
        elif kind == "naive_bpe":
            tok = swt.NaiveBPE()
            tok.merges_list = list(NOT_ORDER_EQUIVALENT)
            self.entry, self.handle = "swt_bpe_encode_naive", tok._ensure_naive_table()
            assert not self.handle.order_equivalent()
            m, split = RisingFloor(tok.merges_list), splitter()
            self.expected = lambda sents: [m.tokenize(s, split) for s in sents]
        elif kind == "fast_wp":
            tok = swt.FastWP()
            tok.vocab = set(handmade_vocab())
            tok._build_trie()
            orc = oracle.OracleWP(tok._tokens)
            self.entry, self.handle = "swt_wp_encode", tok._trie

            def expected(sents):
                ids, off, st = orc.tokenize_batch_ids(sents)
                return ids, off, st[:len(sents)]

            self.expected = expected
        else:
            tok = swt.NaiveWP()
            tok.vocab = set(handmade_vocab())
            m = MaxMatch(tok.vocab)
            self.entry, self.handle = "swt_wp_encode_naive", tok._ensure_naive_trie()
            self.expected = lambda sents: model_batch(m, sents)
        self.tok = tok  # owns the handle

    def call(self, N, text, off, cap):
        """the C function itself with room for `cap` ids -> (return code, *n_tokens, ids, offsets, statuses or None)"""
        n_sent = off.size - 1
        ids = np.full(max(cap, 1), 0xDEADBEEF, dtype=np.uint32)
        out_off = np.full(n_sent + 1, 0xABABABABABABABAB, dtype=np.uint64)
        st = np.full(max(n_sent, 1), 0xEE, dtype=np.uint8)
        nt = C.c_uint64(0xABABABABABABABAB)
        args = [self.handle._h, N.ptr(text, N.u8p), N.ptr(off, N.u64p), n_sent, N.ptr(ids, N.u32p), cap, N.ptr(out_off, N.u64p)]
        args += [N.ptr(st, N.u8p), C.byref(nt)] if self.status else [C.byref(nt), 0]
        rc = getattr(N.lib(), self.entry)(*args)
        return rc, nt.value, ids, out_off, st[:n_sent] if self.status else None

    def same(self, got, sents, what):
        """ids, offsets and statuses of a full call against self.expected"""
        rc, nt, ids, off, st = got
        assert rc == 0, what
        ids = ids[:nt]
        want = self.expected(sents)
        if self.kind == "naive_bpe":  # the model spells tokens: the ids through the tokenizer's own symbol table, as its tests do
            toks = self.tok.decode_ids(ids)
            woff = np.zeros(len(sents) + 1, dtype=np.uint64)
            woff[1:] = np.cumsum([len(w) for w in want])
            assert np.array_equal(off, woff), what + ": offsets"
            assert toks == [t for w in want for t in w], what + ": ids"
            return
        wids, woff, wst = want
        if self.status:
            assert np.array_equal(st, wst), what + ": statuses"
        assert np.array_equal(off, woff), what + ": offsets"
        assert np.array_equal(ids, wids), what + ": ids"


KINDS = ["fast_bpe", "naive_bpe", "fast_wp", "naive_wp"]


@pytest.fixture(scope="module", params=KINDS)
def enc(request, swt, oracle, dev):
    return Encoder(request.param, swt, oracle)


def test_generator():
    """exact sizes; the refused word is there (FastWP's statuses are not all zero) and rare"""
    for n_bytes, n_sent in CASES:
        sents, text, off = batch(n_bytes, n_sent)
        assert len(sents) == n_sent and text.size == n_bytes == int(off[-1])
    sents, _, _ = batch(SMALL_BYTES, 300)
    assert 0 < sum(".z" in s for s in sents) < 150


@pytest.mark.parametrize("n_bytes,n_sent", CASES)
def test_host_path_seams(dev, enc, n_bytes, n_sent):
    sents, text, off = batch(n_bytes, n_sent)
    got = enc.call(dev, text, off, max(n_bytes, 1))
    enc.same(got, sents, "%s, %d bytes in %d sentences" % (enc.kind, n_bytes, n_sent))
    if enc.kind == "fast_wp" and n_bytes >= SMALL_BYTES - 1:
        assert got[4].any() and not got[4].all()  # refused sentences and accepted ones


@pytest.mark.parametrize("path", list(CAPACITY_CASES))
def test_capacity_one_id_short(dev, enc, path):
    """SWT_ERR_CAPACITY comes with the true count and with complete offsets and statuses, on every path"""
    n_bytes, n_sent = CAPACITY_CASES[path]
    _, text, off = batch(n_bytes, n_sent)
    rc, nt, _, full_off, full_st = enc.call(dev, text, off, n_bytes)
    assert rc == 0 and nt > 0 and int(full_off[-1]) == nt
    rc, short_nt, _, short_off, short_st = enc.call(dev, text, off, nt - 1)
    assert rc == dev.ERR_CAPACITY
    assert short_nt == nt
    assert np.array_equal(short_off, full_off)
    if enc.status:
        assert np.array_equal(short_st, full_st)
    assert enc.call(dev, text, off, nt)[0] == 0  # exactly enough is enough
