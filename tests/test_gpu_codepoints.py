"""Every code point, and every (class, UTF-8 length) pair at every seam, through each device copy of "decode a character, classify
it, spread the class over its continuation bytes" -- exact against the C oracle, the MaxMatch model and the lowercase fixture.

The inputs are tests/codepoint_cases.py (S1, S16, E, P; tests/test_codepoint_cases.py is their self-check on the CPU).  The text is
lowered by the fixture before it goes to an encoder or to the oracle (K.lower: the 26 host code points stay as they are), so no
comparison here depends on this interpreter's str.lower(), and none goes through pack_and_lower, which skips the device when the
interpreter's Unicode version differs and for small batches.  The device's own lowercase is compared with the fixture in the
first group of tests, through the C functions themselves.

  copy                                     reached by
  lower_kernel, lead_count / cp_to_byte /  test_lower_* (swt_utf8_prepare_joined, swt_utf8_prepare, swt_utf8_lower)
    sep_split kernels
  lane_split (running text, Mode 0)        test_fastbpe_s1 / _s16 / _p  [never]
  lane_split (one workgroup, Mode 2)       test_fastbpe_single_launch
  lane_split without a class table         test_fastbpe_encode_word
  wordref_kernel<kDedupBpe>, giant_word    test_fastbpe_* [always], the giant layout of P
  the same through NaiveBPE's entry        test_naivebpe
  wp_encode_kernel, wordref<kDedupWp>      test_fastwp_s1 [never / always], test_fastwp_single_launch, test_fastwp_p
  wp_naive_kernel                          test_naivewp_*
  census_kernel and its long-word walk     test_census_*

What a path cannot show from outside.  FastBPE, NaiveBPE, NaiveWP and the census read the bert_ws and bert_punct bits only; FastWP
reads py_space and py_alnum only.  Every one of those bits changes the output of "ab" + c + "ab" whether or not the vocabulary
knows c: FastWP gives two words for a space, one ['UNK'] for an unknown alphanumeric character and status 1 for any other unknown
character; a KNOWN character shows its alnum bit once more through the trie's link to the punctuation root (a ##c token ends its
run).  What stays invisible is a wrong class for a code point that no input holds between two letters -- which is why S1 holds all
of them -- and, in raw-word mode (encode_word), the class table as a whole: it is not read.

Mutants (values only, one line each, built outside the tree, each run once on the MI355X against this file's tests of its kernel
and against the tests the suite had for that kernel before; DESIGN.md 4.4c and profiles/codepoints.txt have the same table):

  mutant                                               this file                                    the old tests
  lane_split: cls_tab[cp & 0xFFFFu]                    16 of 19 fail (all but the three below)      lane_pipeline + lane_spans: 8 pass
  lane_split: cls2 shifted by cp & 15u, not twice it   the same 16 fail                             6 of 8 fail
  lane_split: two smear steps, not three               the same 16 fail                             8 pass
  census_kernel: cls_tab[cp & 0xFFFFu]                 test_census_*: 21 of 21 fail                 parity -k train: 19 pass
  wp_encode_kernel, phase B: cls_tab[cp & 0xFFFFu]     test_fastwp_*: 9 of 9 pass                   wp_seams: 207 pass
  lower_kernel, 4 bytes: (lo >> 12) & 0x0Fu            test_lower_*: 25 of 28 fail                  parity -k lower: 1 of 2 fails

The 16: test_fastbpe_s1[never], test_fastbpe_s16[never], test_fastbpe_p, test_fastbpe_single_launch, test_naivebpe_e,
test_naivebpe_p.  The three that pass under a lane_split mutant are test_fastbpe_s1[always], test_fastbpe_s16[always] (the dedup path
splits in wordref_kernel) and test_fastbpe_encode_word (no class table); the three that pass under the lower_kernel mutant are
test_lower_host_code_point_among_empty_sentences (no cased 4-byte letter).  The phase B mutant is output-equivalent: those classes
only propose segment starts, every walker classifies for itself, and a sentence whose walkers do not meet is redone sequentially.
So is `lo >> 12` without its mask, which was not built: every cased code point above U+FFFF lies below U+40000.

Needs a real MI355X: `-m gpu`."""
import ctypes as C

import numpy as np
import pytest

from tests import codepoint_cases as K
from tests.test_naive_wp_encode import MaxMatch

pytestmark = pytest.mark.gpu

PARTS = list(K.OFFSETS)  # P in six parts, one per offset of the lead byte against the seam: every layout and seam in each


@pytest.fixture(scope="module")
def dev(native):
    if native.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests need an MI355X (there is no CPU fallback to test)")
    native.init(0)
    return native


_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def s1_packed():
    return cached("s1_packed", lambda: K.pack(K.s1_lowered()))


def s16_lowered():
    return cached("s16_lowered", lambda: [K.lower(t) for t in K.s16()])


def e_sentences():
    """E as S1 spells a code point"""
    return cached("e_sentences", lambda: [K.lower("ab" + chr(cp) + "ab") for cp in K.edge_set()])


def p_part(d):
    return cached(("p", d), lambda: [p for p in K.position_family() if p.offset == d])


def first_difference(got_ids, got_off, want_ids, want_off, texts):
    n = min(got_off.size, want_off.size) - 1
    for i in range(n):
        a = got_ids[int(got_off[i]):int(got_off[i + 1])]
        b = want_ids[int(want_off[i]):int(want_off[i + 1])]
        if int(got_off[i]) != int(want_off[i]) or a.size != b.size or not np.array_equal(a, b):
            t = texts[i]
            return "sentence %d %r (%s): got %s, want %s" % (i, t[:24], " ".join("U+%04X" % ord(c) for c in t[:8]),
                                                            [hex(x) for x in a[:8].tolist()], [hex(x) for x in b[:8].tolist()])
    return "no sentence differs (lengths %d / %d)" % (got_off.size, want_off.size)


def same(got, want, texts, what):
    if len(want) == 3:
        bad = np.flatnonzero(got[2] != want[2])
        assert bad.size == 0, "%s: %d statuses differ, first at sentence %d %r: got %d, want %d" % (
            what, bad.size, bad[0], texts[int(bad[0])][:24], got[2][bad[0]], want[2][bad[0]])
    if not (np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0])):
        pytest.fail("%s: %s" % (what, first_difference(got[0], got[1], want[0], want[1], texts)))


# =============================================================================================== lowercase and offsets

def lower_expected(texts):
    """(bytes, offsets, need_host) from unicode_lower.json alone"""
    buf, off = K.pack([K.lower(t) for t in texts])
    need = np.fromiter((K.has_host(t) for t in texts), dtype=np.uint8, count=len(texts))
    return buf, off, need


def call_prepare_joined(N, texts):
    joined = K.join(texts)
    n = len(texts)
    out = np.full(max(int(joined.size) - (n - 1), 1), 0xEE, dtype=np.uint8)
    off = np.full(n + 1, 0xABABABABABABABAB, dtype=np.uint64)
    need = np.full(n, 0xEE, dtype=np.uint8)
    rc = N.lib().swt_utf8_prepare_joined(N.ptr(joined, N.u8p), int(joined.size), n, N.ptr(out, N.u8p), N.ptr(off, N.u64p), N.ptr(need, N.u8p))
    assert rc == 0, N.lib().swt_last_error()
    return out[:int(joined.size) - (n - 1)], off, need


def call_prepare(N, texts):
    buf = K.pack(texts)[0].copy()
    n = len(texts)
    cp_off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(np.fromiter(map(len, texts), dtype=np.uint64, count=n), out=cp_off[1:])
    off = np.full(n + 1, 0xABABABABABABABAB, dtype=np.uint64)
    need = np.full(n, 0xEE, dtype=np.uint8)
    rc = N.lib().swt_utf8_prepare(N.ptr(buf, N.u8p) if buf.size else None, int(buf.size), N.ptr(cp_off, N.u64p), n, N.ptr(off, N.u64p),
                                  N.ptr(need, N.u8p))
    assert rc == 0, N.lib().swt_last_error()
    return buf, off, need


def call_lower(N, texts):
    buf, off = K.pack(texts)
    buf = buf.copy()
    need = np.full(len(texts), 0xEE, dtype=np.uint8)
    rc = N.lib().swt_utf8_lower(N.ptr(buf, N.u8p) if buf.size else None, N.ptr(off, N.u64p), len(texts), N.ptr(need, N.u8p))
    assert rc == 0, N.lib().swt_last_error()
    return buf, off, need


LOWER_CALLS = {"prepare_joined": call_prepare_joined, "prepare": call_prepare, "lower": call_lower}


def same_lower(got, want, texts, what):
    buf, off, need = got
    wbuf, woff, wneed = want
    assert np.array_equal(off, woff), "%s: offsets differ, first at sentence %d" % (what, int(np.flatnonzero(off != woff)[0]))
    bad = np.flatnonzero(need != wneed)
    assert bad.size == 0, "%s: need_host differs for %d sentences, first %d %r" % (what, bad.size, bad[0], texts[int(bad[0])][:16])
    if not np.array_equal(buf, wbuf):
        at = int(np.flatnonzero(buf != wbuf)[0])
        s = int(np.searchsorted(woff, at, side="right")) - 1
        pytest.fail("%s: byte %d differs, in sentence %d %r: got %s, want %s" % (
            what, at, s, texts[s][:16], bytes(buf[int(woff[s]):int(woff[s + 1])][:24]).hex(), bytes(wbuf[int(woff[s]):int(woff[s + 1])][:24]).hex()))


def s1_lower_expected():
    def make():
        buf, off = s1_packed()
        need = np.zeros(len(K.s1()), dtype=np.uint8)
        need[[cp - 1 for cp in K.host_cps()]] = 1
        return buf, off, need
    return cached("s1_lower_expected", make)


@pytest.mark.parametrize("entry", list(LOWER_CALLS))
def test_lower_s1(dev, entry):
    """every code point: the bytes, the byte offsets, and need_host for exactly the 26 sentences of the host code points.  The
    batch is 8.8 MB: the scan over the 1-KiB blocks has two levels"""
    same_lower(LOWER_CALLS[entry](dev, K.s1()), s1_lower_expected(), K.s1(), "swt_utf8_" + entry)


@pytest.mark.parametrize("d", PARTS)
@pytest.mark.parametrize("entry", list(LOWER_CALLS))
def test_lower_p(dev, entry, d):
    """every representative around the 1-KiB block of the offset kernels (and every other seam, which these kernels do not have)"""
    for p in p_part(d):
        same_lower(LOWER_CALLS[entry](dev, p.texts), cached(("lower", p.name), lambda: lower_expected(p.texts)), p.texts, "%s, %s" % (entry, p.name))


@pytest.mark.parametrize("entry", list(LOWER_CALLS))
def test_lower_level2(dev, entry):
    """the characters on both sides of byte 1,048,576: block 1,024 is the first of the second scan level"""
    texts, _ = K.level2_batch()
    same_lower(LOWER_CALLS[entry](dev, texts), cached("lower_level2", lambda: lower_expected(texts)), texts, entry)


def test_lower_nul_batch(dev):
    """texts that hold U+0000 go by their code-point lengths"""
    texts = list(K.nul_batch())
    same_lower(call_prepare(dev, texts), lower_expected(texts), texts, "swt_utf8_prepare, U+0000")


@pytest.mark.parametrize("entry", list(LOWER_CALLS))
def test_lower_host_code_point_among_empty_sentences(dev, entry):
    """the binary search of lower_kernel: the flagged sentence behind and before runs of empty ones, and a host code point as the
    first and as the last character of the batch"""
    host = sorted(K.host_cps())
    h2, h3 = chr(next(c for c in host if c < 0x800)), chr(next(c for c in host if c >= 0x800))
    batches = [[h2], [h3 + "A"], ["A" + h3], [""] * 7 + [h2] + [""] * 9, [h3] + [""] * 70, [""] * 70 + [h3],
               [h2 + "abc"] + ["x"] * 100 + ["abc" + h3], [""] * 3 + ["ab" + h2 + "ab"] + [""] * 64 + ["É" + h3 + "É"] + [""] * 5 + ["Ab"],
               [""] * 1000 + [h3] + [""] * 1000 + ["A"] + [""] * 500 + [h2, "", h3, ""]]
    batches += [[("" if i % 3 else "Zz") for i in range(k)] + [c + "q"] + [""] * k for k in (1, 2, 63, 64, 65, 255) for c in (h2, h3)]
    for texts in batches:
        same_lower(LOWER_CALLS[entry](dev, texts), lower_expected(texts), texts, "%s, %d sentences" % (entry, len(texts)))


# ============================================================================================================ the tables

def bpe_merges():
    """proper, with 2-, 3- and 4-byte symbols on both sides of a pair: a wrong decode changes a lookup"""
    r = K.representatives()
    l2, l3, l4 = (chr(r[("letter", n)]) for n in (2, 3, 4))
    c2, c3, c4 = (K.lower(chr(r[("cased", n)])) for n in (2, 3, 4))
    return [("a", "b"), ("c", "d"), ("ab", l2), ("ab", l3), ("ab", l4), ("ab", c4), (l3, l4), (l3 + l4, l3 + l4), ("ab", "cd"), (c2, "ab"),
            (c3, "ab"), (l4, "ab"), ("ab" + l2, "ab"), (l3 + l4 + l3 + l4, l3 + l4 + l3 + l4), ("b", "a"), ("ab" + c4, "ab")]


@pytest.fixture(scope="module")
def fastbpe(swt, oracle, dev):
    tok = swt.FastBPE()
    tok.merges_list = bpe_merges()
    tok._build_table()
    return tok, oracle.OracleBPE(tok.merges_list)


@pytest.fixture(scope="module")
def naivebpe(swt, oracle, dev):
    tok = swt.NaiveBPE()
    tok.merges_list = bpe_merges()
    table = tok._ensure_naive_table()
    assert table.order_equivalent()
    return tok, table, oracle.OracleBPE(tok.merges_list)


def wp_vocab():
    tab = K.class_table()
    v = {"a", "b", "##a", "##b", ".", "[UNK]"}
    for cp in K.edge_set():
        if not tab[cp] & (K.WS | K.SPACE):
            v.update((chr(cp), "##" + chr(cp)))
    return v


@pytest.fixture(scope="module")
def fastwp(swt, oracle, dev):
    tok = swt.FastWP()
    tok.vocab = wp_vocab()
    tok._build_trie()
    return tok, oracle.OracleWP(tok._tokens)


def oracle_bpe_of(oracle, orc, key, lowered):
    return cached(("obpe", key), lambda: K.oracle_bpe(oracle, orc, lowered))


MODES = ["never", "always"]


def bpe_encode(dev, table, mode, lowered, flags=0, naive=False):
    text, off = K.pack(lowered) if not isinstance(lowered, tuple) else lowered
    table.set_option(dev.OPT_DEDUP, dev.DEDUP_NEVER if mode == "never" else dev.DEDUP_ALWAYS)
    try:
        return table.encode_naive(text, off, flags) if naive else table.encode(text, off, flags)
    finally:
        table.set_option(dev.OPT_DEDUP, dev.DEDUP_AUTO)


# ================================================================================================================ FastBPE

@pytest.mark.parametrize("mode", MODES)
def test_fastbpe_s1(dev, oracle, fastbpe, mode):
    tok, orc = fastbpe
    want = oracle_bpe_of(oracle, orc, "s1", K.s1_lowered())
    same(bpe_encode(dev, tok._table, mode, s1_packed()), want, K.s1_lowered(), "FastBPE %s, S1" % mode)


@pytest.mark.parametrize("mode", MODES)
def test_fastbpe_s16(dev, oracle, fastbpe, mode):
    tok, orc = fastbpe
    want = oracle_bpe_of(oracle, orc, "s16", s16_lowered())
    same(bpe_encode(dev, tok._table, mode, s16_lowered()), want, s16_lowered(), "FastBPE %s, S16" % mode)


@pytest.mark.parametrize("d", PARTS)
def test_fastbpe_p(dev, oracle, fastbpe, d):
    """the direct path and the dedup path on lowered text, and the separator form (the device lowers) on the text as it is"""
    tok, orc = fastbpe
    for p in p_part(d):
        lowered = [K.lower(t) for t in p.texts]
        want = K.oracle_bpe(oracle, orc, lowered)
        for mode in MODES:
            same(bpe_encode(dev, tok._table, mode, lowered), want, lowered, "FastBPE %s, %s" % (mode, p.name))
        got = tok._table.encode_joined(K.join(p.texts), len(p.texts))
        assert got is not None
        same(got, want, lowered, "FastBPE joined, %s" % p.name)


def single_launch_batches(max_bytes, max_sents=64):
    """E, and the head of every `sentences` batch of P (the seams at 16, 64, 384 and 512 bytes), in batches under the limits"""
    out, cur, size = [], [], 0
    for t in e_sentences():
        if len(cur) == max_sents or size + K.nbytes(t) > max_bytes:
            out.append(cur)
            cur, size = [], 0
        cur.append(t)
        size += K.nbytes(t)
    out.append(cur)
    for p in K.position_family():
        if p.layout == "sentences":
            cur, size = [], 0
            for t in p.texts:
                if len(cur) == max_sents or size + K.nbytes(t) > max_bytes:
                    break
                cur.append(K.lower(t))
                size += K.nbytes(t)
            out.append(cur)
    return out


def test_fastbpe_single_launch(dev, oracle, fastbpe):
    """one workgroup writing the caller's arrays: up to kDirectBytes = 1,024 bytes and kDirectSents = 64 sentences.  The library
    has no counter that names the path a call took; the limits are read from the source (K.constants(), asserted on the CPU by
    test_constants_are_the_kernels), so a change of them fails there instead of turning this into a second direct-path test"""
    tok, orc = fastbpe
    k = K.constants()
    assert k == K.EXPECTED_CONSTANTS
    batches = single_launch_batches(k["kDirectBytes"], k["kDirectSents"])
    assert all(sum(map(K.nbytes, b)) <= k["kDirectBytes"] and len(b) <= k["kDirectSents"] for b in batches)
    assert any(sum(map(K.nbytes, b)) > 900 for b in batches) and any(len(b) == 64 for b in batches)
    for i, b in enumerate(batches):
        same(bpe_encode(dev, tok._table, "never", b), K.oracle_bpe(oracle, orc, b), b, "FastBPE single launch, batch %d" % i)


def test_fastbpe_encode_word(dev, fastbpe):
    """raw-word mode reads no class table: "ab" + c + "ab" is ONE word whatever c is.  One word per call, as encode_word does it,
    for every code point of E; all of E as the sentences of one call (tiled) and of calls of 64 (one workgroup)"""
    tok, orc = fastbpe
    words = e_sentences()
    want = [orc.encode_word_ids(w) for w in words]
    woff = np.zeros(len(words) + 1, dtype=np.uint64)
    np.cumsum([w.size for w in want], out=woff[1:])
    wids = np.concatenate(want)
    same(bpe_encode(dev, tok._table, "never", words, flags=dev.BPE_RAW_WORDS), (wids, woff), words, "raw words, one call")
    for i in range(0, len(words), 64):
        got = bpe_encode(dev, tok._table, "never", words[i:i + 64], flags=dev.BPE_RAW_WORDS)
        assert np.array_equal(got[0], wids[int(woff[i]):int(woff[min(i + 64, len(words))])]), "raw words, 64 from %d" % i
    for i in range(len(words)):
        assert tok.encode_word(words[i]) == orc.encode_word(words[i]), "encode_word(%r)" % words[i]


# =============================================================================================================== NaiveBPE

def test_naivebpe_e(dev, oracle, naivebpe):
    tok, table, orc = naivebpe
    words = e_sentences()
    want = oracle_bpe_of(oracle, orc, "e", words)
    for mode in MODES:
        same(bpe_encode(dev, table, mode, words, naive=True), want, words, "NaiveBPE %s, E" % mode)


@pytest.mark.parametrize("d", PARTS)
def test_naivebpe_p(dev, oracle, naivebpe, d):
    tok, table, orc = naivebpe
    for p in p_part(d):
        lowered = [K.lower(t) for t in p.texts]
        want = K.oracle_bpe(oracle, orc, lowered)
        for mode in MODES:
            same(bpe_encode(dev, table, mode, lowered, naive=True), want, lowered, "NaiveBPE %s, %s" % (mode, p.name))


# ================================================================================================================= FastWP

def wp_encode(dev, trie, mode, lowered):
    text, off = K.pack(lowered) if not isinstance(lowered, tuple) else lowered
    trie.set_option(dev.OPT_DEDUP, dev.DEDUP_NEVER if mode == "never" else dev.DEDUP_ALWAYS)
    try:
        return trie.encode(text, off)
    finally:
        trie.set_option(dev.OPT_DEDUP, dev.DEDUP_AUTO)


@pytest.mark.parametrize("mode", MODES)
def test_fastwp_s1(dev, oracle, fastwp, mode):
    tok, orc = fastwp
    want = cached("owp_s1", lambda: K.oracle_wp(oracle, orc, K.s1_lowered()))
    assert 0 < int(want[2].sum()) < want[2].size  # refused sentences and accepted ones
    same(wp_encode(dev, tok._trie, mode, s1_packed()), want, K.s1_lowered(), "FastWP %s, S1" % mode)


def test_fastwp_single_launch(dev, oracle, fastwp):
    """up to kWpDirectBytes = 2,048 bytes and kWpDirectSents = 64 sentences (read from the source, as above): E, and the heads of
    P's batches"""
    tok, orc = fastwp
    k = K.constants()
    assert k == K.EXPECTED_CONSTANTS
    batches = single_launch_batches(k["kWpDirectBytes"], k["kWpDirectSents"])
    assert all(sum(map(K.nbytes, b)) <= k["kWpDirectBytes"] and len(b) <= k["kWpDirectSents"] for b in batches)
    assert any(sum(map(K.nbytes, b)) > k["kDirectBytes"] for b in batches)  # beyond FastBPE's limit, within this one
    for i, b in enumerate(batches):
        same(wp_encode(dev, tok._trie, "never", b), K.oracle_wp(oracle, orc, b), b, "FastWP single launch, batch %d" % i)


@pytest.mark.parametrize("d", PARTS)
def test_fastwp_p(dev, oracle, fastwp, d):
    tok, orc = fastwp
    for p in p_part(d):
        lowered = [K.lower(t) for t in p.texts]
        want = K.oracle_wp(oracle, orc, lowered)
        for mode in MODES:
            same(wp_encode(dev, tok._trie, mode, lowered), want, lowered, "FastWP %s, %s" % (mode, p.name))


# ================================================================================================================ NaiveWP

class WindowedMaxMatch(MaxMatch):
    """MaxMatch for words of thousands of characters: the longest-prefix search starts at the longest token instead of at the
    whole word.  Same answer (no longer prefix can be a token); test_windowed_model_is_maxmatch compares the two."""

    def __init__(self, vocab):
        super().__init__(vocab)
        self.longest = max(map(len, self.vocab))
        self.plain = "#" in self.vocab or "##" in self.vocab  # a piece could be cut out of the '##' put back: leave it to MaxMatch

    def encode_word(self, word):
        if self.plain:
            return super().encode_word(word)
        pieces, p, n, head = [], 0, len(word), ""
        while p < n:
            i = min(n - p, self.longest - len(head))
            while i > 0 and head + word[p:p + i] not in self.vocab:
                i -= 1
            if i == 0:
                return ["[UNK]"]
            pieces.append(head + word[p:p + i])
            p += i
            head = "##"
        return pieces


def naive_wp_model(m, lowered):
    """(ids, offsets, status) as the device must give them, the split by the fixture's classes"""
    ids, off, st = [], [0], []
    memo = {}
    for t in lowered:
        toks = []
        for w in K.split_words(t):
            p = memo.get(w)
            if p is None:
                p = memo[w] = m.encode_word(w) or ()
            if not p:
                toks = None
                break
            toks += p
        st.append(0 if toks is not None else 1)
        if toks is not None:
            ids += m.ids_of(toks)
        off.append(len(ids))
    return np.array(ids, dtype=np.uint32), np.array(off, dtype=np.uint64), np.array(st, dtype=np.uint8)


@pytest.fixture(scope="module")
def naivewp(swt, dev):
    tok = swt.NaiveWP()
    tok.vocab = wp_vocab()
    return tok, tok._ensure_naive_trie(), WindowedMaxMatch(tok.vocab)


def test_windowed_model_is_maxmatch(naivewp):
    _, _, m = naivewp
    plain = MaxMatch(m.vocab)
    for w in e_sentences() + ["##", "#a", "a##b", "ab" * 40, "abq", "qab", "a.b"]:
        for word in K.split_words(w):
            assert m.encode_word(word) == plain.encode_word(word), word


def test_naivewp_e(dev, naivewp):
    tok, trie, m = naivewp
    words = e_sentences()
    text, off = K.pack(words)
    same(trie.encode_naive(text, off), naive_wp_model(m, words), words, "NaiveWP, E")
    for i, b in enumerate(single_launch_batches(2048)[:100]):
        text, off = K.pack(b)
        same(trie.encode_naive(text, off), naive_wp_model(m, b), b, "NaiveWP single launch, batch %d" % i)


@pytest.mark.parametrize("k", range(4))
def test_naivewp_s1_quarter(dev, naivewp, k):
    """code points k * 4, k * 4 + 16, ... of S1 (four tests: every 4th code point in all)"""
    tok, trie, m = naivewp
    lowered = K.s1_lowered()[4 * k::16]
    text, off = K.pack(lowered)
    same(trie.encode_naive(text, off), naive_wp_model(m, lowered), lowered, "NaiveWP, S1[%d::16]" % (4 * k))


@pytest.mark.parametrize("d", PARTS)
def test_naivewp_p(dev, naivewp, d):
    tok, trie, m = naivewp
    for p in p_part(d):
        lowered = [K.lower(t) for t in p.texts]
        text, off = K.pack(lowered)
        same(trie.encode_naive(text, off), naive_wp_model(m, lowered), lowered, "NaiveWP, %s" % p.name)


# ================================================================================================================= census

def census_from_text(N, lowered, wordpiece=False):
    text, off = K.pack(lowered)
    return (N.BpeTrainer.from_text_wordpiece if wordpiece else N.BpeTrainer.from_text)(text, off)


def census_joined(N, texts):
    """swt_bpe_train_create_joined itself (BpeTrainer.from_texts declines when the interpreter's Unicode version differs)"""
    joined = K.join(texts)
    need = np.full(len(texts), 0xEE, dtype=np.uint8)
    h = C.c_void_p()
    N.check(N.lib().swt_bpe_train_create_joined(N.ptr(joined, N.u8p), int(joined.size), len(texts), N.ptr(need, N.u8p), C.byref(h)))
    assert not need.any() and h.value
    return N.BpeTrainer(h)


def same_census(tr, orc, what):
    gs, go, gf = tr.export()
    ws, wo, wf = orc.export()
    assert np.array_equal(go, wo), "%s: word offsets differ (%d / %d words)" % (what, go.size - 1, wo.size - 1)
    assert np.array_equal(gf, wf), "%s: frequencies differ" % what
    if not np.array_equal(gs, ws):
        at = int(np.flatnonzero(gs != ws)[0])
        pytest.fail("%s: symbol %d differs: got %#x, want %#x" % (what, at, gs[at], ws[at]))
    tr.close()


def same_census_wp(N, tr, orc_wp, orc_bpe, what):
    """the oracle names a '##c' symbol by first appearance, the device WP_CONT + c: same words and frequencies, the oracle's
    names in bijection with the code points at their places (OracleBPETrainer's stream of the same text), and the device's ids
    are those code points, + WP_CONT behind a word's first symbol"""
    gs, go, gf = tr.export()
    ws, wo, wf = orc_wp.export()
    cs, co, cf = orc_bpe.export()
    assert np.array_equal(wo, co) and np.array_equal(wf, cf)
    assert np.array_equal(go, wo) and np.array_equal(gf, wf), "%s: words or frequencies differ" % what
    first = np.zeros(cs.size, dtype=bool)
    first[wo[:-1].astype(np.int64)] = True
    assert np.array_equal(ws[first], cs[first]) and np.all(ws[~first] >= N.SYM_BASE)
    key = np.unique((ws[~first].astype(np.int64) << 21) | cs[~first].astype(np.int64))
    pairs = np.stack([key >> 21, key & 0x1FFFFF])
    assert np.unique(pairs[0]).size == pairs.shape[1] == np.unique(pairs[1]).size  # a bijection
    for k in range(0, pairs.shape[1], max(pairs.shape[1] // 50, 1)):
        assert orc_wp.symbol(int(pairs[0, k])) == "##" + chr(int(pairs[1, k]))
    want = np.where(first, cs, cs + np.uint32(N.WP_CONT)).astype(np.uint32)
    if not np.array_equal(gs, want):
        at = int(np.flatnonzero(gs != want)[0])
        pytest.fail("%s: symbol %d differs: got %#x, want %#x" % (what, at, gs[at], want[at]))
    tr.close()


CENSUS = ["from_text", "from_texts", "from_text_wordpiece"]


@pytest.mark.parametrize("form", CENSUS)
def test_census_s16(dev, oracle, form):
    """the joined form lowers on the device and hands a batch with a host code point back, so it gets S16 without the sentences
    that hold one (26 at the most); the other two get all of it, lowered by the fixture"""
    if form == "from_texts":
        texts = cached("s16_nohost", lambda: [t for t in K.s16() if not K.has_host(t)])
        assert len(K.s16()) - 26 <= len(texts) < len(K.s16())
        lowered = cached("s16_nohost_lowered", lambda: [K.lower(t) for t in texts])
        same_census(census_joined(dev, texts), K.oracle_census(oracle, lowered), "joined, S16")
        return
    lowered = s16_lowered()
    orc = K.oracle_census(oracle, lowered)
    if form == "from_text":
        same_census(census_from_text(dev, lowered), orc, "from_text, S16")
    else:
        same_census_wp(dev, census_from_text(dev, lowered, True), K.oracle_census(oracle, lowered, True), orc, "from_text_wordpiece, S16")


@pytest.mark.parametrize("d", PARTS)
@pytest.mark.parametrize("form", CENSUS)
def test_census_p(dev, oracle, form, d):
    for p in p_part(d):
        lowered = [K.lower(t) for t in p.texts]
        orc = K.oracle_census(oracle, lowered)
        if form == "from_text":
            same_census(census_from_text(dev, lowered), orc, "from_text, %s" % p.name)
        elif form == "from_texts":
            same_census(census_joined(dev, p.texts), orc, "joined, %s" % p.name)
        else:
            same_census_wp(dev, census_from_text(dev, lowered, True), K.oracle_census(oracle, lowered, True), orc, "wordpiece, %s" % p.name)
