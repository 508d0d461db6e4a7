"""FastWP token spans on the device (swt_wp_encode_spans, swt_wp_encode_spans_dev; csrc/swt_wp.hip, the span instantiation of
wp_encode_kernel) against the reference's own answers (tests/golden/fastwp_spans.json) and, at the kernel's seams, against the
Python model that reproduces them (tests/wp_span_cases.py).  Every input also goes through swt_wp_encode: ids, offsets and
statuses of the two calls are equal bit for bit.  The outputs are fenced by sentinel words behind the documented capacity (two span
words and one word index for every id the call has room for: n_bytes); the `_dev` form runs on a side stream over outputs filled
with garbage.  Needs a real MI355X: `-m gpu`."""
import functools

import numpy as np
import pytest

from tests.test_gpu_lane_spans import fill, nbytes
from tests.test_gpu_wp_seams import handmade_vocab, handmade_words
from tests.wp_span_cases import UNK, WpSpanModel, seam_batches

pytestmark = pytest.mark.gpu
PAD = 16
SENTINEL = 0xDEADBEEF
STRADDLE_PARTS = 4


@pytest.fixture(scope="module")
def dev(native):
    if native.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests need an MI355X (there is no CPU fallback to test)")
    native.init(0)
    return native


@pytest.fixture(scope="module")
def caps(dev):
    return dev.WpTrie.encode_spans_capacity()


def pack(sents):
    """lowercased str or bytes sentences -> (text uint8, offsets uint64)"""
    raw = [s if isinstance(s, bytes) else s.encode("utf-8") for s in sents]
    off = np.zeros(len(raw) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in raw], dtype=np.uint64)
    return np.frombuffer(b"".join(raw) + b"\0", dtype=np.uint8)[:-1].copy(), off


def fenced(n, dtype, fill_value):
    a = np.full(n + 2 * PAD, fill_value, dtype=dtype)
    a[:PAD] = a[n + PAD:] = np.array(SENTINEL).astype(dtype)
    return a


def fences_hold(*arrays):
    for a in arrays:
        s = np.array(SENTINEL).astype(a.dtype)
        assert (a[:PAD] == s).all() and (a[a.size - PAD:] == s).all(), "a sentinel word was overwritten"


def run_host(dev, trie, text, off, codepoints, with_word=True):
    """swt_wp_encode_spans, sentinels around every output -> (ids, offsets, status, spans[n, 2], word or None)"""
    n_sent, cap = int(off.size) - 1, max(int(text.size), 1)
    ids, spans, word = fenced(cap, np.uint32, 0x5A5A5A5A), fenced(2 * cap, np.uint32, 0x5A5A5A5A), fenced(cap, np.uint32, 0x5A5A5A5A)
    out_off, status = fenced(n_sent + 1, np.uint64, 0x5A), fenced(max(n_sent, 1), np.uint8, 0x5A)
    nt = np.zeros(1, dtype=np.uint64)
    p = dev.ptr
    dev.check(dev.lib().swt_wp_encode_spans(trie._h, p(text, dev.u8p) if text.size else None, p(off, dev.u64p), n_sent, p(ids[PAD:], dev.u32p), cap,
                                            p(out_off[PAD:], dev.u64p), p(status[PAD:], dev.u8p), p(nt, dev.u64p),
                                            dev.SPAN_CODEPOINTS if codepoints else 0, p(spans[PAD:], dev.u32p),
                                            p(word[PAD:], dev.u32p) if with_word else None))
    fences_hold(ids, spans, word, out_off, status)
    n = int(nt[0])
    if not with_word:
        assert (word[PAD:PAD + cap] == 0x5A5A5A5A).all()
    return (ids[PAD:PAD + n].copy(), out_off[PAD:PAD + n_sent + 1].copy(), status[PAD:PAD + n_sent].copy(),
            spans[PAD:PAD + 2 * n].reshape(-1, 2).copy(), word[PAD:PAD + n].copy() if with_word else None)


def run_dev(dev, trie, text, off, codepoints, with_word=True):
    """swt_wp_encode_spans_dev on torch tensors and a side stream, the outputs pre-filled with garbage and fenced"""
    import torch

    n_sent, cap = int(off.size) - 1, max(int(text.size), 1)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt).copy()).cuda()  # noqa: E731
    d_text = up(np.concatenate([text, np.zeros(16, np.uint8)]), np.uint8)
    d_off = up(off, np.int64)
    outs = [up(fenced(cap, np.uint32, 0xA5A5A5A5), np.int32), up(fenced(2 * cap, np.uint32, 0xA5A5A5A5), np.int32),
            up(fenced(cap, np.uint32, 0xA5A5A5A5), np.int32), up(fenced(n_sent + 1, np.uint64, 0xA5), np.int64),
            up(fenced(max(n_sent, 1), np.uint8, 0xA5), np.uint8), up(fenced(1, np.uint64, 0xA5), np.int64)]
    d_ids, d_spans, d_word, d_out_off, d_status, d_nt = outs
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        trie.encode_spans_dev(d_text.data_ptr(), int(text.size), d_off.data_ptr(), n_sent, d_ids.data_ptr() + 4 * PAD,
                              d_out_off.data_ptr() + 8 * PAD, d_status.data_ptr() + PAD, d_nt.data_ptr() + 8 * PAD,
                              d_spans.data_ptr() + 4 * PAD, (d_word.data_ptr() + 4 * PAD) if with_word else None,
                              codepoints=codepoints, stream=stream.cuda_stream)
    stream.synchronize()
    ids, spans, word = (t.cpu().numpy().view(np.uint32) for t in (d_ids, d_spans, d_word))
    out_off, nt = (t.cpu().numpy().view(np.uint64) for t in (d_out_off, d_nt))
    status = d_status.cpu().numpy()
    fences_hold(ids, spans, word, out_off, status, nt)
    n = int(nt[PAD])
    if not with_word:
        assert (word[PAD:PAD + cap] == 0xA5A5A5A5).all()
    return (ids[PAD:PAD + n].copy(), out_off[PAD:PAD + n_sent + 1].copy(), status[PAD:PAD + n_sent].copy(),
            spans[PAD:PAD + 2 * n].reshape(-1, 2).copy(), word[PAD:PAD + n].copy() if with_word else None)


def check(dev, trie, sents, want, name, runners=(run_host, run_dev)):
    """want = (ids, offsets, status, spans in code points, spans in bytes, word), as WpSpanModel.batch returns them"""
    text, off = pack(sents)
    base = trie.encode(text, off)
    for k, what in enumerate(("ids", "offsets", "statuses")):
        assert np.array_equal(base[k], want[k]), "swt_wp_encode: %s differ from the expected (%s)" % (what, name)
    for runner in runners:
        for codepoints in (True, False):
            got = runner(dev, trie, text, off, codepoints)
            tag = "%s, %s, %s" % (name, runner.__name__, "code points" if codepoints else "bytes")
            for k, what in enumerate(("ids", "offsets", "statuses")):
                assert got[k].dtype == base[k].dtype and np.array_equal(got[k], base[k]), "%s differ from swt_wp_encode's (%s)" % (what, tag)
            bad = np.flatnonzero((got[3] != want[3 if codepoints else 4]).any(axis=1))
            assert bad.size == 0, "span of token %d: %s, expected %s (%s)" % (bad[0], got[3][bad[0]], want[3 if codepoints else 4][bad[0]], tag)
            assert np.array_equal(got[4], want[5]), "word indices differ (%s)" % tag


# ------------------------------------------------------------------------------------------------- the reference's rows

@functools.lru_cache(maxsize=None)
def fixture_parts():
    """{part: (vocabulary, texts, expected as WpSpanModel.batch returns it, built from the fixture rows alone)}"""
    from subword_tokenizers_amd import synth
    from tests.conftest import load_golden

    fx = load_golden("fastwp_spans.json")
    pan = load_golden("ref/data/pan_tadeusz.json")[:fx["pan"]["n"]]
    out = {}
    for part, vocab, texts, rows in (("pan", sorted(set(synth.pretrained_vocab())), pan, fx["pan"]["rows"]),
                                     ("fuzz", sorted(set(fx["fuzz"]["vocab"])), [r["text"] for r in fx["fuzz"]["rows"]], fx["fuzz"]["rows"])):
        index = {t: i for i, t in enumerate(vocab)}
        index[UNK] = len(vocab)
        ids, off, cp, by, wd = [], [0], [], [], []
        for text, row in zip(texts, rows):
            low = text.lower()
            pre = np.concatenate([[0], np.cumsum([len(c.encode("utf-8")) for c in low], dtype=np.int64)]).astype(np.int64)
            ids += [index[t] for t in row["tokens"]]
            cp += row["spans"]
            by += [int(pre[x]) for x in row["spans"]]
            wd += row["word"]
            off.append(len(ids))
        want = (np.array(ids, dtype=np.uint32), np.array(off, dtype=np.uint64), np.zeros(len(texts), dtype=np.uint8),
                np.array(cp, dtype=np.uint32).reshape(-1, 2), np.array(by, dtype=np.uint32).reshape(-1, 2), np.array(wd, dtype=np.uint32))
        out[part] = (vocab, texts, want)
    return out


@pytest.mark.parametrize("part", ["pan", "fuzz"])
def test_fixture_rows(dev, part):
    """every row of the fixture, one batch and then sentence by sentence, through both calls in both units"""
    vocab, texts, want = fixture_parts()[part]
    trie = dev.WpTrie(vocab)
    lowered = [t.lower() for t in texts]
    check(dev, trie, lowered, want, "fixture part %s" % part)
    for i in range(0, len(texts), 7):  # one sentence per call: the single-launch form over pinned memory
        a, b = int(want[1][i]), int(want[1][i + 1])
        one = (want[0][a:b], np.array([0, b - a], dtype=np.uint64), want[2][i:i + 1], want[3][a:b], want[4][a:b], want[5][a:b])
        check(dev, trie, lowered[i:i + 1], one, "fixture part %s, row %d" % (part, i), runners=(run_host,))


@pytest.mark.parametrize("part", ["pan", "fuzz"])
def test_python_methods(swt, dev, part):
    """FastWP.fast_encode_spans_batch and FastWP.fast_tokenize_with_offsets on the texts as the user has them (not lowercased)"""
    from tests.conftest import load_golden

    vocab, texts, want = fixture_parts()[part]
    rows = load_golden("fastwp_spans.json")[part]["rows"]
    tok = swt.FastWP()
    tok.vocab = set(vocab)
    tok._build_trie()
    ids, off, status, spans, word = tok.fast_encode_spans_batch(list(texts))
    assert np.array_equal(ids, want[0]) and np.array_equal(off, want[1]) and not status.any()
    assert np.array_equal(spans, want[3]) and np.array_equal(word, want[5])
    base = tok.encode_ids_batch(list(texts))
    assert np.array_equal(ids, base[0]) and np.array_equal(off, base[1]) and np.array_equal(status, base[2])
    for text, row in list(zip(texts, rows))[::5]:
        got = tok.fast_tokenize_with_offsets(text)
        assert [t for t, _ in got] == row["tokens"] == tok.tokenize(text), text
        assert [x for _, se in got for x in se] == row["spans"], text
    with pytest.raises(TypeError):
        tok.fast_tokenize_with_offsets(b"a")
    with pytest.raises(TypeError):
        tok.fast_encode_spans_batch(["a", 1])


def test_python_methods_refuse_as_tokenize_batch_does(swt, dev):
    """a text the reference does not return from raises, as FastWP.tokenize_batch does; a multi-token corner is spelled out"""
    tok = swt.FastWP()
    tok.vocab = {"a", "##a", ".", "#"}  # '##' is "#", "#", "#", ... for ever
    tok._build_trie()
    assert tok.fast_tokenize_with_offsets("aa a.") == [("a", (0, 1)), ("##a", (1, 2)), ("a", (3, 4)), (".", (4, 5))]
    for text in ("a ##", "a .z"):
        with pytest.raises(RuntimeError):
            tok.tokenize_batch([text])
        with pytest.raises(RuntimeError):
            tok.fast_encode_spans_batch([text])
    tok.vocab = {"a", "#", "###"}  # '##' is "#", "###": two tokens, one id on the device
    tok._build_trie()
    assert tok.tokenize("a ## a") == ["a", "#", "###", "a"]
    assert tok.fast_tokenize_with_offsets("a ## a") == [("a", (0, 1)), ("#", (2, 4)), ("###", (2, 4)), ("a", (5, 6))]
    ids, off, status, spans, word = tok.fast_encode_spans_batch(["a ## a", "", " a"])
    assert ids.tolist() == [2, 5, 2, 2] and off.tolist() == [0, 3, 3, 4] and word.tolist() == [0, 1, 2, 0]
    assert spans.tolist() == [[0, 1], [2, 4], [5, 6], [1, 2]]


# ------------------------------------------------------------------------------------------------- the seams

@functools.lru_cache(maxsize=None)
def handmade_model():
    return WpSpanModel(handmade_vocab())


@functools.lru_cache(maxsize=None)
def seams(caps):
    block, chunk, tile, direct_bytes, direct_sents = caps
    assert block == 64
    return seam_batches(chunk, tile, direct_bytes, direct_sents)


@pytest.fixture(scope="module")
def handmade_trie(dev):
    return dev.WpTrie(handmade_model().tokens)


@pytest.mark.parametrize("part", range(STRADDLE_PARTS))
def test_byte_straddles(dev, caps, handmade_trie, part):
    """a 2- and a 4-byte character, a punctuation character and 'a.b' across a 64-byte block, the tile boundary and the end of
    the staged bytes, at pads 0..19 (off0 != 0): spans are relative to the sentence, not to the chunk"""
    batches = [b for b in seams(caps) if b[0].startswith("straddle")]
    assert len(batches) == 120
    for name, sents in batches[part::STRADDLE_PARTS]:
        check(dev, handmade_trie, sents, handmade_model().batch(sents), name)


def test_forms(dev, caps, handmade_trie):
    """the one-lane walk in global memory, the direct form's limits, phases C and D mixed, runs of empty sentences"""
    batches = [b for b in seams(caps) if not b[0].startswith("straddle")]
    assert len(batches) >= 11
    total = sum(nbytes(s) for _, sents in seams(caps) for s in sents)
    assert total < 1 << 20
    for name, sents in batches:
        check(dev, handmade_trie, sents, handmade_model().batch(sents), name)


def test_dedup_knob_is_ignored(dev, caps):
    """SWT_OPT_DEDUP forced on: swt_wp_encode takes the word-level dedup pipeline, the spans call must not (a unique chunk has no
    position) and still returns the same ids"""
    trie = dev.WpTrie(handmade_model().tokens)
    name, sents = [b for b in seams(caps) if b[0].startswith("6 KB")][0]
    want = handmade_model().batch(sents)
    trie.set_option(dev.OPT_DEDUP, dev.DEDUP_ALWAYS)
    check(dev, trie, sents, want, name + ", dedup forced on")
    check(dev, trie, sents[:3], handmade_model().batch(sents[:3]), name + ", dedup forced on, three sentences")
    trie.set_option(dev.OPT_DEDUP, dev.DEDUP_NEVER)
    check(dev, trie, sents, want, name + ", dedup off")


# ------------------------------------------------------------------------------------------------- malformed UTF-8 (bytes only)

def test_malformed_utf8_is_safe(dev, caps, handmade_trie):
    """stray continuation bytes and a lead byte clipped at a sentence end, in the direct and in the tiled form.  No golden: the ids
    are swt_wp_encode's, every span lies in its sentence, starts and word indices do not decrease, the sentinels stay intact"""
    import random

    rng = random.Random(77)
    W = handmade_words()
    bad = [b"ab\x80\x80 cd", b"\x80ab", b"ab \xc5", b"\xbc\xc3\xb3 ab", b"x \xf0\x9f", b"\x98\x80 a.b", b"a\xe2\x82", b"\xac.", b"\xff ab \xfe",
           b"a.\x80b", b"\xc5"]
    for total in (0, caps[3] + 700):
        sents = list(bad)
        while sum(len(s) for s in sents) < total:
            sents += [fill(W.plain + W.soft, 300, rng).encode("utf-8"), rng.choice(bad)]
        text, off = pack(sents)
        base = handmade_trie.encode(text, off)
        for runner in (run_host, run_dev):
            ids, out_off, status, spans, word = runner(dev, handmade_trie, text, off, False)
            assert np.array_equal(ids, base[0]) and np.array_equal(out_off, base[1]) and np.array_equal(status, base[2])
            spans = spans.astype(np.int64)
            for s in range(len(sents)):
                a, b = int(out_off[s]), int(out_off[s + 1])
                sp, wd = spans[a:b], word[a:b].astype(np.int64)
                assert (sp[:, 0] <= sp[:, 1]).all() and (sp[:, 1] <= len(sents[s])).all(), (s, sents[s], sp)
                assert (np.diff(sp[:, 0]) >= 0).all() and (np.diff(wd) >= 0).all(), (s, sents[s], sp, wd)
                assert b == a or (wd[0] == 0 and wd[-1] < b - a), (s, wd)


# ------------------------------------------------------------------------------------------------- arguments

def test_arguments(dev, handmade_trie):
    sents = ["ab a.b", "", "x,y żół"]
    text, off = pack(sents)
    want = handmade_model().batch(sents)
    for runner in (run_host, run_dev):
        got = runner(dev, handmade_trie, text, off, True, with_word=False)  # NULL word: accepted, nothing written there
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[3], want[3]) and got[4] is None
        none, off0 = np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64)
        got = runner(dev, handmade_trie, none, off0, True)  # n_sent = 0
        assert got[0].size == 0 and got[1].tolist() == [0] and got[3].shape == (0, 2)
    p = dev.ptr
    ids, out_off, status, nt = np.zeros(16, np.uint32), np.zeros(4, np.uint64), np.zeros(3, np.uint8), np.zeros(1, np.uint64)
    args = (handmade_trie._h, p(text, dev.u8p), p(off, dev.u64p), 3, p(ids, dev.u32p), 16, p(out_off, dev.u64p), p(status, dev.u8p), p(nt, dev.u64p))
    assert dev.lib().swt_wp_encode_spans(*args, dev.SPAN_CODEPOINTS, None, None) == dev.ERR_INVALID  # NULL spans
    spans = np.zeros(32, np.uint32)
    assert dev.lib().swt_wp_encode_spans(*args, 2, p(spans, dev.u32p), None) == dev.ERR_INVALID  # an unknown flag
    assert dev.lib().swt_wp_encode_spans_dev(handmade_trie._h, None, 0, None, 0, None, None, None, None, 0, None, None, None) == dev.ERR_INVALID
