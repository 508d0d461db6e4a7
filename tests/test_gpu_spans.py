"""Token spans on the device (csrc/swt_spans.hip): swt_token_spans / swt_token_spans_dev and the encode_spans_batch /
tokenize_with_offsets methods against tests/span_cases.py (the split from the class-table fixture, the spans from walking the
tokens) and against what the imported reference recorded (tests/golden/spans.json)."""
import os

import numpy as np
import pytest

from tests import codepoint_cases as K
from tests import span_cases as P

pytestmark = pytest.mark.gpu

UNK = "[UNK]"
SENTINEL = 0xDEADBEEF
PAD = 8


@pytest.fixture(scope="module")
def dev(native):
    if native.device_count() < 1:
        pytest.fail("no HIP device")
    native.init(0)
    return native


@pytest.fixture(scope="module")
def caps(dev):
    return dev.token_spans_capacity()


def run_host(dev, packed, flagged, codepoints, table=None):
    """swt_token_spans with sentinel words around the three outputs -> (spans int64[n, 2], word int64[n], status)"""
    text, off, ids, tok_off = packed
    if table is None:
        table = P.length_table(flagged)
    tab, base = table
    n, n_sent = int(ids.size), int(off.size) - 1
    spans = np.full(2 * n + 2 * PAD, SENTINEL, dtype=np.uint32)
    word = np.full(n + 2 * PAD, SENTINEL, dtype=np.uint32)
    status = np.full(n_sent + 2 * PAD, 0xEE, dtype=np.uint8)
    p = dev.ptr
    rc = dev.lib().swt_token_spans(p(text, dev.u8p) if text.size else None, p(off, dev.u64p), n_sent, p(ids, dev.u32p) if n else None,
                                   p(tok_off, dev.u64p), p(tab, dev.u32p), base, tab.size, int(flagged),
                                   dev.SPAN_CODEPOINTS if codepoints else 0, p(spans[PAD:], dev.u32p), p(word[PAD:], dev.u32p),
                                   p(status[PAD:], dev.u8p))
    dev.check(rc)
    for a in (spans, word):
        assert (a[:PAD] == SENTINEL).all() and (a[a.size - PAD:] == SENTINEL).all()
    assert (status[:PAD] == 0xEE).all() and (status[status.size - PAD:] == 0xEE).all()
    return spans[PAD:PAD + 2 * n].reshape(-1, 2).astype(np.int64), word[PAD:PAD + n].astype(np.int64), status[PAD:PAD + n_sent].copy()


def run_dev(dev, packed, flagged, codepoints, fill=0x5A, table=None, with_word=True):
    """swt_token_spans_dev on torch tensors and a side stream, the outputs pre-filled with garbage and fenced by sentinels"""
    import torch

    text, off, ids, tok_off = packed
    tab, base = table if table is not None else P.length_table(flagged)
    n, n_sent = int(ids.size), int(off.size) - 1
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt).copy()).cuda()
    d_text = up(np.concatenate([text, np.zeros(16, np.uint8)]), np.uint8)
    d_off, d_tok_off = up(off, np.int64), up(tok_off, np.int64)
    d_ids = up(np.concatenate([ids, np.zeros(4, np.uint32)]), np.int32)
    d_tab = up(np.concatenate([tab, np.zeros(4, np.uint32)]), np.int32)
    garbage = int(np.array([fill * 0x01010101], dtype=np.uint32).view(np.int32)[0])
    sent = int(np.array([SENTINEL], dtype=np.uint32).view(np.int32)[0])
    d_spans = torch.full((2 * n + 2 * PAD,), garbage, dtype=torch.int32, device="cuda")
    d_word = torch.full((n + 2 * PAD,), garbage, dtype=torch.int32, device="cuda")
    d_status = torch.full((n_sent + 2 * PAD,), fill, dtype=torch.uint8, device="cuda")
    for t in (d_spans, d_word):
        t[:PAD] = sent
        t[t.numel() - PAD:] = sent
    d_status[:PAD] = 0xEE
    d_status[d_status.numel() - PAD:] = 0xEE
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        rc = dev.lib().swt_token_spans_dev(d_text.data_ptr(), int(text.size), d_off.data_ptr(), n_sent, d_ids.data_ptr(), d_tok_off.data_ptr(),
                                           d_tab.data_ptr(), base, tab.size, int(flagged), dev.SPAN_CODEPOINTS if codepoints else 0,
                                           d_spans.data_ptr() + 4 * PAD, (d_word.data_ptr() + 4 * PAD) if with_word else None,
                                           d_status.data_ptr() + PAD, stream.cuda_stream)
    dev.check(rc)
    stream.synchronize()
    spans, word, status = (t.cpu().numpy() for t in (d_spans, d_word, d_status))
    spans, word = spans.view(np.uint32), word.view(np.uint32)
    for a in (spans, word):
        assert (a[:PAD] == SENTINEL).all() and (a[a.size - PAD:] == SENTINEL).all()
    assert (status[:PAD] == 0xEE).all() and (status[status.size - PAD:] == 0xEE).all()
    if not with_word:
        assert (word[PAD:PAD + n] == np.uint32(fill * 0x01010101)).all()
    return spans[PAD:PAD + 2 * n].reshape(-1, 2).astype(np.int64), word[PAD:PAD + n].astype(np.int64), status[PAD:PAD + n_sent].copy()


def check_batch(dev, batch, flagged, units=(True, False), runner=run_host, packed=None):
    packed = packed if packed is not None else batch.packed(flagged)
    for codepoints in units:
        want_spans, want_word, want_status = batch.expected(codepoints)
        spans, word, status = runner(dev, packed, flagged, codepoints)
        assert status.tolist() == want_status.tolist(), (batch.name, flagged, codepoints)
        bad = np.flatnonzero((spans != want_spans).any(axis=1) | (word != want_word))
        assert bad.size == 0, (batch.name, flagged, codepoints, int(bad[0]), spans[bad[0]].tolist(), want_spans[bad[0]].tolist(),
                               int(word[bad[0]]), int(want_word[bad[0]]))


# ------------------------------------------------------------------------------------------------------------ 1. golden

@pytest.fixture(scope="module")
def fixture_rows(golden):
    fx = golden("spans.json")
    pan = golden(fx["pan"]["texts_ref"])[:fx["pan"]["n"]]
    return {"pan": (pan, fx["pan"]), "fuzz": (fx["fuzz"]["texts"], fx["fuzz"])}


def _want(texts, part, model):
    """tokens, code-point spans, byte spans and word ids the fixture implies, flat over the sentences, and the token offsets"""
    toks, spans, bspans, wid, off = [], [], [], [], [0]
    for text, words in zip(texts, part[model]):
        low = text.lower()
        flat = [t for w in words for t in w]
        s, w = P.expected_spans(low, flat, UNK)
        assert [x for se in P.word_spans(low) for x in se] == part["offsets"][len(off) - 1]
        toks += flat
        spans += s
        bspans += P.to_bytes(low, s)
        wid += w
        off.append(len(toks))
    return toks, np.array(spans).reshape(-1, 2), np.array(bspans).reshape(-1, 2), np.array(wid), off


@pytest.mark.parametrize("part", ["pan", "fuzz"])
@pytest.mark.parametrize("cls", ["FastBPE", "NaiveBPE"])
def test_golden_bpe(swt, dev, ref_dir, fixture_rows, cls, part):
    texts, rows = fixture_rows[part]
    tok = getattr(swt, cls)()
    tok.load_resources(os.path.join(ref_dir, "resources/pretrained/FastBPE"))
    toks, spans, bspans, wid, off = _want(texts, rows, "FastBPE")
    ids, tok_off, got_spans, got_word = tok.encode_spans_batch(list(texts))
    assert tok_off.tolist() == off and tok.decode_ids(ids) == toks
    assert np.array_equal(got_spans, spans) and np.array_equal(got_word, wid)
    # the same ids in bytes, through the binding
    text, t_off = dev.pack_and_lower(list(texts))
    _, syms = tok._span_parts()
    b_spans, b_word, status = dev.token_spans(text, t_off, ids, tok_off, tok._span_lengths(syms), dev.SYM_BASE, True, codepoints=False)
    assert not status.any() and np.array_equal(b_spans, bspans) and np.array_equal(b_word, wid)


@pytest.mark.parametrize("part,vocab", [("pan", "pretrained"), ("fuzz", "tests")])
def test_golden_naive_wp(swt, dev, ref_dir, golden, fixture_rows, part, vocab):
    texts, rows = fixture_rows[part]
    tok = swt.NaiveWP()
    tok.vocab = set(golden("ref/resources/%s/FastWordPiece/vocab.json" % vocab))
    toks, spans, bspans, wid, off = _want(texts, rows, "NaiveWP")
    ids, tok_off, status, got_spans, got_word = tok.encode_spans_batch(list(texts))
    names = tok._naive_tokens + ["['UNK']", UNK]
    assert not status.any() and tok_off.tolist() == off and [names[i] for i in ids.tolist()] == toks
    assert np.array_equal(got_spans, spans) and np.array_equal(got_word, wid)
    text, t_off = dev.pack_and_lower(list(texts))
    b_spans, b_word, st = dev.token_spans(text, t_off, ids, tok_off, tok._span_lengths(), 0, False, codepoints=False)
    assert not st.any() and np.array_equal(b_spans, bspans) and np.array_equal(b_word, wid)
    if part == "fuzz":
        assert UNK in toks


# ------------------------------------------------------------------------------------------------------------- 2. seams

@pytest.mark.parametrize("name,ch", P.seam_characters(), ids=[n for n, _ in P.seam_characters()])
@pytest.mark.parametrize("role", P.ROLES)
def test_seams(dev, caps, role, name, ch):
    pos = P.seam_positions(*caps)
    for i, d in enumerate(P.OFFSETS):
        batch = P.seam_batch(role, ch, d, pos)
        assert len(batch.leads) == len(pos)
        check_batch(dev, batch, flagged=bool(i % 2) ^ (role in ("word", "whole")))


def test_long_sentences(dev, caps):
    block, chunk, tile = caps
    for batch in (P.long_word_batch(), P.punct_words_batch(), P.long_tokens_batch(chunk)):
        assert max(K.nbytes(t) for t in batch.texts) > chunk
        for flagged in (True, False):
            check_batch(dev, batch, flagged)
    assert K.nbytes(P.long_word_batch().texts[1]) > 3 * tile and K.nbytes(P.punct_words_batch().texts[1]) > 3 * tile


def test_long_sentences_dev_form(dev, caps):
    for batch in (P.long_word_batch(), P.punct_words_batch()):
        check_batch(dev, batch, True, units=(False,), runner=run_dev)


# -------------------------------------------------------------------------------------------------------- 3. degenerate

def test_no_sentences(dev):
    empty = (np.zeros(0, np.uint8), np.zeros(1, np.uint64), np.zeros(0, np.uint32), np.zeros(1, np.uint64))
    spans, word, status = run_host(dev, empty, True, True)
    assert spans.shape == (0, 2) and word.size == 0 and status.size == 0
    spans, word, status = dev.token_spans(*empty, np.zeros(0, np.uint32), 0, False)
    assert spans.shape == (0, 2) and word.size == 0 and status.size == 0


def test_empty_sentences_in_a_row(dev):
    texts = [""] * 2500 + ["ab cd. abcd"] + [""] * 2500
    batch = P.Batch("empties", texts, [P.segment(t, None, "pairs") for t in texts])
    assert len(texts) == 5001 and sum(len(k) for k in batch.toks) == 5
    for flagged in (True, False):
        check_batch(dev, batch, flagged)
    check_batch(dev, batch, True, runner=run_dev)
    only = P.Batch("only-empties", [""] * 70, [[]] * 70)
    check_batch(dev, only, True)
    check_batch(dev, only, False, runner=run_dev)


def test_whitespace_and_single_marks(dev):
    texts = [" ", "\t   　", "", ".", "—", "   ", "a", " . ", "　ab "]
    batch = P.Batch("blank", texts, [P.segment(t, None, "one") for t in texts])
    assert [len(k) for k in batch.toks] == [0, 0, 0, 1, 1, 0, 1, 1, 1]
    for flagged in (True, False):
        check_batch(dev, batch, flagged)
    # tokens for a sentence that has no word
    bad = P.Batch("blank-with-token", texts, [[(1, False)]] + batch.toks[1:])
    assert bad.expected()[2].tolist() == [1] + [0] * 8
    check_batch(dev, bad, False)


def test_every_alignment_of_a_sentence_start(dev, caps):
    l3, l4 = K.giant_letters()
    body = "abé" + l3 + l4 + ". cd" + l4 + "ab —" + l3
    import random
    rng = random.Random(16)
    texts = []
    for a in range(16):
        texts += ["q" * ((a - sum(map(K.nbytes, texts))) % 16 or 16), body * 3 + "x" * a]
    starts = np.cumsum([0] + [K.nbytes(t) for t in texts])[:-1]
    assert {int(s) % 16 for s in starts[1::2]} == set(range(16))
    batch = P.Batch("alignments", texts, [P.segment(t, rng) for t in texts])
    for flagged in (True, False):
        check_batch(dev, batch, flagged)
    # and a chunk's worth behind every alignment
    long = [t + " " + K.giant(caps[1] + 40) for t in texts]
    check_batch(dev, P.Batch("alignments-long", long, [P.segment(t, rng) for t in long]), True)


# ---------------------------------------------------------------------------------------------------------- 4. mismatch

@pytest.mark.parametrize("case,batch", P.mismatch_batches(), ids=[c for c, _ in P.mismatch_batches()])
def test_mismatch(dev, case, batch):
    want_status = batch.expected()[2]
    assert want_status.tolist() == [0, 0, 0, 1, 0, 0]
    for flagged in (True, False):
        packed = P.packed_with_holes(batch, flagged)
        check_batch(dev, batch, flagged, packed=packed)                  # sentinels around the host arrays
        check_batch(dev, batch, flagged, packed=packed, runner=run_dev)  # ... and around the device arrays
    spans, word, _ = run_dev(dev, P.packed_with_holes(batch, True), True, False)
    lo, hi = (sum(len(k) for k in batch.toks[:i]) for i in (3, 4))
    assert not spans[lo:hi].any() and not word[lo:hi].any()
    assert spans[:lo].any() and spans[hi:].any()


def test_ids_of_another_text_are_safe(dev):
    """ids and lengths that have nothing to do with the text: every sentence is a mismatch or happens to tile, nothing else is touched"""
    rng = np.random.default_rng(3)
    texts = ["ab cd. " * int(k) for k in rng.integers(0, 30, size=40)]
    text, off = K.pack(texts)
    n = rng.integers(0, 200, size=40)
    tok_off = np.zeros(41, dtype=np.uint64)
    np.cumsum(n, out=tok_off[1:])
    ids = rng.integers(0, 2 * (P.MAX_LEN + 3), size=int(tok_off[-1])).astype(np.uint32)
    for flagged in (False, True):
        use = ids if not flagged else (ids % 7 + P.SYM_BASE).astype(np.uint32) | np.where(ids & 1, P.CONT, 0).astype(np.uint32)
        for runner in (run_host, run_dev):
            spans, word, status = runner(dev, (text, off, use, tok_off), flagged, True)
            assert set(status.tolist()) <= {0, 1}
            for s in np.flatnonzero(status):
                lo, hi = int(tok_off[s]), int(tok_off[s + 1])
                assert not spans[lo:hi].any() and not word[lo:hi].any()
            for s in np.flatnonzero(status == 0):
                lo, hi = int(tok_off[s]), int(tok_off[s + 1])
                assert (spans[lo:hi, 1] <= len(texts[s])).all()


# ---------------------------------------------------------------------------------------------------------- 5. dev form

def test_dev_form_equals_host_form_and_repeats(dev, caps):
    import random
    rng = random.Random(99)
    texts = []
    for k in range(300):
        texts.append(K.fill(K.SHORT + ("żółw", "—", "x\U0001F600y", "ab.cd"), rng.randint(0, 160), rng))
    texts[17] = K.giant(caps[1] + 100) + " ab"
    batch = P.Batch("dev", texts, [P.segment(t, rng) for t in texts])
    for flagged in (True, False):
        packed = batch.packed(flagged)
        for codepoints in (True, False):
            host = run_host(dev, packed, flagged, codepoints)
            want = batch.expected(codepoints)
            assert np.array_equal(host[0], want[0]) and np.array_equal(host[1], want[1]) and not host[2].any()
            first = run_dev(dev, packed, flagged, codepoints, fill=0x5A)
            second = run_dev(dev, packed, flagged, codepoints, fill=0xC3)
            for a, b, c in zip(host, first, second):
                assert np.array_equal(a, b) and np.array_equal(b, c)
    no_word = run_dev(dev, batch.packed(True), True, True, with_word=False)
    assert np.array_equal(no_word[0], batch.expected(True)[0])


# ------------------------------------------------------------------------------------------------------------ 6. Python

def _check_python(tok, texts, ids_spans, names):
    tok_off, spans, word = ids_spans
    pre = tok.preprocessing(texts)
    for i, text in enumerate(texts):
        low = text.lower()
        lo, hi = int(tok_off[i]), int(tok_off[i + 1])
        toks, sp, w = names[lo:hi], spans[lo:hi].tolist(), word[lo:hi].tolist()
        groups = {}
        for t, (s, e), k in zip(toks, sp, w):
            groups.setdefault(k, []).append((t, s, e))
        assert sorted(groups) == list(range(len(pre[i]))) and w == sorted(w), text
        for k, (wtext, (ws, we)) in enumerate(pre[i]):
            g = groups[k]
            assert g[0][1] == ws and g[-1][2] == we and all(a[2] == b[1] for a, b in zip(g, g[1:])), text
            for t, s, e in g:
                assert (t == UNK and low[s:e] == wtext) or low[s:e] == P.token_body(t), (text, t, s, e)


@pytest.mark.parametrize("cls", ["FastBPE", "NaiveBPE"])
def test_python_bpe_on_train5k(swt, dev, ref_dir, corpora, cls):
    texts = corpora["t5k"][:500]
    tok = getattr(swt, cls)()
    tok.load_resources(os.path.join(ref_dir, "resources/pretrained/FastBPE"))
    ids, tok_off, spans, word = tok.encode_spans_batch(texts)
    assert np.array_equal(ids, tok.encode_ids_batch(texts)[0])
    _check_python(tok, texts, (tok_off, spans, word), tok.decode_ids(ids))
    want = [("i", (0, 1)), ("##̇", (1, 2)), ("##stan", (2, 6)), ("##bul", (6, 9)), ("x", (10, 11)), ("##€", (11, 12)), ("##y", (12, 13))]
    if cls == "FastBPE":
        assert tok.tokenize_with_offsets("İstanbul x€y") == want
    else:
        got = tok.tokenize_with_offsets("İstanbul x€y")
        assert [t for t, _ in got] == tok.tokenize("İstanbul x€y") and got[0][1][0] == 0 and got[-1][1][1] == 13
    assert tok.tokenize_with_offsets("") == [] and tok.encode_spans_batch([])[2].shape == (0, 2)


def test_python_naive_wp_on_train5k(swt, dev, golden, corpora):
    texts = corpora["t5k"][:500]
    tok = swt.NaiveWP()
    tok.vocab = set(golden("ref/resources/pretrained/FastWordPiece/vocab.json"))
    status = tok.encode_ids_batch(texts)[2]
    endless = [t for t, s in zip(texts, status.tolist()) if s]
    texts = [t for t, s in zip(texts, status.tolist()) if not s]
    print("NaiveWP on train-5K[:500]: %d sentences on which the reference does not return" % len(endless))
    assert len(texts) >= 250
    if endless:  # such a sentence raises as in tokenize_batch, before any span is asked for
        with pytest.raises(RuntimeError, match="does not terminate"):
            tok.encode_spans_batch(texts[:3] + endless[:1])
    ids, tok_off, st, spans, word = tok.encode_spans_batch(texts)
    names = tok._naive_tokens + ["['UNK']", UNK]
    assert not st.any()
    _check_python(tok, texts, (tok_off, spans, word), [names[i] for i in ids.tolist()])
    got = tok.tokenize_with_offsets(texts[0])
    assert [t for t, _ in got] == tok.tokenize_batch([texts[0]])[0]
    assert [se for _, se in got] == [tuple(x) for x in spans[:int(tok_off[1])].tolist()]
    tiny = swt.NaiveWP()
    tiny.vocab = {"ab", "##c", "."}
    assert tiny.tokenize_with_offsets(" Abc  xyz.") == [("ab", (1, 3)), ("##c", (3, 4)), (UNK, (6, 9)), (".", (9, 10))]
