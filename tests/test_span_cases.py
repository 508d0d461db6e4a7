"""Token spans without a GPU: tests/span_cases.py reproduces what the imported reference recorded (tests/golden/spans.json), its
seam builders put the characters where they say, the length tables are right, and swt_token_spans checks its arguments before it
looks for a device."""
import ctypes as C

import numpy as np
import pytest

from tests import codepoint_cases as K
from tests import span_cases as P

UNK = "[UNK]"


def _sentences(golden):
    """(model, lowercase text, recorded offsets, tokens per word) of every sentence of the fixture"""
    fx = golden("spans.json")
    pan = golden(fx["pan"]["texts_ref"])[:fx["pan"]["n"]]
    for part, texts in (("pan", pan), ("fuzz", fx["fuzz"]["texts"])):
        for model in ("FastBPE", "NaiveWP"):
            for text, off, words in zip(texts, fx[part]["offsets"], fx[part][model]):
                yield model, text.lower(), off, words


def test_fixture_shape(golden):
    fx = golden("spans.json")
    assert fx["pan"]["n"] == 200 and len(fx["pan"]["offsets"]) == 200
    n = len(fx["fuzz"]["texts"])
    assert n >= 100 and fx["fuzz"]["dropped"] * 10 <= n + fx["fuzz"]["dropped"]
    joined = "".join(fx["fuzz"]["texts"])
    for ch in "  　İ́«»—\U0001F600":
        assert ch in joined
    assert any(UNK in w for row in fx["fuzz"]["NaiveWP"] for w in row)
    assert any(len(w) > 1 for row in fx["fuzz"]["NaiveWP"] for w in row)


def test_expected_spans_reproduces_the_reference(golden):
    n = 0
    for model, text, off, words in _sentences(golden):
        # the split: preprocessing's offsets
        assert [x for se in P.word_spans(text) for x in se] == off, text
        got = P.expected_spans(text, [t for w in words for t in w], UNK)
        assert got is not None, (model, text)
        spans, wid = got
        at = 0
        for k, toks in enumerate(words):
            s, e = off[2 * k], off[2 * k + 1]
            mine = spans[at:at + len(toks)]
            # the word's tokens tile its span, and every span cut from the text spells its token
            assert mine[0][0] == s and mine[-1][1] == e and all(a[1] == b[0] for a, b in zip(mine, mine[1:]))
            assert wid[at:at + len(toks)] == [k] * len(toks)
            for tok, (a, b) in zip(toks, mine):
                assert tok == UNK and (a, b) == (s, e) or text[a:b] == P.token_body(tok)
            at += len(toks)
        assert at == len(spans)
        n += 1
    assert n >= 600


def test_istanbul_has_nine_code_points():
    text = "İstanbul x€y".lower()
    assert P.word_spans(text) == [(0, 9), (10, 13)]  # U+20AC is a currency sign, not punctuation
    toks = ["i", "##\u0307", "##stan", "##bul", "x", "##€", "##y"]
    spans, wid = P.expected_spans(text, toks)
    assert spans == [(0, 1), (1, 2), (2, 6), (6, 9), (10, 11), (11, 12), (12, 13)] and wid == [0, 0, 0, 0, 1, 1, 1]
    assert P.to_bytes(text, spans)[1] == (1, 3) and P.to_bytes(text, spans)[5] == (12, 15)


def test_expectation_rejects_what_does_not_tile():
    text = "ab cd"
    ok = [(1, False), (1, True), (2, False)]
    assert P.spans_from_lengths(text, ok) == ([(0, 1), (1, 2), (3, 5)], [0, 0, 1])
    assert P.spans_from_lengths(text, [(0, False), (0, False)]) == ([(0, 2), (3, 5)], [0, 1])
    for bad in ([(2, False)], ok + [(1, False)], [(1, False), (2, False)], [(1, True), (1, True), (2, False)],
                [(0, False), (1, True), (2, False)], [(1, False), (0, True), (2, False)], [(2, False), (None, False)]):
        assert P.spans_from_lengths(text, bad) is None
    cases = dict(P.mismatch_batches())
    assert len(cases) == 20
    for name, b in cases.items():
        status = b.expected()[2]
        assert status.tolist() == [0, 0, 0, 1, 0, 0], name
        for flagged in (True, False):
            text_u8, off, ids, tok_off = P.packed_with_holes(b, flagged)
            assert ids.size == int(tok_off[-1])
    assert sum(len(k) > 64 for _, b in cases.items() for k in b.toks) >= 8


def test_hand_made_ids_follow_the_header():
    for flagged in (True, False):
        table, base = P.length_table(flagged)
        b = P.Batch("x", ["abc d€."], [[(2, False), (1, True), (0, False), (1, False)]])
        _, _, ids, _ = b.packed(flagged)
        for tid, (length, cont) in zip(ids.tolist(), b.toks[0]):
            s = tid & 0x7FFFFFFF
            entry = 1 if s < base else int(table[s - base])
            assert entry & 0xFFFFFF == length
            assert bool(tid >> 31 if flagged else (entry >> 31 if s >= base else 0)) == cont
        assert P.NO_LENGTH_ID[flagged] - base == table.size
    assert ids_of("abc", [(1, False), (1, True), (1, True)]) == [97, 98 | P.CONT, 99 | P.CONT]


def ids_of(text, toks):
    return P.make_ids(text, toks, True)


def test_seam_builders_place_the_character(native):
    block, chunk, tile = native.token_spans_capacity()
    assert 0 < block < chunk <= tile and chunk % block == 0
    pos = P.seam_positions(block, chunk, tile)
    chars = P.seam_characters()
    assert {name[:-1] for name, _ in chars} >= {"letter", "bert_ws", "bert_punct"}
    for name, ch in chars[:6]:
        for role in P.ROLES:
            for d in P.OFFSETS:
                b = P.seam_batch(role, ch, d, pos)
                data = b"".join(K.utf8(t) for t in b.texts)
                lead = K.utf8(ch)
                assert len(b.leads) == len(pos), (name, role, d)
                for at in b.leads:
                    assert data[at:at + len(lead)] == lead
                if role == "sentence":
                    starts = set(np.cumsum([0] + [K.nbytes(t) for t in b.texts]).tolist())
                    assert set(b.leads) <= starts
                else:
                    assert K.nbytes(b.texts[0]) > 2 * tile
                spans, word, status = b.expected()
                assert not status.any() and spans.shape[0] == sum(len(k) for k in b.toks)
    letter = P.seam_batch("token", "a", 0, pos)
    text, (spans, _) = letter.texts[0], P.spans_from_lengths(letter.texts[0], letter.toks[0])
    cps = {len(K.utf8(text)[:at].decode()) for at in letter.leads}
    assert cps <= {s for s, _ in spans}  # a token starts at the placed letter
    for b in (P.long_word_batch(), P.punct_words_batch(), P.long_tokens_batch(chunk)):
        assert not b.expected()[2].any()
        assert max(K.nbytes(t) for t in b.texts) > min(3 * tile, chunk)
    assert K.nbytes(P.long_word_batch().texts[1]) > 3 * tile and len(P.punct_words_batch().toks[1]) >= 40000 - 22


def test_length_tables(swt, native):
    tokens = sorted({"a", "##a", "ab", "##abc", "€", "##żółć", "#", "[UNK]"})
    t = native.wp_length_table(tokens)
    assert t.dtype == np.uint32 and t.size == len(tokens) + 2
    at = dict(zip(tokens, t.tolist()))
    assert at["a"] == 1 and at["ab"] == 2 and at["€"] == 1 and at["#"] == 1 and at["[UNK]"] == 5
    assert at["##a"] == 1 | native.SPAN_LEN_CONT and at["##abc"] == 3 | native.SPAN_LEN_CONT
    assert at["##żółć"] == 4 | native.SPAN_LEN_CONT
    assert t[-2:].tolist() == [native.SPAN_WHOLE_WORD, native.SPAN_WHOLE_WORD]
    assert native.bpe_length_table(["ab", "żół", "##"]).tolist() == [2, 3, 2]
    # the tables follow their tokenizer's: a rebuilt symbol table or vocabulary gets a new one
    bpe = swt.FastBPE()
    bpe.merges_list = [("a", "b"), ("ab", "c")]
    bpe._build_table()
    assert bpe._span_lengths(bpe._syms).tolist() == [2, 3]
    bpe.merges_list = [("a", "b")]
    bpe._build_table()
    assert bpe._span_lengths(bpe._syms).tolist() == [2]
    wp = swt.NaiveWP()
    wp.vocab = {"a", "##bc"}
    wp._ensure_naive_trie()
    assert wp._span_lengths().tolist() == [2 | native.SPAN_LEN_CONT, 1, 0, 0]
    wp.vocab.add("abc")
    wp._ensure_naive_trie()
    assert wp._span_lengths().tolist() == [2 | native.SPAN_LEN_CONT, 1, 3, 0, 0]
    assert not hasattr(swt.FastWP, "tokenize_with_offsets") or "tokenize_with_offsets" not in vars(swt.FastWP)


def _call(native, text, off, ids, tok_off, table, spans, word, status, n_sent=None):
    p = lambda a, t: native.ptr(a, t) if a is not None else None
    n = len(off) - 1 if n_sent is None else n_sent
    return native.lib().swt_token_spans(p(text, native.u8p), p(off, native.u64p), n, p(ids, native.u32p), p(tok_off, native.u64p),
                                        p(table, native.u32p), 0, 6, 0, native.SPAN_CODEPOINTS,
                                        p(spans, native.u32p), p(word, native.u32p), p(status, native.u8p))


def test_arguments_are_checked_before_the_device(native):
    text = np.frombuffer(b"ab cd", dtype=np.uint8)
    off = np.array([0, 2, 5], dtype=np.uint64)
    ids = np.array([4, 4], dtype=np.uint32)
    tok_off = np.array([0, 1, 2], dtype=np.uint64)
    table = np.array([0, 0, 1, 1, 2, 2], dtype=np.uint32)
    spans, word, status = np.zeros(4, dtype=np.uint32), np.zeros(2, dtype=np.uint32), np.zeros(2, dtype=np.uint8)
    good = [text, off, ids, tok_off, table, spans, word, status]
    for missing in (0, 1, 2, 3, 4, 5, 7):  # word (6) may be NULL
        args = list(good)
        args[missing] = None
        assert _call(native, *args, n_sent=2) == native.ERR_INVALID, missing
        assert b"null" in native.lib().swt_last_error()
    for bad_off in (np.array([0, 3, 2], dtype=np.uint64), np.array([2, 0, 5], dtype=np.uint64)):
        assert _call(native, text, bad_off, ids, tok_off, table, spans, word, status) == native.ERR_INVALID
        assert _call(native, text, off, ids, bad_off, table, spans, word, status) == native.ERR_INVALID
    huge = np.array([0, 1 << 32], dtype=np.uint64)
    assert _call(native, text, huge, ids, np.array([0, 2], dtype=np.uint64), table, spans, word, status) == native.ERR_INVALID
    assert native.lib().swt_token_spans(native.ptr(text, native.u8p), native.ptr(off, native.u64p), 2, native.ptr(ids, native.u32p),
                                        native.ptr(tok_off, native.u64p), native.ptr(table, native.u32p), 0, 6, 0, 2,
                                        native.ptr(spans, native.u32p), None, native.ptr(status, native.u8p)) == native.ERR_INVALID
    a, b, c = C.c_uint32(), C.c_uint32(), C.c_uint32()
    assert native.lib().swt_token_spans_capacity(C.byref(a), None, C.byref(c)) == 0 and a.value and c.value >= a.value
    assert native.lib().swt_token_spans_dev(None, 0, None, 1, None, None, None, 0, 0, 0, 0, None, None, None, None) == native.ERR_INVALID


def test_no_device_is_an_error_not_a_fallback(swt, native):
    if native.device_count() > 0:
        pytest.skip("a device is present: the no-device answer cannot be seen here")
    text = np.frombuffer(b"ab cd", dtype=np.uint8)
    off = np.array([0, 5], dtype=np.uint64)
    ids = np.array([4, 4], dtype=np.uint32)
    tok_off = np.array([0, 2], dtype=np.uint64)
    table = np.array([0, 0, 1, 1, 2, 2], dtype=np.uint32)
    spans, word, status = np.zeros(4, dtype=np.uint32), np.zeros(2, dtype=np.uint32), np.zeros(1, dtype=np.uint8)
    assert _call(native, text, off, ids, tok_off, table, spans, word, status) == native.ERR_NO_DEVICE
    with pytest.raises(native.NoDeviceError):
        native.token_spans(text, off, ids, tok_off, table, 0, False)
    bpe = swt.FastBPE()
    bpe.merges_list = [("a", "b")]
    wp = swt.NaiveWP()
    wp.vocab = {"a", "##b"}
    for tok in (bpe, wp):
        with pytest.raises(native.NoDeviceError):
            tok.encode_spans_batch(["ab ab"])
        with pytest.raises(native.NoDeviceError):
            tok.tokenize_with_offsets("ab")
        with pytest.raises(TypeError):
            tok.encode_spans_batch("ab")
        with pytest.raises(TypeError):
            tok.encode_spans_batch(["ab", 3])
