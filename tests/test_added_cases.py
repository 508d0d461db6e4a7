"""The plain-Python model of added tokens (tests/added_cases.py) against the `tokenizers` wheel's recorded output
(tests/golden/added_tokens.json), the dense-id rule of batching.with_added against the model's, what add_tokens and
swt_added_create refuse, and the library's exports -- all without a device."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import added_cases as A

NAMES = ("swt_added_create", "swt_added_destroy", "swt_added_find", "swt_added_find_dev", "swt_added_splice", "swt_added_splice_dev",
         "swt_added_capacity")
METHODS = ("add_tokens", "add_special_tokens", "added_tokens", "clear_added_tokens")
CLASSES = ("FastBPE", "NaiveBPE", "FastWP", "NaiveWP")


@pytest.fixture(scope="module")
def recorded(golden):
    return golden("added_tokens.json")


def _tokenizer(swt, ref_dir, cls, which="pretrained"):
    tok = getattr(swt, cls)()
    tok.load_resources(os.path.join(ref_dir, "resources", which, "FastBPE" if "BPE" in cls else "FastWordPiece"))
    return tok


# ---- the model against the wheel

def test_golden_is_what_the_generator_would_record(recorded):
    cases = A.golden_cases()
    assert [c["name"] for c in recorded["cases"]] == [name for name, _, _ in cases]
    for rec, (_, added, texts) in zip(recorded["cases"], cases):
        assert rec["added"] == [[c, bool(s)] for c, s in added] and rec["texts"] == texts
    assert sum(len(c["texts"]) for c in recorded["cases"]) >= 45


def test_model_equals_the_wheel(recorded, swt):
    """matches, offsets and word ids of every text of every case; and the wheel's in-between pieces are NaiveWP's over the
    model-blanked text, word for word -- the blanks hide a match and split nothing else"""
    naive = swt.NaiveWP()
    naive.vocab = set(recorded["vocab"])
    index = {tok: i for i, tok in enumerate(recorded["vocab"])}
    index["[UNK]"] = len(recorded["vocab"]) + 1
    base, n_matches = 1000, 0
    for case in recorded["cases"]:
        added = [(c, s) for c, s in case["added"]]
        patterns = A.patterns_of(added)
        strings = [c if s else c.lower() for c, s in added]
        for text, toks, ids, offs, words in zip(case["texts"], case["tokens"], case["ids"], case["offsets"], case["word_ids"]):
            low = text.lower()
            matches = A.find_matches(low, patterns)
            n_matches += len(matches)
            got = [(strings.index(t), o[0], o[1]) for t, i, o in zip(toks, ids, offs) if i < 0]
            assert got == matches, (case["name"], text)
            # the pieces in between, as an encoder gives them over the blanked text: their own words counted from 0
            plain = [(i, tuple(o), w) for i, o, w in zip(ids, offs, words) if i >= 0]
            rank = {w: k for k, w in enumerate(sorted({w for _, _, w in plain}))}
            plain = [(i, o, rank[w]) for i, o, w in plain]
            blanked = A.blank(low, matches)
            assert len(blanked) == len(low) and len(blanked.encode("utf-8")) == len(low.encode("utf-8"))
            pieces = [(tok, (s, e)) for tok, (s, e) in _naive_pieces(swt, naive, blanked)]
            assert [index[t] for t, _ in pieces] == [i for i, _, _ in plain], (case["name"], text)
            want = [(i if i >= 0 else base + strings.index(t), tuple(o), w) for t, i, o, w in zip(toks, ids, offs, words)]
            assert A.splice(plain, matches, base) == want, (case["name"], text)
    assert n_matches > 150


def _naive_pieces(swt, naive, text):
    """NaiveWP.tokenize over the pre-tokenizer's words, with the words' spans (a piece's own span is not needed here)"""
    out = []
    for word, span in naive.preprocessing([text])[0]:
        out.extend((piece, span) for piece in naive.encode_word(word))
    return out


def test_model_by_hand():
    pats = ["ab", "abc", "bcd"]
    assert A.find_matches("abcd", pats) == [(1, 0, 3)]
    assert A.find_matches("abcbcd", pats) == [(1, 0, 3), (2, 3, 6)]
    assert A.find_matches("ababcd", pats) == [(0, 0, 2), (1, 2, 5)]
    assert A.find_matches("examplx example", ["exam", "example"]) == [(0, 0, 4), (1, 8, 15)]  # the longer one fails at its last byte
    assert A.blank("a[é€]b", [(0, 1, 5)]) == "a \u00a0\u2003 b"
    # x<user>x: the second x starts a word
    assert A.splice([(7, (0, 1), 0), (7, (7, 8), 1)], [(0, 1, 7)], 100) == [(7, (0, 1), 0), (100, (1, 7), 1), (7, (7, 8), 2)]
    assert A.splice([], [(2, 0, 6), (2, 6, 12)], 50) == [(52, (0, 6), 0), (52, (6, 12), 1)]
    assert A.splice([(1, (0, 2), 0), (2, (2, 4), 0)], [], 9) == [(1, (0, 2), 0), (2, (2, 4), 0)]


def test_the_deviation_is_pinned():
    """this library lowercases before anything else: "[mask]" in a text is "[MASK]" (the wheel matches special tokens on the raw
    text and would split it into "[", "mask", "]")"""
    added = [("[MASK]", True)]
    assert A.find_matches("paris is the [mask] of france.".lower(), A.patterns_of(added)) == [(0, 13, 19)]
    assert A.find_matches("Paris is the [MASK] of France.".lower(), A.patterns_of(added)) == [(0, 13, 19)]
    tokens, dense = A.dense_ids(["[PAD]", "[UNK]", "[CLS]", "[SEP]", "a"], 5, added)
    assert dense == [5] and tokens == ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "a"]


def test_blanks_are_whitespace_to_the_pre_tokenizer(native):
    for ch in A.BLANKS.values():
        assert native.class_of(ord(ch)) & native.CLS_BERT_WS
    assert [len(ch.encode("utf-8")) for ch in (A.BLANKS[1], A.BLANKS[2], A.BLANKS[3])] == [1, 2, 3]


# ---- the dense-id rule

@pytest.mark.parametrize("cls", CLASSES)
def test_dense_ids(swt, native, ref_dir, cls):
    tok = _tokenizer(swt, ref_dir, cls, "tests" if "WP" in cls else "pretrained")
    base_list, base_mask, base_special = tok.vocab_list(), tok.mask_id(), tok.special_ids()
    base = tok._batch_vocabulary()
    assert base.added_base is None
    assert tok.add_special_tokens(["[MASK]"]) == 1  # rule 1 or 2: nothing is appended
    assert tok.vocab_list() == base_list and tok.mask_id() == base_mask
    assert tok.add_special_tokens(["[SEP]", "[MASK]", "[mask]"]) == 1  # a re-added token, in any case, is not new
    assert tok.vocab_list() == base_list
    assert tok.add_tokens(["<User>", "<|end|>"], special=True) == 2 and tok.add_tokens(["Domain-Term", "ex", "##x"]) == 3
    order = [("[MASK]", True), ("[SEP]", True), ("<User>", True), ("<|end|>", True), ("Domain-Term", False), ("ex", False), ("##x", False)]
    assert tok.added_tokens() == order
    voc = tok._batch_vocabulary()
    tokens, dense = A.dense_ids(base_list, base_mask, order)
    assert tok.vocab_list() == tokens and voc.added_dense.tolist() == dense
    assert tokens[:len(base_list)] == base_list and tok.mask_id() == base_mask and tok.special_ids() == base_special  # no base id moves
    assert dense[0] == base_mask and dense[1] == base_special["sep"]
    assert tokens[base_mask] == "[MASK]"
    assert dense[2] == max(len(base_list), base_mask + 1) and tok.token_to_id("<User>") == dense[2] and tok.token_to_id("domain-term") == dense[4]
    # the encoder-side ids lie past every id of the encoder and map to the dense ids in the map's own convention
    assert voc.added_base >= tok._enc.id_cap() and voc.n_map == voc.added_base + len(order)
    assert voc.cmap.size == (2 if voc.flagged else 1) * voc.n_map
    assert voc.cmap[voc.added_base:voc.n_map].tolist() == dense
    assert np.array_equal(voc.cmap[:base.n_map], base.cmap[:base.n_map])
    if voc.flagged:
        assert np.array_equal(voc.cmap[voc.n_map:voc.n_map + base.n_map], base.cmap[base.n_map:])
        assert (voc.cmap[voc.n_map + base.n_map:] == native.BATCH_NONE).all()  # never flagged with SWT_BPE_CONT
    # classes and decode flags
    cls_tab, flags = voc.cls_tab, voc.decode_tables[2]
    assert cls_tab.size == len(tokens)
    for (content, special), d in zip(order, dense):
        if special:
            assert d == base_mask == len(base_list) or cls_tab[d] == 2
            assert flags[d] & native.TOK_SPECIAL
        elif content.lower() not in base_list:
            assert cls_tab[d] == 0 and not flags[d] & native.TOK_SPECIAL  # "##x" too: an appended ordinary token starts a word
        else:
            assert cls_tab[d] == base.cls_tab[d]  # an ordinary token the vocabulary holds keeps its class: "##x" goes on continuing
    assert "##x" in base_list and base.cls_tab[base_list.index("##x")] == 1 and "domain-term" not in base_list  # both branches are taken
    assert np.array_equal(cls_tab[:len(base_list)], base.cls_tab)  # (no special added token here is an ordinary base token)
    assert not np.isin(np.array([d for (c, s), d in zip(order, dense) if s]), voc.rand_ids).any()
    # the list survives load_resources and reset; clear_added_tokens gives the base back
    tok.load_resources(os.path.join(ref_dir, "resources", "tests" if "WP" in cls else "pretrained", "FastBPE" if "BPE" in cls else "FastWordPiece"))
    assert tok.added_tokens() == order and tok.vocab_list() == tokens
    tok.reset()
    assert tok.added_tokens() == order
    tok.clear_added_tokens()
    assert tok.added_tokens() == []
    tok = _tokenizer(swt, ref_dir, cls, "tests" if "WP" in cls else "pretrained")
    assert tok.vocab_list() == base_list and tok._batch_vocabulary().added_base is None


@pytest.mark.parametrize("cls", CLASSES)
def test_save_resources_does_not_see_added_tokens(swt, ref_dir, cls, tmp_path):
    """the files of save_resources are byte for byte what they are without added tokens, and nothing else is written"""
    tok = _tokenizer(swt, ref_dir, cls, "tests")
    tok.save_resources(str(tmp_path / "plain"))
    assert tok.add_special_tokens(["[MASK]", "<user>"]) == 2 and tok.add_tokens(["Domain-Term"]) == 1
    tok._batch_vocabulary()
    tok.save_resources(str(tmp_path / "added"))
    names = sorted(os.listdir(tmp_path / "plain"))
    assert names == sorted(os.listdir(tmp_path / "added")) == ["merges.json" if "BPE" in cls else "vocab.json"]
    for name in names:
        assert (tmp_path / "plain" / name).read_bytes() == (tmp_path / "added" / name).read_bytes()
    again = getattr(swt, cls)()
    again.load_resources(str(tmp_path / "added"))
    assert again.added_tokens() == []  # the caller re-adds


def test_a_vocabulary_that_holds_mask(swt):
    tok = swt.NaiveWP()
    tok.vocab = {"a", "[MASK]", "b", "##b", "[SEP]"}
    base = tok.vocab_list()
    assert tok.add_special_tokens(["[MASK]", "[SEP]", "<s>"]) == 3
    assert tok.mask_id() == base.index("[MASK]") and tok.vocab_list() == base + ["<s>"]
    assert tok._batch_vocabulary().added_dense.tolist() == [base.index("[MASK]"), base.index("[SEP]"), len(base)]


# ---- what is refused

@pytest.mark.parametrize("cls", CLASSES)
def test_add_tokens_refusals(swt, native, cls):
    tok = getattr(swt, cls)()
    bad = ["", "a b", "a\u00a0b", "a\u2003b", "\U0001F600", "x\U00010000", "q" * 65, "é" * 33, "a\tb"]
    for token in bad:
        want = A.refusal(token, 0, lambda ch: native.class_of(ord(ch)) & native.CLS_BERT_WS)
        assert want is not None
        with pytest.raises(ValueError) as err:
            tok.add_tokens(["fine", token])
        assert repr(token) in str(err.value)
        assert tok.added_tokens() == []  # nothing of a refused call is kept
    assert tok.add_tokens(["q" * 64, "é" * 32]) == 2
    with pytest.raises(TypeError):
        tok.add_tokens("a string")
    with pytest.raises(TypeError):
        tok.add_tokens([1])
    assert tok.add_tokens(["<%d>" % k for k in range(4094)]) == 4094
    with pytest.raises(ValueError) as err:
        tok.add_tokens(["one-more"])
    assert "'one-more'" in str(err.value) and "4096" in str(err.value)
    assert tok.add_tokens(["<7>"]) == 0 and len(tok.added_tokens()) == 4096


def test_fastwp_with_a_whitespace_token_refuses(swt):
    tok = swt.FastWP()
    tok.vocab = {"a", "a b", "##b"}
    tok._build_trie()
    with pytest.raises(ValueError):
        tok.add_tokens(["<user>"])
    tok = swt.FastWP()
    assert tok.add_tokens(["<user>"]) == 1  # before a vocabulary is there nothing can be said: the encode refuses
    tok.vocab = {"a", "a b", "##b"}
    tok._build_trie()
    with pytest.raises(ValueError):
        tok.encode_batch(["a <user>"])


def _create(native, patterns):
    blob = np.frombuffer(b"".join(patterns) + b"\0", dtype=np.uint8)
    off = np.zeros(len(patterns) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(p) for p in patterns])
    h = C.c_void_p()
    rc = native.lib().swt_added_create(native.ptr(blob, native.u8p), native.ptr(off, native.u64p), len(patterns), C.byref(h))
    if rc == 0:
        native.lib().swt_added_destroy(h)
    return rc


def test_create_refusals(native):
    """the limits of swt_added_create, which needs no device"""
    assert _create(native, [b"[mask]", "été€".encode(), b"q" * 64]) == 0
    assert _create(native, [b"<%04x>" % k for k in range(4096)]) == 0
    for patterns in ([], [b"<%04x>" % k for k in range(4097)], [b""], [b"q" * 65], [b"a", b"a"], [b"a b"], ["a\u00a0b".encode()],
                     ["a\u2003".encode()], [b"a\0"], ["\U0001F600".encode()], [b"\xed\xa0\x80"], [b"\xc3"], [b"\x80"], [b"\xc0\x80"],
                     [b"\xe0\x80\x80"], [b"a\xff"]):
        assert _create(native, patterns) == native.ERR_INVALID, patterns
        assert native.lib().swt_last_error()


# ---- the library's surface

def test_symbols_and_signatures(native, swt):
    lib = C.CDLL(native._build.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name) and name in native.SIGNATURES, name
    for name in METHODS:
        for cls in CLASSES:
            assert callable(getattr(getattr(swt, cls), name)), (cls, name)
    S, vp, u64 = native.SIGNATURES, C.c_void_p, C.c_uint64
    assert S["swt_added_create"] == (C.c_int, [native.u8p, native.u64p, C.c_uint32, native.vpp])
    assert S["swt_added_destroy"] == (None, [vp])
    assert S["swt_added_find"] == (C.c_int, [vp, native.u8p, native.u64p, u64, native.u8p, native.u64p, native.u32p, native.u32p, u64, native.u64p])
    assert S["swt_added_find_dev"] == (C.c_int, [vp, vp, u64, vp, u64, vp, vp, vp, vp, vp, vp])
    assert S["swt_added_splice"][1][4] is u64 and S["swt_added_splice"][1][8] is C.c_uint32 and len(S["swt_added_splice"][1]) == 13
    assert S["swt_added_splice_dev"][1][4] is u64 and S["swt_added_splice_dev"][1][8] is C.c_uint32 and len(S["swt_added_splice_dev"][1]) == 14
    step, halo, tile, n_max, len_max = native.added_capacity()
    assert step >= 128 and step % 64 == 0 and halo == len_max - 1 == 63 and tile >= step and n_max == 4096
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "swt.h"), encoding="utf-8") as f:
        header = f.read()
    for name in NAMES:
        assert name + "(" in header
