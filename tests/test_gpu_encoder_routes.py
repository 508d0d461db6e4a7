"""The route of encode_ids_batch is one decision for the four classes: past 64 texts the joined call, unless a text holds U+0000
or the device leaves a text's lowercase to str.lower(); otherwise pack_and_lower and the host call.  Whatever the route, a text
gets the ids it gets alone.  The tables are the hand-made ones of tests/test_gpu_host_paths.py (NaiveBPE's is not
order-equivalent, so its list order shows), the WordPiece vocabulary with the three tokens more that spell the two special texts
below (FastWP refuses a sentence with a letter it has no edge for); the texts are a few of that file's words each.  Needs a real
MI355X: `-m gpu`."""
import random

import numpy as np
import pytest

from tests.test_gpu_host_paths import KINDS, NOT_ORDER_EQUIVALENT, PROPER, WORDS, dev, handmade_vocab  # noqa: F401  (dev: a fixture)

pytestmark = pytest.mark.gpu

N_TEXTS = 70  # the smallest batch past the 64-text threshold that leaves room for the variants
WITH_NUL = "ab \0 cd"  # U+0000 as a word of its own: join_texts counts it and the joined call is not tried
HOST_LOWER = "İ abab"  # U+0130 lowercases to two code points: the device flags the text, the joined call returns None
SPELLED = {"\0", "i", "##\u0307"}  # what the vocabulary needs for the two


def texts_of(kind):
    rng = random.Random(KINDS.index(kind) + 1)
    return [""] + [" ".join(rng.choice(WORDS) for _ in range(rng.randint(1, 4))) for _ in range(N_TEXTS - 1)]


class Tokenizer:
    """one of the four over its hand-made table: the tokenizer, its handle and the handle's joined call"""

    def __init__(self, kind, swt):
        self.kind, self.status = kind, kind.endswith("wp")
        if kind == "fast_bpe":
            self.tok = swt.FastBPE()
            self.tok.merges_list = list(PROPER)
            self.tok._build_table()
            self.joined = self.tok._table.encode_joined
        elif kind == "naive_bpe":
            self.tok = swt.NaiveBPE()
            self.tok.merges_list = list(NOT_ORDER_EQUIVALENT)
            self.joined = self.tok._ensure_naive_table().encode_naive_joined
        elif kind == "fast_wp":
            self.tok = swt.FastWP()
            self.tok.vocab = set(handmade_vocab()) | SPELLED
            self.tok._build_trie()
            self.joined = self.tok._trie.encode_joined
        else:
            self.tok = swt.NaiveWP()
            self.tok.vocab = set(handmade_vocab()) | SPELLED
            self.joined = self.tok._ensure_naive_trie().encode_naive_joined


@pytest.fixture(scope="module", params=KINDS)
def enc(request, swt, dev):  # noqa: F811
    return Tokenizer(request.param, swt)


def forms(kind):
    """name -> texts: the four forms of one batch"""
    texts = texts_of(kind)
    return {"joined": texts, "packed": texts[:64], "nul": texts[:30] + [WITH_NUL] + texts[30:],
            "host lowercase": texts[:50] + [HOST_LOWER] + texts[50:]}


def test_every_route_gives_a_text_the_ids_it_gets_alone(dev, enc):  # noqa: F811
    tok, alone = enc.tok, {}
    for name, texts in forms(enc.kind).items():
        got = tok.encode_ids_batch(texts)
        ids, off = got[0], got[1]
        assert off.size == len(texts) + 1 and int(off[-1]) == ids.size, name
        if enc.status:
            assert got[2].size == len(texts) and not got[2].any(), name
        for i, t in enumerate(texts):
            if t not in alone:
                alone[t] = tok.encode_ids_batch([t])[0].tolist()
            assert ids[int(off[i]):int(off[i + 1])].tolist() == alone[t], (name, i, t)
        assert tok.tokenize_batch(texts) == [tok.tokenize(t) for t in texts], name  # (the Naive classes: their Python loop)
    assert alone[WITH_NUL] and alone[HOST_LOWER] and alone[""] == []


def test_the_long_way_is_taken(dev, enc):  # noqa: F811
    """the joined call answers for the plain batch and returns None for the text only str.lower() lowercases"""
    joined_call, f = enc.joined, forms(enc.kind)
    joined, n_nul = dev.join_texts(f["joined"])
    assert n_nul == 0 and dev.device_lower_ok()
    got = joined_call(joined, N_TEXTS)
    want = enc.tok.encode_ids_batch(f["joined"])
    assert got is not None and all(np.array_equal(a, b) for a, b in zip(got, want))
    joined, n_nul = dev.join_texts(f["host lowercase"])
    assert n_nul == 0 and joined_call(joined, N_TEXTS + 1) is None
    assert dev.join_texts(f["nul"])[1] == 1


def test_spans_by_tiling_agree_with_the_ids(dev, enc):  # noqa: F811
    if enc.kind == "fast_wp":
        return  # its spans come from the trie walk (fast_encode_spans_batch, tests/test_gpu_fastwp_spans.py)
    tok = enc.tok
    texts = texts_of(enc.kind) + [WITH_NUL, HOST_LOWER]
    want = tok.encode_ids_batch(texts)
    got = tok.encode_spans_batch(texts)
    assert len(got) == len(want) + 2
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    ids, off, spans, word = got[0], got[1], got[-2], got[-1]
    assert spans.shape == (ids.size, 2) and word.shape == (ids.size,)
    toks = tok.decode_ids(ids) if enc.kind.endswith("bpe") else [(tok._naive_tokens + ["['UNK']", "[UNK]"])[i] for i in ids.tolist()]
    n_unk = 0
    for i, t in enumerate(texts):
        low = t.lower()
        for k in range(int(off[i]), int(off[i + 1])):
            piece = low[int(spans[k, 0]):int(spans[k, 1])]
            if toks[k] == "[UNK]":  # it stands for its whole word
                n_unk += 1
                assert piece and not any(c.isspace() for c in piece), (i, k)
            else:
                assert piece == (toks[k][2:] if toks[k].startswith("##") else toks[k]), (i, k, toks[k], piece)
    assert (n_unk > 0) == (enc.kind == "naive_wp")
