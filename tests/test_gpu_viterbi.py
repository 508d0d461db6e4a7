"""UnigramWP on the device against the model of tests/viterbi_cases.py, element by element, at every seam of the skeleton (MI355X)."""
import math
import random

import numpy as np
import pytest

from tests import batch_cases as B
from tests import viterbi_cases as V
from tests.maxmatch_cases import fill
from tests.test_gpu_wp_seams import CAP, DIRECT_BYTES, DIRECT_SENTS, TILE, dev  # noqa: F401  (dev: the fixture)

pytestmark = pytest.mark.gpu
SCORES = {"dyadic": V.dyadic(V.HANDMADE, 5), "equal": {t: -1.0 for t in V.HANDMADE}, 
          "log": dict(zip(sorted(V.HANDMADE), np.log(np.random.RandomState(6).dirichlet(np.ones(len(V.HANDMADE)))).tolist()))}


def make(swt, scores, max_word_chars=100):
    tok = swt.UnigramWP(max_word_chars=max_word_chars)
    tok.vocab = set(V.HANDMADE)
    tok.set_scores(scores)
    return tok, V.Model(V.HANDMADE, scores, max_word_chars)


def exact(n, seed, tail="", words=V.WORDS):
    t = fill(n - len(tail.encode()), random.Random(seed), words) + tail
    assert len(t.encode()) == n
    return t


def spread(total, n_sent, seed):
    per = total // n_sent
    return [exact(per, seed + k, words=V.WORDS[:17]) for k in range(n_sent - 1)] + [exact(total - per * (n_sent - 1), seed - 1, words=V.WORDS[:17])]


TEXTS = {
    "single workgroup": ["", ""] + [" ".join(V.WORDS[:18]), "", "xq abcd q,abcde", "x" * 100, "x" * 101 + " ab", "ab" + "x" * 98 + " abc" + "x" * 98] + ["", ""]
    + ["żół €€ż \U0001F600\U0001F600a 中中ż abcd"] * 3 + [""],
    "tiles": [""] + [exact(90, k) for k in range(40)] + ["", ""] + [exact(30, 100 + k) for k in range(60)] + ["", ""],
    "words on and across the tile seam": [exact(TILE, 1, " abcde"), exact(TILE - 3, 2, "żół"), "abx", exact(2 * TILE, 3, "abcd")] * 3,
    "a word ends on the chunk seam": [exact(CAP, 4, " abcde"), "abcd", exact(CAP - 5, 5, "€€ż"), "abcde", exact(40, 6)] * 2,
    "a sentence longer than a chunk, single workgroup": ["ab", "", exact(CAP + 300, 7, "abcde żół abcd"), "", "abcd"],
    "a sentence longer than a chunk, among tiles": [exact(60, 8)] * 30 + ["", exact(DIRECT_BYTES + 500, 9, " abcde " + "x" * 100 + " 中中ż"), ""] + [exact(70, 10)] * 20,
    "host: 2,048 bytes in 64 sentences": spread(DIRECT_BYTES, DIRECT_SENTS, 20),
    "host: 2,049 bytes": spread(DIRECT_BYTES + 1, DIRECT_SENTS, 21),
    "host: 65 sentences": spread(1000, DIRECT_SENTS + 1, 22),
    "host: 64 KiB in 4,096 sentences": spread(65536, 4096, 23),
    "host: 64 KiB and a byte": spread(65537, 700, 24),
    "host: 4,097 sentences": spread(4097 * 6, 4097, 25),
}


CASES = [(name, kind, chars) for name in TEXTS for kind, chars in [("dyadic", 100), ("log", 100), ("equal", 100), ("dyadic", 4), ("log", 4)]
         if not name.startswith("host") or (kind, chars) == ("dyadic", 100)]


@pytest.mark.parametrize("name,kind,max_word_chars", CASES)
def test_the_device_equals_the_model(swt, dev, name, kind, max_word_chars):
    tok, model = make(swt, SCORES[kind], max_word_chars)
    texts = TEXTS[name]
    assert (len(texts) <= DIRECT_SENTS and sum(len(t.encode()) for t in texts) <= DIRECT_BYTES) == ("single workgroup" in name or name.startswith("host: 2,048"))
    got = tok._ensure_scored_trie().encode_viterbi(*dev.pack_and_lower(texts))
    want = model.batch(swt.SubwordTokenizer._split, texts)
    assert np.array_equal(got[2], want[2]) and np.array_equal(np.asarray(got[1], dtype=np.uint64), want[1]), name
    assert np.array_equal(got[0], want[0]), name
    if name == "single workgroup" and max_word_chars == 100:
        assert tok.tokenize("abcde") == model.encode_word("abcde") != swt.NaiveWP.encode_word(tok, "abcde")
        assert model.unk in want[0] and tok.tokenize_batch(texts) == model.tokenize(swt.SubwordTokenizer._split, texts)
        tok.max_word_chars = 4  # changed after the scores went to the trie: it still reaches the next call
        assert tok.tokenize("abcde abcd") == ["[UNK]"] + model.encode_word("abcd")


def test_encode_batch_on_the_device(swt, dev):
    tok, model = make(swt, SCORES["log"])
    texts, split = TEXTS["single workgroup"], swt.SubwordTokenizer._split
    rows, spans, word = [], [], []
    for text in texts:
        rows.append([]), spans.append([]), word.append([])
        for w, (piece_word, (start, end)) in enumerate(split(text.lower())):
            at = start
            for t in model.encode_word(piece_word):
                width = end - start if t == "[UNK]" else len(t) - 2 * (at > start)
                rows[-1].append(model.ids_of([t])[0]), spans[-1].append((at, at + width)), word[-1].append(w)
                at += width
    voc, sp = tok._batch_vocabulary(), tok.special_ids()
    s = B.spec(12, pad_id=sp["pad"], unk_id=sp["unk"], cls_id=sp["cls"], sep_id=sp["sep"])
    want = B.expected_batch(rows, s, (voc.cmap, voc.n_map, voc.flagged), (spans, word))
    got = tok.encode_batch(texts, max_length=12, padding="max_length", return_offsets=True, device=True)
    for k in ("input_ids", "attention_mask", "offset_mapping", "word_ids"):
        assert np.array_equal(got[k].cpu().numpy(), want[k]), k


def test_fit_scores(swt, dev):
    corpus = TEXTS["tiles"][:50] + ["abcde abcd abcde"] * 5
    tok, _ = make(swt, SCORES["equal"])  # (the scores it starts with do not matter: iteration 0 is MaxMatch)
    totals = tok.fit_scores(corpus, iterations=3, alpha=0.5)
    naive, split, want, scores = swt.NaiveWP(), swt.SubwordTokenizer._split, [], None
    naive.vocab = set(V.HANDMADE)
    for it in range(3):
        rows = [naive.tokenize(t) for t in corpus] if it == 0 else V.Model(V.HANDMADE, scores).tokenize(split, corpus)
        count = {t: sum(r.count(t) for r in rows) for t in V.HANDMADE}
        norm = sum(count.values()) + 0.5 * len(V.HANDMADE)
        scores = {t: float(np.float32(math.log((c + 0.5) / norm))) for t, c in count.items()}
        want.append(sum(len(r) for r in rows))
    assert totals == want and tok.scores() == scores
