"""UnigramWP's expected counts on the device against the model of tests/marginal_cases.py: every count and every stat, at every seam
of the skeleton and by both routes (MI355X)."""
import math

import numpy as np
import pytest

from tests import marginal_cases as M
from tests import viterbi_cases as V
from tests.test_gpu_sample import CASES, LOG, WEIGHTS
from tests.test_gpu_viterbi import TEXTS, dev  # noqa: F401  (dev: the fixture)

pytestmark = pytest.mark.gpu
TOKENS = sorted(M.HANDMADE)


def make(swt, kind, max_word_chars=100):  # -> (the tokenizer, its trie under the weights as given, the model)
    tok = swt.UnigramWP(max_word_chars=max_word_chars)
    tok.vocab = set(M.HANDMADE)
    tok.set_scores(LOG)
    trie = tok._ensure_scored_trie()
    trie.set_weights([WEIGHTS[kind][t] for t in TOKENS])
    return tok, trie, M.Marginal(M.HANDMADE, WEIGHTS[kind], max_word_chars)


def by_device_pointers(trie, text, off):
    import torch
    d_text = torch.from_numpy(np.concatenate([text, np.zeros(64, dtype=np.uint8)])).cuda()
    d_off, out = torch.from_numpy(off.view(np.int64)).cuda(), torch.full((trie.n_vocab + 3,), -1, dtype=torch.int64, device="cuda")
    trie.expected_counts_dev(d_text.data_ptr(), int(text.size), d_off.data_ptr(), int(off.size - 1), out[3:].data_ptr(), out.data_ptr())
    got = out.cpu().numpy()
    return got[3:].view(np.uint64), got[:3]


def same(got, want, what):
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0]), what


@pytest.mark.parametrize("name,kind,max_word_chars", CASES)
def test_the_device_equals_the_model(swt, dev, name, kind, max_word_chars):
    _, trie, model = make(swt, kind, max_word_chars)
    want, packed = model.batch(swt.SubwordTokenizer._split, TEXTS[name]), dev.pack_and_lower(TEXTS[name])
    same(trie.expected_counts(*packed), want, name + ", host pointers")
    same(by_device_pointers(trie, *packed), want, name + ", device pointers")
    if name == "single workgroup" and max_word_chars == 100:  # words, UNK words, and at 2^-64 a likelihood that float32 cannot hold
        assert want[1][0] and want[1][1] and (kind != "2^-64" or want[1][2] < -6400 << 24)


@pytest.mark.parametrize("n_sent", [1, 300])
def test_colliding_adds_lose_nothing(swt, dev, n_sent):
    _, trie, model = make(swt, "log at 1")
    per, (pieces, like) = 20000 // n_sent, model.expected("abcde")
    texts = [" ".join(["abcde"] * per)] * (n_sent - 1) + [" ".join(["abcde"] * (20000 - per * (n_sent - 1)))]
    want = np.zeros(len(TOKENS), dtype=np.uint64)
    for k, q in pieces:
        want[k] += np.uint64(20000 * q)
    same(trie.expected_counts(*dev.pack_and_lower(texts)), (want, [20000, 0, 20000 * like]), n_sent)


def m_step(counts, alpha):
    c = counts.astype(np.float64) * 2.0 ** -32
    return {t: float(np.float32(math.log((float(x) + alpha) / (float(c.sum()) + alpha * len(TOKENS))))) for t, x in zip(TOKENS, c)}


def test_expected_counts_and_soft_fit(swt, dev):
    corpus, split = TEXTS["tiles"][:50] + ["abcde abcd abcde xq"] * 5, swt.SubwordTokenizer._split
    tok, _, _ = make(swt, "alpha 0")  # (the weights its trie was left with do not matter: the layer makes its own, at alpha 1)
    counts, stats = M.Marginal(M.HANDMADE, M.weights(LOG, 1.0)).batch(split, corpus)
    got = tok.expected_counts(corpus)
    assert np.array_equal(got["counts"], counts.astype(np.float64) * 2.0 ** -32) and got["counts"].dtype == np.float64
    assert (got["words"], got["unk_words"], got["log2_likelihood"]) == (stats[0], stats[1], stats[2] * 2.0 ** -24) and stats[1] >= 5
    assert np.array_equal(tok.expected_counts(corpus, device=True).pop("counts").cpu().numpy().view(np.uint64), counts)
    scores, want = {t: float(np.float32(s)) for t, s in LOG.items()}, []
    for _ in range(2):
        counts, stats = M.Marginal(M.HANDMADE, M.weights(scores, 1.0)).batch(split, corpus)
        scores = m_step(counts, 0.5)
        want.append(stats[2] * 2.0 ** -24)
    assert tok.fit_scores(corpus, iterations=2, alpha=0.5, method="soft") == want and tok.scores() == scores


def test_hard_stays_the_default_and_what_is_refused(swt, dev):
    corpus, split = TEXTS["tiles"][:50] + ["abcde abcd abcde"] * 5, swt.SubwordTokenizer._split
    tok, naive = swt.UnigramWP(), swt.NaiveWP()
    tok.vocab = naive.vocab = set(M.HANDMADE)
    with pytest.raises(ValueError):
        tok.expected_counts(corpus)  # (no scores yet)
    with pytest.raises(ValueError):
        tok.fit_scores(corpus, method="medium")
    totals, want, scores = tok.fit_scores(corpus, alpha=0.5), [], None
    for it in range(2):
        rows = [naive.tokenize(t) for t in corpus] if it == 0 else V.Model(M.HANDMADE, scores).tokenize(split, corpus)
        count = {t: sum(r.count(t) for r in rows) for t in TOKENS}
        scores = {t: float(np.float32(math.log((c + 0.5) / (sum(count.values()) + 0.5 * len(TOKENS))))) for t, c in count.items()}
        want.append(sum(len(r) for r in rows))
    assert totals == want and all(type(t) is int for t in totals) and tok.scores() == scores
    soft = tok.fit_scores(corpus, iterations=1, method="soft")  # (seeded by the scores it has: no MaxMatch step)
    assert soft == [M.Marginal(M.HANDMADE, M.weights(scores, 1.0)).batch(split, corpus)[1][2] * 2.0 ** -24]
