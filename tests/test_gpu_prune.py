"""UnigramWP's removal losses against the model of tests/prune_cases.py and against a real removal, and train_unigram (MI355X)."""
import json
import os

import numpy as np
import pytest

from tests import prune_cases as P
from tests.test_gpu_viterbi import CASES, SCORES, TEXTS, dev  # noqa: F401  (dev: the fixture)

pytestmark = pytest.mark.gpu
TOKENS = sorted(P.HANDMADE)


def make(swt, scores, max_word_chars=100, without=()):
    tok = swt.UnigramWP(max_word_chars=max_word_chars)
    tok.vocab = set(P.HANDMADE) - set(without)
    tok.set_scores(scores)
    return tok._ensure_scored_trie(), P.Prune(tok.vocab, scores, max_word_chars)


def by_device_pointers(trie, text, off):
    import torch
    d_text = torch.from_numpy(np.concatenate([text, np.zeros(64, dtype=np.uint8)])).cuda()
    d_off, out = torch.from_numpy(off.view(np.int64)).cuda(), torch.full((3 * trie.n_vocab + 3,), -1, dtype=torch.int64, device="cuda")
    trie.removal_losses_dev(d_text.data_ptr(), int(text.size), d_off.data_ptr(), int(off.size - 1), out[3:].data_ptr(), out.data_ptr())
    got = out.cpu().numpy()
    return got[3:].view(np.uint64).reshape(3, -1), got[:3]


@pytest.mark.parametrize("name,kind,max_word_chars", CASES)
def test_the_device_equals_the_model(swt, dev, name, kind, max_word_chars):
    trie, model = make(swt, SCORES[kind], max_word_chars)
    want, packed = model.batch(swt.SubwordTokenizer._split, TEXTS[name]), dev.pack_and_lower(TEXTS[name])
    for route, got in (("host", trie.removal_losses(*packed)), ("device", by_device_pointers(trie, *packed))):
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0]), (name, route)
    if name == "single workgroup" and max_word_chars == 100:  # words, UNK words, orphans, and with the log scores a loss
        assert want[1][0] and want[1][1] and want[0][2].any() and (kind != "log" or want[0][1].any())


@pytest.mark.parametrize("n_sent", [1, 300])
def test_colliding_adds_lose_nothing(swt, dev, n_sent):
    trie, model = make(swt, SCORES["log"])
    per, (total, path, loss) = 20000 // n_sent, model.word("abcde")
    texts = [" ".join(["abcde"] * per)] * (n_sent - 1) + [" ".join(["abcde"] * (20000 - per * (n_sent - 1)))]
    want = np.zeros((3, len(TOKENS)), dtype=np.uint64)
    for t in path:
        want[0, model.ids[t]] += np.uint64(20000)
    for t, u in loss.items():
        want[2 if u is None else 1, model.ids[t]] = 20000 * (1 if u is None else u)
    got = trie.removal_losses(*dev.pack_and_lower(texts))
    assert np.array_equal(got[0], want) and got[1].tolist() == [20000, 0, 20000 * total]


def test_a_loss_is_what_the_removal_costs(swt, dev):
    packed = dev.pack_and_lower(TEXTS["tiles"] + TEXTS["single workgroup"])
    (counts, loss, orphaned), (words, unk, total) = make(swt, SCORES["dyadic"])[0].removal_losses(*packed)
    assert loss.any() and orphaned.any() and (counts[orphaned == 0] > 0).sum() >= 5
    for k in np.nonzero(counts)[0]:
        after = make(swt, SCORES["dyadic"], without=[TOKENS[k]])[0].removal_losses(*packed)[1]
        assert after[0] + after[1] == words + unk and after[1] == unk + int(orphaned[k]), TOKENS[k]
        if not orphaned[k]:
            assert after[2] == total - int(loss[k]), TOKENS[k]  # exactly: with these scores every float32 sum is exact


class Logged:  # (mixed into UnigramWP below) every prune with the vocabulary it met and the figures it was given
    def prune(self, corpus, max_vocab, losses=None):
        before = sorted(self.vocab)
        removed = super().prune(corpus, max_vocab, losses)
        self.log.append((before, losses, removed, max_vocab))
        return removed


def test_train_unigram(swt, dev):
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref", "data", "pan_tadeusz.json")
    corpus = json.load(open(path, encoding="utf-8"))[:300]
    tok = type("LoggedUnigramWP", (Logged, swt.UnigramWP), {"log": []})()
    rounds = tok.train_unigram(corpus, 300)
    seed = tok.log[0][0]
    assert len(seed) > 900 and len(rounds) == len(tok.log) >= 4 and [r[0] for r in rounds] == [len(b) for b, _, _, _ in tok.log]
    assert {t for t in seed if tok._mandatory(t)} <= tok.vocab == set(tok.scores()) and len(tok.vocab) <= 300  # (some 150 are mandatory)
    assert all(a[2] >= b[2] for a, b in zip(rounds, rounds[1:])) and tok.removal_losses(corpus)["unk_words"] <= rounds[-1][2]
    for before, losses, removed, target in tok.log:
        free = [(t in removed, x) for t, x, o in zip(before, losses["loss"], losses["orphaned"]) if not tok._mandatory(t) and not o]
        assert removed and len(before) - len(removed) >= target
        assert max(x for g, x in free if g) <= min([x for g, x in free if not g], default=np.inf)
