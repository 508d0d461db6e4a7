"""The model of tests/viterbi_cases.py against a search over every segmentation and against MaxMatch; the refusals (no device)."""
import itertools
import random

import numpy as np
import pytest

from tests import viterbi_cases as V
from tests.test_naive_wp_encode import naivewp_cases


def exhaustive(vocab, score, word):
    """the best total in Python floats; on equal totals the longer last piece, then the longer one before it, and so on"""
    n, found = len(word), []
    for cuts in itertools.product((0, 1), repeat=n - 1):
        at = [0] + [k + 1 for k, c in enumerate(cuts) if c] + [n]
        pieces = [word[a:b] if a == 0 else "##" + word[a:b] for a, b in zip(at, at[1:])]
        if all(p in vocab for p in pieces):
            found.append((sum(score[p] for p in pieces), [b - a for a, b in zip(at, at[1:])][::-1], pieces))
    return max(found)[2] if found else ["[UNK]"]


@pytest.mark.parametrize("seed", range(6))
def test_the_model_finds_the_best_of_all_segmentations(seed):
    rng = random.Random(seed)
    pieces = {"".join(rng.choice("abż") for _ in range(rng.randint(1, 4))) for _ in range(30)} | {"a", "b"}
    vocab = sorted({p if rng.random() < 0.5 else "##" + p for p in pieces} | {"##a", "##ż"})
    score = V.dyadic(vocab, seed, span=3 + 10 * (seed % 2))  # few values: many ties
    model, words = V.Model(vocab, score), ["".join(rng.choice("abż") for _ in range(rng.randint(1, 12))) for _ in range(150)]
    want = [exhaustive(set(vocab), score, word) for word in words]
    assert [model.encode_word(word) for word in words] == want and 0 < want.count(["[UNK]"]) < 150


def test_equal_scores_give_the_fewest_pieces(swt):
    model = V.Model(V.HANDMADE, {t: -1.0 for t in V.HANDMADE})
    naive = swt.NaiveWP()
    naive.vocab = set(V.HANDMADE)
    assert naive.encode_word("abcde") == ["abc", "##d", "##e"] and model.encode_word("abcde") == ["ab", "##cde"]
    assert model.encode_word("abcd") == ["a", "##bcd"]  # three ways in two pieces: the longest last piece
    assert all(len(model.encode_word(w)) <= len(naive.encode_word(w)) for w in V.WORDS)


def test_rewarding_the_pieces_of_maxmatch(swt, golden):
    """Scores 0 for the tokens of the recorded NaiveWP rows and -64 for the rest, except the 334 tokens of the fixture, which
    stand a few 2^-8 above or below 0 so that where two segmentations into MaxMatch's pieces would tie (pod ##z, po ##dz) the
    recorded one totals more: the model then gives every one of the 989 recorded rows."""
    (vocab, texts, tokens), = [(v, t, k) for name, v, t, k in naivewp_cases() if name == "pan_tadeusz_pretrained"]
    fixture = golden("viterbi_maxmatch_scores.json")
    used = {t for row in tokens for t in row}
    assert len(tokens) == 989 and set(fixture["scores"]) <= used
    scores = {t: fixture["scores"].get(t, fixture["used_default"] if t in used else fixture["unused"]) for t in vocab}
    assert V.Model(vocab, scores).tokenize(swt.SubwordTokenizer._split, texts) == tokens


def test_unigram_wp_refuses(swt):
    tok = swt.UnigramWP()
    tok.vocab = {"a", "b", "##b"}
    with pytest.raises(ValueError, match="no scores"):
        tok.encode_ids_batch(["ab"])
    with pytest.raises(ValueError, match="'##b'"):
        tok.set_scores({"a": 0.0, "b": -1.0})
    for bad in (float("nan"), float("inf"), 1e39):
        with pytest.raises(ValueError, match="'b'"):
            tok.set_scores({"a": 0.0, "b": bad, "##b": 0.0})
    tok.set_scores({"a": 0.0, "b": -1.5, "##b": -0.25, "more": 3.0})
    assert tok.scores() == {"a": 0.0, "b": -1.5, "##b": -0.25}
    for kw in ({"dropout": {"probability": 0.1}}, {"maxmatch_dropout": {"probability": 0.1}}):
        for call in (tok.encode_ids_batch, tok.tokenize_batch, tok.encode_batch):
            with pytest.raises(ValueError, match="only"):
                call(["ab"], **kw)


def test_abi_checks_come_before_the_device(native):
    trie = native.WpTrie(["a", "b", "##b"])
    text, off = np.frombuffer(b"ab", dtype=np.uint8).copy(), np.array([0, 2], dtype=np.uint64)
    for entry in (lambda: trie.encode_viterbi(text, off), lambda: trie.encode_viterbi_joined(text, 1),
                  lambda: trie.encode_viterbi_dev(1, 2, 1, 1, 1, 1, 1, 1)):
        with pytest.raises(native.SwtError) as err:
            entry()
        assert err.value.code == native.ERR_STATE
    for scores in ([0.0, 0.0], [0.0, float("nan"), 0.0], [0.0, 0.0, float("-inf")]):
        with pytest.raises(native.SwtError) as err:
            trie.set_scores(scores)
        assert err.value.code == native.ERR_INVALID
    for value in (0, 1025):
        with pytest.raises(native.SwtError) as err:
            trie.set_option(native.OPT_MAX_WORD_CHARS, value)
        assert err.value.code == native.ERR_INVALID
    trie.set_scores([0.0, -1.0, -2.0])
