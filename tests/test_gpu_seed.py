"""The substring census of the device (swt_substring_counts) against the model of tests/seed_cases.py, entry for entry, and
UnigramWP.seed_substrings / train_unigram(seed="substrings") on top of it (MI355X).  Everything is integers: equality is exact."""
import json
import os
import random

import numpy as np
import pytest

from tests import seed_cases as S

pytestmark = pytest.mark.gpu
GIANT = [(S.letters(random.Random(9), 1124), 3), ("abcab", 2)]  # (the tile is 1,024: asserted below)
CASES = {  # name -> (words, max_chars, min_count, max_word, table_bits)
    **{"lengths L=%d" % L: (S.lengths(L), L, 1, 0, 0) for L in (2, 3, 16, 32)},
    "flag and overlap": ([("abab", 3), ("aaaa", 5), ("ab", 2), ("xyzab", 1), ("zab", 4)], 16, 1, 0, 0),
    "longer than a tile": (GIANT, 32, 1, 0, 0),
    "longer than max_word": (GIANT, 32, 1, 1024, 0),
    "colliding, library's table": (S.colliding(2000, "abc"), 16, 1, 0, 0),
    "colliding, 2^12 slots": (S.colliding(2000, "abc"), 16, 1, 0, 12),
    "chained probes, 2^12 slots": (S.colliding(700, "abcdef"), 16, 1, 0, 12),
    "one new key for the whole grid": (S.common_gram(), 16, 1, 0, 0),
    "wide counts": ([("xabc", 2 ** 32 - 1), ("abcy", 2 ** 32 - 1), ("zabcz", 2 ** 32 - 1)], 4, 1, 0, 0),
    "min_count": ([("ab", 4), ("cd", 5), ("cdx", 1), ("ef", 3), ("ef", 2)], 3, 5, 0, 0),
    "code points": ([("\U0001F600\U0001F601\U00020000", 2), ("!", 7), (",", 1), ("a\U0010FFFFb", 1), ("￿\U00010000", 3)], 16, 1, 0, 0),
    "no words": ([], 16, 1, 0, 0),
}


@pytest.fixture(scope="module")
def dev(native):
    if native.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests need an MI355X (there is no CPU fallback to test)")
    native.init(0)
    return native


def run(dev, words, max_chars, min_count=1, max_word=0, table_bits=0):
    return S.table(*dev.substring_counts(*S.pack(words), max_chars, min_count, max_word, table_bits))


@pytest.mark.parametrize("name", CASES)
def test_the_device_equals_the_model(dev, name):
    words, max_chars, min_count, max_word, bits = CASES[name]
    want = S.census(words, max_chars, min_count, max_word)
    assert run(dev, words, max_chars, min_count, max_word, bits) == want
    assert bool(want) == bool(words) and (not bits or 2 ** bits > len(S.census(words, max_chars)) > 2 ** bits // 20)
    if name == "longer than a tile":
        assert len(words[0][0]) > dev.substring_counts_capacity()[0]
    if name == "min_count":
        assert want == {(False, (99, 100)): 6, (False, (101, 102)): 5} and S.census(words, 3, 4)[(False, (97, 98))] == 4


@pytest.mark.parametrize("k", [-1, 0, 1, 2, 31, 32])
def test_tile_seams(dev, k):
    tile, halo, longest = dev.substring_counts_capacity()
    words = S.seam(tile, k)
    off = S.pack(words)[1].tolist()
    assert tile - k in off and 2 * tile - k not in off and off[-1] == 2 * tile + 40 and (halo, longest) == (31, 32)
    for max_chars in (5, longest):
        assert run(dev, words, max_chars) == S.census(words, max_chars)


def test_a_full_table_is_a_status(dev):
    words = S.colliding(40, "abc")
    assert len(S.census(words, 16)) > 16
    rc, _, _ = dev.substring_counts_into(*S.pack(words), 16, 1, 0, 4, None, None, None, None)
    assert rc == dev.ERR_NOMEM and b"full" in dev.lib().swt_last_error()
    with pytest.raises(dev.SwtError):
        dev.substring_counts(*S.pack(words), 16, 1, 0, 4)
    assert run(dev, words, 16) == S.census(words, 16)  # the process goes on, and the library's own table holds them all


def test_a_capacity_too_small_says_what_is_needed(dev):
    words = S.lengths(16)
    want, packed = S.census(words, 16), S.pack(words)
    n, m = len(want), sum(len(key[1]) for key in want)
    for out_cap, cps_cap in ((n - 1, m), (n, m - 1), (0, 0)):
        off, cps = np.full(n + 1, 77, dtype=np.uint64), np.full(m, 77, dtype=np.uint32)
        flag, count = np.full(n, 77, dtype=np.uint8), np.full(n, 77, dtype=np.uint64)
        got = dev.substring_counts_into(*packed, 16, 1, 0, 0, off, cps, flag, count, out_cap, cps_cap)
        assert got == (dev.ERR_CAPACITY, n, m)
        assert off[out_cap + 1:].tolist() == [77] * (n - out_cap) and flag[out_cap:].tolist() == count[out_cap:].tolist() == [77] * (n - out_cap)
        assert cps[cps_cap:].tolist() == [77] * (m - cps_cap)


def corpus(name):
    if name == "tutorial":
        return S.TUTORIAL
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref", "data", "train-5K.json")
    return json.load(open(path, encoding="utf-8"))[:300]


def word_list(tok, texts):
    return [(word, 1) for sentence in tok.preprocessing([t.lower() for t in texts]) for word, _ in sentence]


@pytest.mark.parametrize("name", ["tutorial", "train-5K"])
def test_seed_substrings_from_resident_text(swt, dev, name):
    tok, texts = swt.UnigramWP(), corpus(name)
    words = word_list(tok, texts)
    want = S.census(words, 16, 2, tok.max_word_chars)
    base = {ch for word, _ in words for ch in word}
    tokens, counts = tok.seed_substrings(texts, 10 ** 9, return_counts=True)
    assert counts == {S.token(key): v for key, v in want.items()} and len(want) > 20
    assert tokens == sorted(base | {"##" + ch for ch in base} | set(counts)) and not tok.vocab
    # a size in the middle of a tie: the order decides who is in
    size = 2 * len(base) + len(want) // 2
    ranked = [S.token(key) for key, _ in sorted(want.items(), key=S.seed_order)]
    assert tok.seed_substrings(texts, size) == sorted(base | {"##" + ch for ch in base} | set(ranked[:len(want) // 2]))
    assert tok.seed_substrings(texts, 3) == sorted(base | {"##" + ch for ch in base})


def test_train_unigram_from_substrings(swt, dev):
    tok = swt.UnigramWP()
    words = word_list(tok, S.TUTORIAL)
    always = 2 * len({ch for word, _ in words for ch in word})  # what prune always keeps: 'c' and '##c', and with them no word is orphaned
    pieces = {S.token(key) for key in S.census(words, 16, 2)}
    max_vocab = always + 6
    assert len(pieces) > 6
    rounds = tok.train_unigram(S.TUTORIAL, max_vocab, seed="substrings")
    assert rounds and rounds[0][0] == min(4 * max_vocab, always + len(pieces)) and always < len(tok.vocab) <= max_vocab
    assert {t for t in tok.vocab if not tok._mandatory(t)} <= pieces
    assert tok.removal_losses(S.TUTORIAL)["unk_words"] == 0
