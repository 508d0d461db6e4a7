"""The project's own model of the substring census (include/swt.h, swt_substring_counts) in plain Python -- a Counter over
(i > 0, code points) with Python ints --, the order of UnigramWP.seed_substrings as one sort key, and the word lists of the tests."""
import random
from collections import Counter

import numpy as np

TUTORIAL = ["This is a sentence.", "Another example sentence."]  # the README's corpus


def census(words, max_chars, min_count=1, max_word=0):
    """words: [(str, frequency)] -> {(flag, code points): count} of the keys with count >= min_count"""
    count = Counter()
    for word, f in words:
        c = tuple(map(ord, word))
        for i in range(len(c) if not max_word or len(c) <= max_word else 0):
            for n in range(2, min(max_chars, len(c) - i) + 1):
                count[(i > 0, c[i:i + n])] += f
    return {key: v for key, v in count.items() if v >= min_count}


def token(key):
    return "##" * key[0] + "".join(map(chr, key[1]))


def seed_order(item):  # of a (key, count) pair: greater count x length, greater count, smaller token
    return -item[1] * len(item[0][1]), -item[1], token(item[0])


def pack(words):
    """-> sym uint32, word_off uint64[n + 1], freq uint32[n]"""
    off = np.zeros(len(words) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(w) for w, _ in words], dtype=np.uint64)
    sym = np.array([ord(ch) for w, _ in words for ch in w], dtype=np.uint32)
    return sym, off, np.array([f for _, f in words], dtype=np.uint32)


def table(off, cps, flag, count):
    """the entries of a call as the model's dict; a key that comes twice fails here"""
    keys = [(bool(flag[k]), tuple(cps[int(off[k]):int(off[k + 1])].tolist())) for k in range(len(flag))]
    assert int(off[0]) == 0 and len(set(keys)) == len(keys), "a key appears twice"
    return dict(zip(keys, map(int, count)))


def letters(rng, n, alphabet="abc"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def lengths(L):  # words of 1, 2, L, L + 1 and 3 L code points
    rng = random.Random(L)
    return [(letters(rng, n), f) for f, n in enumerate((1, 2, L, L + 1, 3 * L), 1)]


def seam(tile, k):
    """words of 7 letters, except that a word ends (and the next starts) exactly at tile - k and the middle of a word lies at
    2 * tile - k; the list runs 40 positions past the second seam"""
    rng, words, at = random.Random(k), [], 0
    for target in (tile - k, 2 * tile - k + 3, 2 * tile + 40):
        while at < target:
            n = 7 if target - at >= 14 else target - at
            words.append((letters(rng, n, "abcd"), 1 + len(words) % 3))
            at += n
    return words


def colliding(n, alphabet, seed=5):
    rng = random.Random(seed)
    return [("x" + letters(rng, 4, alphabet), 1) for _ in range(n)]


def common_gram(n=10000):  # unique words that all hold "qwert"
    return [("".join("abcdefghij"[int(d)] for d in "%04d" % i) + "qwert", 1) for i in range(n)]
