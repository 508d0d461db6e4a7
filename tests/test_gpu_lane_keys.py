"""The KEYS of the narrow FastBPE running-text kernel (csrc/swt_bpe_encode.hip: slot_key, scan_keys, KeyScan; csrc/swt_bpe_narrow.h)
against the C oracle, ids and offsets exact.

In the narrow kernel a val[] entry of a pair is the round's key itself, rank << 16 | the slot's index in its word: the split
writes the slot (counted across its 64-byte blocks), a round writes two entries with theirs, and a scan is a plain minimum over
two reads of two entries off one clamped base.  What can go wrong is what these tests aim at: a scan that reads past or before its
word (words of every group edge, a word without a pair beside one of a very low rank), a slot that is counted wrongly (words
across block boundaries and the chunk cut), equal ranks in one word (the leftmost one has to win), entries that are no keys
(FOREIGN symbols, dead slots), the tail of the rounds with few words, literal_rounds on the same entries (an improper table, words
beyond 32 symbols), and a table whose merged codes are not letters + rank (a merged string spelled twice: code_of_rank).

Every call asks for the narrow kernel at every size (SWT_OPT_LANE_NARROW = 2) and asserts that the launch took it
(swt_debug_bpe_table_info 11 == 1, through run() of tests/test_gpu_lane_narrow.py): a call that fell back to the wide kernel
would give the same arrays.  All texts are built from a fixed seed; nothing here reads a file outside the repository.  Needs a real
MI355X: `-m gpu`."""
import random

import pytest

from tests.test_gpu_lane_narrow import CAP, CONT, FOREIGN, dev, info, pre, run, tiled  # noqa: F401  (dev, pre: fixtures)
from tests.test_gpu_lane_spans import IMPROPER, fill, make, nbytes

pytestmark = pytest.mark.gpu

LENGTHS = (2, 3, 4, 5, 6, 8, 9, 12, 13, 16, 17, 31, 32, 33)  # group edges of the scan, length classes, the 32-slot mask and beyond


def words_of(cat, n, count, start=0, ascii_only=False):
    """`count` different words of exactly n symbols (letters) out of the corpus's own words; ascii_only: of n bytes too"""
    out, k = [], start
    while len(out) < count:
        w = cat[k:k + n]
        assert len(w) == n and w.isalpha()
        if not ascii_only or w.isascii():
            out.append(w)
        k += n
    return out


def test_word_lengths(dev, pre):
    """words of every length in LENGTHS: one as the only long word of its chunk, then so many in one chunk that lanes take second
    words -- 70 of them where 70 fit a chunk (up to 8 symbols), else as many as fit 400 bytes beside 60 short words"""
    tok, orc, short, multibyte, cat = pre
    rng = random.Random(0x10)
    two = [w for w in short if len(w) == 2][:40]
    assert len(two) >= 10
    for n in LENGTHS:
        for w in words_of(cat, n, 3, start=1000 + 37 * n):
            for lead in (0, 100):
                run(dev, tok, orc, tiled([fill(two, lead, rng) + w + " " + fill(two, 200, rng)]))
        many = words_of(cat, n, 70 if n <= 8 else 400 // (n + 1), start=5000, ascii_only=True)
        if n > 8:
            many = many + [rng.choice(two) for _ in range(60)]
        rng.shuffle(many)
        text = " ".join(many) + " "
        assert nbytes(text) <= CAP and len(many) >= 70  # one chunk (the text opens the call), more words than lanes
        run(dev, tok, orc, tiled([text]))
    # all lengths in one text of several chunks
    mixed = [w for n in LENGTHS for w in words_of(cat, n, 4, start=9000 + n)]
    run(dev, tok, orc, tiled([fill(mixed + two, 5 * CAP + 3, rng)]))


def test_neighbour_keys(dev, pre):
    """a word of two or three symbols that has no pair, directly beside (in the dense symbol array) a word whose first or last pair
    has a very low rank, in both orders; runs of punctuation marks, which are one-symbol words without a separator"""
    from subword_tokenizers_amd import synth

    tok, orc, short, multibyte, cat = pre
    merges = synth.pretrained_merges()[:8000]
    pairs = set(merges)
    letters = sorted({s for m in merges for s in m if len(s) == 1 and s.isalpha()})
    low = [l + r for l, r in merges[:40] if len(l) == 1 and len(r) == 1][:6]  # two letters, ranks below 40
    assert len(low) == 6
    rng = random.Random(0x20)
    none2 = [a + b for a in letters for b in letters if (a, b) not in pairs][:8]
    none3 = [ab + c for ab in none2 for c in letters if (ab[1], c) not in pairs][:8]
    assert len(none2) == 8 and len(none3) == 8
    sents = []
    for quiet in none2 + none3:
        for lw in low:
            # the low pair as the whole word, as its first pair and as its last pair
            for loud in (lw, lw + quiet[0] + quiet[0], quiet[-1] + quiet[-1] + lw):
                sents += [quiet + " " + loud, loud + " " + quiet, quiet + " " + loud + " " + quiet, loud + " " + quiet + " " + loud]
    for lw in low:
        sents += ["!!!!" + lw, lw + "!!!!", "!" + lw + "!" + lw + "!", "..." + none2[0] + "..." + lw, lw + "," + none3[0] + "," + lw + ".",
                  "!?" * 20 + lw, "(" + none2[1] + ")(" + lw + ")"]
    for k in range(0, len(sents), 40):
        run(dev, tok, orc, tiled(sents[k:k + 40]))          # few words per chunk: the tail's scan
        run(dev, tok, orc, tiled([" ".join(sents[k:k + 40]) + " "]))  # many: the rounds' scans
    # and none of the quiet words merged: a word of letters comes out as its letters
    ids, off = run(dev, tok, orc, tiled([none2[0] + " " + low[0] + " " + none3[0] + " " + low[0]]))
    ids = [int(x) for x in ids]
    assert ids[:2] == [ord(none2[0][0]), ord(none2[0][1]) | CONT] and ids[3:6] == [ord(none3[0][0]), ord(none3[0][1]) | CONT, ord(none3[0][2]) | CONT]


EQUAL = [("a", "a"), ("a", "b"), ("ab", "ab"), ("aa", "aa"), ("abab", "abab"), ("aaaa", "aaaa"), ("aaaa", "a"), ("b", "a")]


def test_equal_ranks_in_one_word(swt, oracle, dev):
    """one pair many times in a word, on a small proper table: the leftmost of equal ranks merges first, one occurrence a round"""
    tok, orc = make(swt, oracle, EQUAL)
    h = tok._table
    assert info(dev, h, 2) == 1 and info(dev, h, 8) == 1 and info(dev, h, 12) == 1 and info(dev, h, 7) == 1
    words = ["aaaa", "abababab", "aaaaaaaaa", "aaa", "aaaaa", "ababab", "aab", "baaab", "aa", "ab", "ba", "abab", "bababa", "aabaab",
             "a" * 31, "a" * 32, "a" * 33, "ab" * 15 + "a", "ab" * 16, "ab" * 17, "a" * 16, "a" * 17, "ba" * 6, "aaab" * 4,
             "aaca", "caaaa", "aaaac", "abcab", "aaéaa", "жabab", "abab😀"]
    rng = random.Random(0x30)
    run(dev, tok, orc, tiled(words))
    run(dev, tok, orc, tiled([" ".join(words) + " "]))
    for n in (CAP - 1, CAP + 1, 3000):
        run(dev, tok, orc, tiled([fill(words, n, rng)]))
    for w in words[:8]:
        run(dev, tok, orc, tiled([" ".join([w] * 75) + " "]))
    # what "leftmost first" means in tokens: aaa -> aa a (not a aa); aaaaa -> aa aa a -> aaaa a -> aaaaa
    ids, _ = run(dev, tok, orc, tiled(["aaa aaaaa"]))
    assert [int(x) for x in ids] == [tok._syms.intern("aa"), ord("a") | CONT, tok._syms.intern("aaaaa")]


def test_foreign_symbols(dev, pre):
    """a letter outside the alphabet at the first, a middle and the last slot of a word and next to the pair that merges: its
    entry is no key, never wins a minimum, and comes out as the code point"""
    tok, orc, short, multibyte, cat = pre
    rng = random.Random(0x40)
    for f in FOREIGN:
        words = []
        for n in (1, 2, 3, 4, 7, 8, 11, 12, 30, 31, 32):
            w = cat[2000 + 31 * n:2000 + 32 * n]
            words += [f + w, w + f, w[:n // 2] + f + w[n // 2:]]
        words += [f + "ie", "ie" + f, "n" + f + "ie", "ie" + f + "ie", f + f, f + "ie" + f, f + f + "ie" + f + f]
        ids, _ = run(dev, tok, orc, tiled(words))
        assert int(ids[0]) == ord(f)
        run(dev, tok, orc, tiled([" ".join(words) + " "]))
        run(dev, tok, orc, tiled([fill(words + short[:50], 3 * CAP + 1, rng)]))


def test_block_boundaries(dev, pre):
    """a word that begins 1, 2, ... bytes before a 64-byte block boundary of the split, and on it (bytes 62, 63 and 64 of the
    staged chunk among them): the slot index is carried from block to block; and a word across the chunk cut, in texts of CAP - 1,
    CAP and CAP + 1 bytes"""
    tok, orc, short, multibyte, cat = pre
    rng = random.Random(0x50)
    two = [w for w in short if len(w) == 2][:40]
    words = [cat[3000:3002], cat[3100:3105], cat[3200:3212], cat[3300:3331], cat[3400:3433], multibyte[0], multibyte[1] + cat[3500:3509]]
    for w in words:
        for edge in (64, 128, 576):
            for start in sorted({edge - 2, edge - 1, edge, edge + 1, edge - nbytes(w) + 1, edge - nbytes(w) // 2}):
                if start >= 0:
                    # the text opens the call (the 64 empty sentences in front of it hold no bytes): byte `start` of the staged chunk
                    run(dev, tok, orc, tiled([fill(two, start, rng) + w + " " + fill(two, 40, rng)]))
        # two block boundaries inside one word
        if nbytes(w) < 60:
            run(dev, tok, orc, tiled([fill(two, 60, rng) + w + w + w + " " + fill(two, 40, rng)]))
        for n in (CAP - 1, CAP, CAP + 1):
            for back in (1, 2, nbytes(w) - 1):
                run(dev, tok, orc, tiled([fill(short, n - back, rng) + w + " " + fill(short, 200, rng)]))
                run(dev, tok, orc, tiled([fill(short, n - nbytes(w) - 1, rng) + w + " "]))  # a text of n bytes that ends with the word


def test_few_words(dev, pre):
    """a chunk with at most 16 words of two symbols or more goes straight to the tail of the rounds (four lanes a word); one
    with 17 runs a round first"""
    tok, orc, short, multibyte, cat = pre
    rng = random.Random(0x60)
    for count in (1, 2, 4, 15, 16, 17, 18):
        for lengths in (LENGTHS[:-1], (2, 3), (31, 32), (9, 12, 13)):
            # words of one byte a symbol, so that every case fits one chunk (18 words of 32 bytes, 10 of one: 614 bytes) and runs
            ws = [words_of(cat, rng.choice(lengths), 1, start=4000 + 40 * k, ascii_only=True)[0] for k in range(count)]
            singles = [rng.choice("aiouwz") for _ in range(10)]  # one-symbol words are not in the list
            text = " ".join(ws[:count // 2] + singles + ws[count // 2:]) + " "
            assert nbytes(text) <= CAP and sum(len(w) >= 2 for w in text.split()) == count  # (the text opens the call)
            run(dev, tok, orc, tiled([text]))


def test_improper_table(swt, oracle, dev):
    """every word through literal_rounds on the keys; the table spells "ab" before the merge that produces it, so its merged codes are
    not letters + rank and come from code_of_rank"""
    tok, orc = make(swt, oracle, IMPROPER)
    h = tok._table
    assert info(dev, h, 2) == 0 and info(dev, h, 8) == 1 and info(dev, h, 12) == 0
    rng = random.Random(0x70)
    words = ["ab", "abc", "aaa", "aaaa", "cd", "xy", "abcabc", "bc", "aab", "xyxy", "żół", "żółżół", "óż", "łłł", "abc" * 11, "a" * 33,
             "abcd" * 8, "aab" * 11, "abéc", "жabc", "abc😀", "aaaaaaaaa", "abababab"]
    run(dev, tok, orc, tiled(words))
    for n in (CAP - 1, CAP + 1, 2500):
        run(dev, tok, orc, tiled([fill(words, n, rng)]))


REPEATED = [("b", "c"), ("a", "b"), ("a", "bc"), ("ab", "c"), ("abc", "d"), ("d", "d"), ("abcd", "dd")]


def test_repeated_merged_string(swt, oracle, dev):
    """("a", "bc") and ("ab", "c") both spell "abc": one symbol for two ranks, so the merged code of a rank is not letters + rank.
    The table is proper and stays eligible (info 8 and 7); its one-occurrence rounds and its tail read code_of_rank (info 12 == 0)"""
    tok, orc = make(swt, oracle, REPEATED)
    h = tok._table
    assert info(dev, h, 1) == 1 and info(dev, h, 2) == 1 and info(dev, h, 8) == 1 and info(dev, h, 7) == 1 and info(dev, h, 12) == 0
    assert info(dev, h, 9) == 4
    rng = random.Random(0x80)
    words = ["abc", "abcd", "abcabc", "aabc", "abcdabcd", "bcbc", "abab", "abcdd", "abcddd", "ddabcdd", "abd", "acb", "abcc", "dddd",
             "abcd" * 8, "abc" * 11, "abcdd" * 7, "ab", "bc", "dd", "ddd", "abécd", "жabcdd", "abcdd😀"]
    run(dev, tok, orc, tiled(words))                       # few words a chunk: the tail
    run(dev, tok, orc, tiled([" ".join(words * 4) + " "]))  # the rounds
    for n in (CAP - 1, CAP + 1, 2500):
        run(dev, tok, orc, tiled([fill(words, n, rng)]))
    ids, _ = run(dev, tok, orc, tiled(["abc abcddd"]))  # abc d d d -> abcd d d -> abcd dd -> abcddd
    assert [int(x) for x in ids] == [tok._syms.intern("abc"), tok._syms.intern("abcddd")]
