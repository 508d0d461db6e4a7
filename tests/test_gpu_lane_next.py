"""The split's next symbol from LDS, the word list, and the rounds' minimum scan and lookup of the FastBPE running-text kernel
(csrc/swt_bpe_encode.hip: lane_split, lane_words_count / lane_words_write, KeyWalk / walk_keys, slot_value) against the C oracle,
ids and sentence offsets exact.

The split of the narrow kernels with rounds proper stores a block's symbols and reads a symbol's successor back from sym[si + 1]
(every other kernel fetches it from its lane).  What can go wrong there is a successor
that is not in the block (the pair of lane 63 and the next block's first symbol, the last symbol of a chunk), one that is there but
does not continue the word (a word start, a sentence start between two letters), and a symbol that is not a code (FOREIGN).  The
rounds scan a word's keys in trips of four entries, of which only the last is clamped: every word length from 2 to 33 symbols has
its own pattern of trips, and words of 2 and 3 symbols must not read their neighbour's entries.  The word list orders the words
of a chunk by length class; the cases put 0 .. 129 words of a class into one chunk, alone and interleaved.

Every case runs through the narrow kernel and the wide one (tests.test_gpu_lane_diet.both) and, with the same texts, over a proper
unpacked table (every); the list cases also through NaiveBPE's list order and BPE-dropout at drop_below = 0, which must spell
FastBPE's words.  Texts are built from fixed
seeds; nothing here reads a file outside the repository.  Needs a real MI355X: `-m gpu`."""
import random

import numpy as np
import pytest

from tests import dropout_cases as D
from tests.test_gpu_dropout import Case, same
from tests.test_gpu_lane_diet import both
from tests.test_gpu_lane_narrow import CAP, FOREIGN, dev, info, pre, run, synthetic, tiled  # noqa: F401  (dev, pre: fixtures)
from tests.test_gpu_lane_spans import IMPROPER, fill, make, nbytes

pytestmark = pytest.mark.gpu

ALPHABET = [chr(ord("a") + i) for i in range(26)] + list("ąćęłńóśźżαβγδε")


@pytest.fixture(scope="module")
def unpacked(swt, oracle, dev):
    """the one table of more than 65,536 merges: proper and not packed, so every call takes the wide kernel on wide values"""
    tok, orc = make(swt, oracle, synthetic(65600, ALPHABET))
    assert info(dev, tok._table, 1) == 0 and info(dev, tok._table, 2) == 1 and info(dev, tok._table, 8) == 0
    return tok, orc


def lead(n, rng, words=("ie", "na", "po", "do")):
    """n bytes exactly that end with a space (n = 0: nothing), so that what follows starts a word at byte n of its sentence"""
    out = fill(list(words), n, rng) if n > 0 else ""
    assert nbytes(out) == n
    return out


def every(dev, tok, orc, unpacked, texts):
    """the narrow kernel, the wide one on the packed table, and the same texts on the proper unpacked table (a letter outside
    its alphabet is a symbol of its own there too: the oracle of that table says what comes out)"""
    out = both(dev, tok, orc, texts)
    run(dev, unpacked[0], unpacked[1], texts, narrow=0)
    return out


def test_word_across_a_block_boundary(dev, pre, unpacked):
    """a word of four symbols and more that starts at bytes 60 .. 66 of a block's neighbourhood: its symbols sit in lanes 62, 63,
    0 and 1 of two blocks; with a character of two, three and four bytes as the last symbol of the block and as the first of the
    next (the longer ones are FOREIGN to the table)"""
    tok, orc, short, multibyte, cat = pre
    utok, uorc = unpacked
    rng = random.Random(0x4E01)
    for edge in (64, 576):
        texts, utexts = [], []
        for start in range(edge - 4, edge + 3):
            for w in (cat[3000:3004], "nie", cat[3100:3107]):
                texts.append(lead(start, rng) + w + " " + lead(40, rng))
            for w in ("abcd", "αβγ", "abcabca"):
                utexts.append(lead(start, rng, ("ab", "ca", "bd")) + w + " " + lead(40, rng, ("ab", "ca")))
            for ch in ("ą", "é", "€", "😀"):
                k = nbytes(ch)
                if start + 2 + k <= edge + 4:
                    # "ni" + ch + "e": ch ends the block when start + 2 + k == edge, opens the next when start + 2 == edge
                    texts.append(lead(start, rng) + "ni" + ch + "e nie")
                    texts.append(lead(start, rng) + ch + "nie" + ch + " " + ch)
        for t in texts:
            every(dev, tok, orc, unpacked, tiled([t]))
        for t in utexts:
            run(dev, utok, uorc, tiled([t]), narrow=0)


def test_empty_blocks_and_a_word_that_ends_on_byte_63(dev, pre, unpacked):
    """a block of whitespace only between two words (no symbol: nothing is stored, nothing read back), and a word whose last
    symbol is lane 63 with a space, a letter of another sentence, or nothing behind it"""
    tok, orc, short, multibyte, cat = pre
    rng = random.Random(0x4E02)
    for w in ("nie", cat[3000:3006], "niż"):
        head = lead(64 - nbytes(w), rng) + w
        assert nbytes(head) == 64
        every(dev, tok, orc, unpacked, tiled([head + " " + "nie", head + " " * 64 + "nie", head + " " * 130 + w, head]))
        every(dev, tok, orc, unpacked, [""] * 63 + [head, "ie nie", lead(CAP, rng)])
    every(dev, tok, orc, unpacked, tiled(["nie" + " " * 61 + " " * 64 + "ie" + " " * 62 + "nie"]))


def test_foreign_neighbours(dev, pre, unpacked):
    """a code point outside the alphabet as the left and as the right neighbour of a pair, as the last symbol of a block, as the
    first symbol of a word and of a block: its entry is its code point and no lookup reads it as a code"""
    tok, orc, short, multibyte, cat = pre
    rng = random.Random(0x4E03)
    for f in FOREIGN:
        k = nbytes(f)
        words = [f + "nie", "ni" + f + "e", "nie" + f, "n" + f + f + "ie", f + "ie" + f]
        for w in words:
            texts = [lead(start, rng) + w + " nie" for start in range(64 - nbytes(w) - 1, 66) if start >= 0]
            every(dev, tok, orc, unpacked, tiled(texts))
        # the last symbol of the block, the pair behind it straddling (not looked up); then the first symbol of the next block
        every(dev, tok, orc, unpacked, tiled([lead(64 - k - 1, rng) + "n" + f + "ie nie", lead(63, rng) + "n" + f + "ie", lead(64, rng) + f + "ie"]))


def test_last_symbol_of_a_chunk(dev, pre, unpacked):
    """the chunk boundary swept over bytes 636 .. 644 inside a word: the cut sends the word to the next chunk, and the last symbol
    the chunk keeps has no successor there"""
    tok, orc, short, multibyte, cat = pre
    rng = random.Random(0x4E04)
    for n in range(CAP - 4, CAP + 5):
        for w in ("nie", cat[3200:3212], "niż", "n" + FOREIGN[1] + "ie"):
            for back in (1, 2, nbytes(w) - 1):
                every(dev, tok, orc, unpacked, tiled([lead(n - back, rng) + w + " " + lead(200, rng)]))
        every(dev, tok, orc, unpacked, tiled([lead(n, rng) + "nie"]))


def test_sentence_starts_between_letters(dev, pre, unpacked):
    """sentence starts with no whitespace in front: between two letters of what would be one word (the pair must not merge), empty
    sentences on the same byte, and the same on a block boundary"""
    tok, orc, short, multibyte, cat = pre
    rng = random.Random(0x4E05)
    for at in (10, 62, 63, 64, 65, 130):
        head = lead(at - 2, rng) + "ni"
        ids, off = every(dev, tok, orc, unpacked, [""] * 30 + [head, "", "", "e", "ie", "", "nie" + cat[3000:3010]] + [""] * 30 + [lead(CAP, rng)])
        assert int(ids[int(off[33])]) == ord("e") and int(off[34]) - int(off[33]) == 1


def chunk_of(words):
    assert nbytes(" ".join(words)) <= CAP - 16, "the words share one chunk"
    return " ".join(words)


def list_texts(two, five, nine, one):
    """chunks that hold 0, 1, 63, 64, 65, 128 and 129 words of a class (as far as a chunk holds them), alone, with one-symbol
    words between, and with the classes interleaved; lengths 4 / 5, 8 / 9 and 32 / 33 side by side"""
    rng = random.Random(0x4E06)
    texts = [chunk_of([one] * 100)]
    for k in (1, 63, 64, 65, 128, 129):
        texts.append(chunk_of([rng.choice(two) for _ in range(k)]))
        texts.append(chunk_of([w for _ in range(k) for w in (rng.choice(two), one)][:2 * k - 1]) if 5 * k <= CAP - 16 else chunk_of([rng.choice(two) for _ in range(k)] + [one]))
    for k in (1, 63, 64, 65):
        texts.append(chunk_of([rng.choice(five) for _ in range(k)]))
    for k in (1, 55):
        texts.append(chunk_of([rng.choice(nine) for _ in range(k)]))
    texts.append(chunk_of([w for _ in range(28) for w in (rng.choice(two), rng.choice(nine), one, rng.choice(five))]))
    texts.append(chunk_of([w for _ in range(22) for w in (rng.choice(nine), rng.choice(five), rng.choice(two), rng.choice(two))]))
    a = two[0][0]
    for n, m in ((4, 5), (8, 9), (32, 33)):
        texts.append(chunk_of([(two[0] * 17)[:n], (two[1] * 17)[:m], a * n, a * m, (five[0] * 7)[:m], (five[0] * 7)[:n]] * 2))
    return texts


def test_word_lists_pretrained(dev, pre):
    tok, orc, short, multibyte, cat = pre
    two = [w for w in short if len(w) == 2 and nbytes(w) == 2][:30]
    five = [w for w in short if len(w) == 5 and nbytes(w) == 5][:30]
    nine = [cat[3000 + 9 * k:3009 + 9 * k] for k in range(30)]
    texts = list_texts(two, five, nine, "a")
    both(dev, tok, orc, texts + [""] * 50)
    for t in texts:  # and each alone in its call, the chunk opening the text
        run(dev, tok, orc, tiled([t]))


def test_word_lists_unpacked_and_improper(swt, oracle, dev, unpacked):
    utok, uorc = unpacked
    rng = random.Random(0x4E07)
    mk = lambda n, k: ["".join(rng.choice(ALPHABET[:8]) for _ in range(n)) for _ in range(k)]
    texts = list_texts(mk(2, 20), mk(5, 20), mk(9, 20), "a")
    run(dev, utok, uorc, texts + [""] * 50, narrow=0)
    tok, orc = make(swt, oracle, IMPROPER)
    assert info(dev, tok._table, 8) == 1 and info(dev, tok._table, 2) == 0
    texts = list_texts(["ab", "aa", "xy", "cd"], ["abcab", "aaaaa", "xyxyx"], ["abcabcabc", "aaaaaaaaa", "abcdxyabc"], "b")
    both(dev, tok, orc, texts + [""] * 50)


def test_word_lists_under_the_other_orders(swt, dev):
    """the same lists through NaiveBPE's list order (a list whose order cannot matter: the proper list with a pair repeated at its
    end) and through BPE-dropout at drop_below = 0: both spell FastBPE's words"""
    texts = list_texts(["ab", "cd", "xy", "qq"], ["abcda", "xyxyx", "qqqqq"], ["abcdabcdq", "xyxyxyxyx", "qqqqqqqqq"], "a")
    c = Case(swt, dev, D.PROPER)
    text, off = dev.pack_and_lower(texts)
    plain = c.tok._table.encode(text, off, flags=dev.BPE_NO_DEDUP)
    same(c.got(texts, 0), plain, "drop_below 0 against swt_bpe_encode")
    naive = swt.NaiveBPE()
    naive.merges_list = list(D.PROPER + [D.PROPER[0]])
    assert not naive._ensure_naive_table().order_equivalent()
    assert naive.tokenize_batch(texts) == c.tok.tokenize_batch(texts)


def test_rounds_by_word_length(dev, pre, unpacked, swt, oracle):
    """every word length from 2 to 33 symbols (the scan's trips: one clamped trip up to five symbols, K = (n - 2) / 4 plain trips
    before it from six), words whose first merge is at slot 0, at the last pair and in the middle, a word of 32 symbols that
    merges down to one, and a FOREIGN left neighbour of the merge"""
    tok, orc, short, multibyte, cat = pre
    rng = random.Random(0x4E08)
    words = [cat[3000 + 40 * n:3000 + 41 * n] for n in range(2, 34)]
    assert [len(w) for w in words] == list(range(2, 34))
    # "ie" merges early in the pretrained list: first merge at slot 0, at the last pair, in the middle
    words += ["ie", "iex", "xie", "iexx", "xiex", "xxie", "iexxx", "xxiex", "xxxie", "ieie", "ieieie"]
    words += [FOREIGN[0] + "ie", "x" + FOREIGN[1] + "ie", FOREIGN[2] + "ien", "ie" + FOREIGN[0]]
    every(dev, tok, orc, unpacked, tiled([w + " " + rng.choice(words) for w in words]))
    every(dev, tok, orc, unpacked, tiled([fill(words, 2 * CAP + 9, rng)]))
    # a power-of-two chain: 32 letters merge down to one symbol in five rounds of the same pair
    chain, s = [], "a"
    for _ in range(5):
        chain.append((s, s))
        s += s
    ctok, corc = make(swt, oracle, chain + [("b", "a"), ("a", "b")])
    assert info(dev, ctok._table, 8) == 1
    ids, off = both(dev, ctok, corc, tiled(["a" * 32 + " " + "a" * 31 + " " + "a" * 33 + " b" + "a" * 32 + " é" + "a" * 4 + " " + "a" * 16 + "b"]))
    assert int(off[-1]) - int(off[-2]) >= 6 and int(ids[int(off[-2])]) == ctok._syms.intern("a" * 32)
    tok, orc = make(swt, oracle, IMPROPER)
    words = ["ab", "abc", "aab", "aaa", "abcd", "xabc", "aaab", "abcab", "xyabc", "aaaaa", "a" * 32, "abc" * 11, "é" + "ab", "ab" + "é" + "abc"]
    both(dev, tok, orc, tiled([fill(words, 2 * CAP + 1, rng)] + words))
