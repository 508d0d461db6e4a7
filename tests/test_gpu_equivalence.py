"""token_sequence_equivalence (source/benchmarks.py:113-183) on the device: swt_token_equivalence over two id streams against a
Counter / set restatement written here, and metrics.equivalence_metrics against the values the imported reference gave
(tests/golden/make_golden_equivalence.py) and against the retained Python body."""
import contextlib
import io
import json
import os
from collections import Counter

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CONT = 0x80000000
V = 12000  # merged symbols of the flagged ("BPE") side = vocabulary of the plain ("WordPiece") side


@pytest.fixture(scope="module")
def dev(native):
    if native.device_count() < 1:
        pytest.fail("no HIP device")
    native.init(0)
    return native


def _maps(base):
    """side a: flagged, map_base = SYM_BASE, both halves permutations of side b's canonical ids; side b: plain, map_base = 0,
    [j] = SYM_BASE + j except that the first 26 are the letters (a's ids below its map_base are code points)"""
    rng = np.random.default_rng(11)
    map_b = (base + np.arange(V)).astype(np.uint32)
    map_b[:26] = np.arange(97, 123)
    map_a = np.concatenate([base + rng.permutation(V), base + rng.permutation(V)]).astype(np.uint32)
    map_a[V + 5] = map_a[5]  # symbol 5: the same canonical id with and without the flag
    assert map_a[6] != map_a[V + 6]
    return map_a, map_b


def _canon(ids, cmap, base, flagged):
    n_map = cmap.size // 2 if flagged else cmap.size
    out = []
    for t in map(int, ids):
        s = t & 0x7FFFFFFF
        out.append(s if s < base else int(cmap[(s - base) + (n_map if flagged and t >> 31 else 0)]))
    return out


def _brute(rows_a, rows_b, side_a, side_b):
    """benchmarks.py:148-156 and :166 over canonical ids"""
    out = []
    for ra, rb in zip(rows_a, rows_b):
        t1, t2 = _canon(ra, *side_a), _canon(rb, *side_b)
        n = min(len(t1), len(t2))
        f1, f2 = Counter(t1), Counter(t2)
        out.append((n, sum(1 for i in range(n) if t1[i] == t2[i]), sum(min(f1[t], f2[t]) for t in f1.keys() & f2.keys()),
                    1 if set(t1) & set(t2) else 0))
    return np.array(out, dtype=np.int64).reshape(-1, 4)


def _pack(rows):
    off = np.zeros(len(rows) + 1, dtype=np.uint64)
    if rows:
        np.cumsum([len(r) for r in rows], out=off[1:])
    ids = np.concatenate([np.asarray(r, dtype=np.uint32) for r in rows]) if rows else np.zeros(0, dtype=np.uint32)
    return ids.astype(np.uint32), off


def _rows(native):
    """the row shapes of the issue; ids of side a: SYM_BASE + k with a random flag or a letter, of side b: j"""
    base = native.SYM_BASE
    wave_cap, block_cap = native.token_equivalence_capacity()
    rng = np.random.default_rng(2024)
    map_a, map_b = _maps(base)
    inv_b = {int(c): j for j, c in enumerate(map_b)}

    def a_ids(n, spread):
        k = rng.integers(0, spread, size=n)
        ids = (base + k).astype(np.uint32) | np.where(rng.random(n) < 0.5, CONT, 0).astype(np.uint32)
        letters = rng.random(n) < 0.1
        ids[letters] = rng.integers(97, 123, size=int(letters.sum())) | np.where(rng.random(int(letters.sum())) < 0.5, CONT, 0)
        return ids.astype(np.uint32)

    def spell_b(canon_ids):
        """side b's ids for canonical ids (30 where b has no token for one: a's symbols that land on b's letter slots)"""
        return np.array([inv_b.get(int(c), 30) for c in canon_ids], dtype=np.uint32)

    def b_like(a, n, spread):
        """n ids of side b: about half spell a token of the row `a` (a quarter at its own position), the rest random"""
        out = rng.integers(0, spread, size=n).astype(np.uint32)
        if len(a):
            sb = spell_b(_canon(a, map_a, base, True))
            for i in np.flatnonzero(rng.random(n) < 0.5):
                out[i] = sb[i % len(sb)] if rng.random() < 0.5 else sb[int(rng.integers(len(sb)))]
        return out

    def a_distinct(n):
        return (base + rng.permutation(V)[:n]).astype(np.uint32)  # unflagged: the first half of the map is a permutation

    ra, rb = [], []

    def add(a, b):
        ra.append(np.asarray(a, dtype=np.uint32))
        rb.append(np.asarray(b, dtype=np.uint32))

    for la in (0, 1, 63, 64, 65):  # rows empty on one side only and on both are among these
        for lb in (0, 1, 63, 64, 65):
            a = a_ids(la, 40)
            add(a, b_like(a, lb, 40))
    for cap in (wave_cap, block_cap):  # the three lengths around each capacity, on either side, crowded and all distinct
        for n in (cap - 1, cap, cap + 1):
            a = a_ids(n, 50)
            add(a, b_like(a, n + 3, 50))
            a = a_ids(n + 5, 5000)
            add(a, b_like(a, n, 5000))
            add(a_distinct(n + 7), rng.permutation(np.arange(26, V))[:n])  # n DISTINCT tokens on the shorter side, some shared
            a = a_distinct(n)
            add(a, rng.permutation(np.concatenate([spell_b(_canon(a, map_a, base, True)), np.arange(7, dtype=np.uint32)])))
    a = a_ids(5000, 3000)  # several thousand tokens on both sides
    add(a, b_like(a, 7000, 3000))
    one_a, one_b = base + 77, int(spell_b([map_a[77]])[0])
    add([one_a] * 6000, [one_b])  # thousands of copies of ONE token against a row that holds it once
    add([one_a], [one_b] * 6000)
    add([one_a] * 6000, [one_b] * 300 + list(range(100, 400)))
    a = a_distinct(9000)  # an all-distinct long row against a shuffle of the same tokens
    add(a, rng.permutation(spell_b(_canon(a, map_a, base, True))))
    for n in (2 * block_cap, 4 * block_cap):  # all distinct and as many as the first partition is cut for: passes that must split
        a = a_distinct(n)
        add(a, rng.permutation(spell_b(_canon(a, map_a, base, True)))[:n - 11])
    n_general = len(ra)
    same, other = int(spell_b([map_a[5]])[0]), int(spell_b([map_a[6]])[0])
    add([base + 5, (base + 5) | CONT], [same, same])    # ids that differ only in SWT_BPE_CONT: one canonical id ...
    add([base + 6, (base + 6) | CONT], [other, other])  # ... and two
    return (ra, rb, (map_a, base, True), (map_b, 0, False), n_general)


def test_kernel_against_brute_force(dev):
    native = dev
    ra, rb, side_a, side_b, n_general = _rows(native)
    want = _brute(ra, rb, side_a, side_b)
    assert tuple(want[n_general]) == (2, 2, 2, 1) and tuple(want[n_general + 1]) == (2, 1, 1, 1)  # the flag rows, by hand
    assert want[:, 1].sum() > 1000 and want[:, 2].sum() > want[:, 1].sum() and 0 < want[:, 3].sum() < len(ra)
    sa, sb = _pack(ra) + side_a, _pack(rb) + side_b
    totals, rows = native.token_equivalence(sa, sb, per_row=True)
    print("rows", len(ra), "tokens", sa[0].size, sb[0].size, "totals", totals.tolist(), "want", want.sum(axis=0).tolist())
    bad = np.flatnonzero((rows.astype(np.int64) != want).any(axis=1))
    assert bad.size == 0, [(int(i), len(ra[i]), len(rb[i]), rows[i].tolist(), want[i].tolist()) for i in bad[:8]]
    assert [int(x) for x in totals] == want.sum(axis=0).tolist()
    # the sides swapped: the same numbers (min and the intersection are symmetric)
    totals_s, rows_s = native.token_equivalence(sb, sa, per_row=True)
    assert np.array_equal(rows_s, rows) and np.array_equal(totals_s, totals)
    # weights, 0 among them, whose sum exceeds 2**32: every row's four values times its weight, in 64 bits
    rng = np.random.default_rng(3)
    weight = rng.integers(2 ** 31, 2 ** 32, size=len(ra), dtype=np.uint64).astype(np.uint32)
    weight[::7] = 0
    weight[1::7] = 1
    assert int(weight.astype(np.uint64).sum()) > 2 ** 32
    got = native.token_equivalence(sa, sb, weight=weight)
    assert [int(x) for x in got] == [sum(int(w) * int(v) for w, v in zip(weight, want[:, c])) for c in range(4)]
    # no rows at all
    empty = (np.zeros(0, np.uint32), np.zeros(1, np.uint64))
    totals0, rows0 = native.token_equivalence(empty + side_a, empty + side_b, per_row=True)
    assert not totals0.any() and rows0.shape == (0, 4)
    # an id beyond its map (either side, flagged or not, short row or long)
    for a, b in (([native.SYM_BASE + V], [3]), ([native.SYM_BASE + 1], [V]), ([(native.SYM_BASE + V) | CONT] * 700, [3] * 700)):
        with pytest.raises(ValueError):
            native.token_equivalence(_pack([np.array(a, dtype=np.uint32)]) + side_a, _pack([np.array(b, dtype=np.uint32)]) + side_b)
    # a map entry of 0xFFFFFFFF is "no canonical id" too (include/swt.h): the id that reaches it is refused, its neighbours are not
    holed = side_b[0].copy()
    holed[40] = 0xFFFFFFFF
    row_a, ok, hit = _pack([np.array([native.SYM_BASE + 1, native.SYM_BASE + 2], dtype=np.uint32)]), np.array([39, 41], np.uint32), np.array([39, 40], np.uint32)
    native.token_equivalence(row_a + side_a, _pack([ok]) + (holed, 0, False))
    with pytest.raises(ValueError, match="1 token ids"):
        native.token_equivalence(row_a + side_a, _pack([hit]) + (holed, 0, False))


def _load(swt, ref_dir, name, res):
    tok = getattr(swt, name)()
    tok.load_resources(os.path.join(ref_dir, res))
    return tok


def _corpus(ref_dir, parts):
    out = []
    for rel, take in parts:
        with open(os.path.join(ref_dir, rel), encoding="utf-8") as f:
            out += json.load(f)[:take]
    return out


def test_fixture_parity(swt, dev, golden, ref_dir):
    """the eight values of the reference's token_sequence_equivalence for three tokenizer pairs: integers exact, floats ==.
    The reference's FastWP never returns from most of pan_tadeusz under the tutorial vocabulary, so for NaiveWP vs FastWP the
    fixture holds the whole corpus as "does not terminate" (here: RuntimeError, what tokenize_batch raises) and the values
    over the sentences the reference finishes."""
    from subword_tokenizers_amd import metrics as M

    entries = golden("equivalence.json")
    assert [(e["tokenizer1"], e["tokenizer2"], e["values"] is None) for e in entries] == [
        ("FastBPE", "FastWP", False), ("NaiveBPE", "FastBPE", False), ("NaiveWP", "FastWP", True), ("NaiveWP", "FastWP", False)]
    for e in entries:
        tok1, tok2 = _load(swt, ref_dir, e["tokenizer1"], e["resources1"]), _load(swt, ref_dir, e["tokenizer2"], e["resources2"])
        corpus = _corpus(ref_dir, e["corpus"])
        if e.get("keep") is not None:
            corpus = [corpus[i] for i in e["keep"]]
        assert len(corpus) == e["sentences"] > 100
        if e["values"] is None:
            with pytest.raises(RuntimeError, match="does not terminate"):
                M.equivalence_metrics(tok1, tok2, corpus)
            continue
        got = M.equivalence_metrics(tok1, tok2, corpus)
        print(e["tokenizer1"], e["tokenizer2"], got)
        assert [type(x) for x in got] == [int, int, float, int, float, int, int, float]
        assert list(got) == e["values"]
        assert M.token_sequence_equivalence(tok1, tok2, corpus) == got
        # the printed report: the reference's format strings (benchmarks.py:329-332) for those numbers
        pos, positions, pos_rate, unordered, unordered_rate, word_matches, total_words, word_rate = e["values"]
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            M.benchmarks(tok1, 0, corpus, pretrained=True, reference_tokenizers=[tok2], compare_only=True)
        out = buf.getvalue()
        assert "=== Token Sequence Equivalence (%s vs %s) ===\n" % (e["tokenizer1"], e["tokenizer2"]) in out
        assert f"Positional match rate: {pos_rate:.2f}% ({pos}/{positions})\n" in out
        assert f"Unordered match rate:  {unordered_rate:.2f}% ({unordered}/{positions})\n" in out
        assert f"Word match rate:       {word_rate:.2f}% ({word_matches}/{total_words})\n" in out


def test_device_path_agrees_with_the_python_body(swt, dev, ref_dir, corpora):
    from subword_tokenizers_amd import metrics as M

    bpe = _load(swt, ref_dir, "FastBPE", "resources/pretrained/FastBPE")
    wp = _load(swt, ref_dir, "FastWP", "resources/pretrained/FastWordPiece")
    got = M.equivalence_metrics(bpe, wp, corpora["pan"])
    assert got == M._equivalence_in_python(bpe, wp, corpora["pan"]) and got[1] > 10000
    assert M.equivalence_metrics(bpe, wp, []) == (0, 0, 0.0, 0, 0.0, 0, 0, 0.0)
    assert M.equivalence_metrics(bpe, wp, ["", "  "]) == M._equivalence_in_python(bpe, wp, ["", "  "])


def test_multi_token_corner_takes_the_python_body(swt, dev, ref_dir, monkeypatch):
    """a FastWP whose encode_word("##") is two tokens (tests/golden/fuzz_wp.json, the odd vocabularies): one id of its output
    stands for several tokens, so the comparison is counted from the token strings"""
    from subword_tokenizers_amd import metrics as M

    wp = swt.FastWP()
    wp.vocab = {"#", "###", "##a", "##b", "a", "b"}
    wp._build_trie()
    assert wp._corner == ["#", "###"]
    bpe = _load(swt, ref_dir, "FastBPE", "resources/tests/FastBPE")
    corpus = ["a ## b", "## a", "a b", "ab ##", "b"]
    ids, _off, status = wp.encode_ids_batch(corpus)
    assert not status.any() and int(ids.max()) == len(wp._tokens) + 2  # the marker is in the output
    assert wp.tokenize_batch(corpus)[:2] == [["a", "#", "###", "b"], ["#", "###", "a"]]
    want = M._equivalence_in_python(wp, bpe, corpus)
    calls = []
    real = M._equivalence_in_python
    monkeypatch.setattr(M, "_equivalence_in_python", lambda *a: calls.append(1) or real(*a))
    assert M.equivalence_metrics(wp, bpe, corpus) == want and calls == [1]
    assert M.token_sequence_equivalence(bpe, wp, corpus) == real(bpe, wp, corpus) and calls == [1, 1]
    # without the marker in the output the same objects are counted on the device
    assert M.equivalence_metrics(wp, bpe, ["a b", "ab"]) == real(wp, bpe, ["a b", "ab"]) and calls == [1, 1]
