"""token_sequence_equivalence (source/benchmarks.py:113-183) without a GPU: the canonical id maps that make the ids of two
tokenizers comparable (metrics._canonical_map), and the retained Python body for objects that only have `tokenize`."""
import numpy as np


def test_canonical_maps_share_one_id_per_stripped_string(swt, native):
    from subword_tokenizers_amd import metrics as M

    bpe = swt.FastBPE()
    bpe.merges_list = [("i", "n"), ("in", "g"), ("#", "#")]
    bpe._build_table()
    assert bpe._syms.strings == ["in", "ing", "##"]
    wp = swt.NaiveWP()
    wp.vocab = {"ing", "##ing", "a", "##a", "##", "in", "[UNK]"}
    canon = M._Canon()
    bmap, bbase, bflag = M._canonical_map(bpe, canon)
    wmap, wbase, wflag = M._canonical_map(wp, canon)
    tokens = sorted(wp.vocab)
    assert bmap.dtype == np.uint32 and wmap.dtype == np.uint32
    assert (bbase, bflag, bmap.size) == (native.SYM_BASE, True, 2 * 3)
    assert (wbase, wflag, wmap.size) == (0, False, len(tokens) + 2)
    at = {t: int(wmap[i]) for i, t in enumerate(tokens)}
    # "ing", "##ing" and the BPE symbol `ing` with and without SWT_BPE_CONT: one id
    assert at["ing"] == at["##ing"] == int(bmap[1]) == int(bmap[3 + 1]) >= native.SYM_BASE
    assert at["in"] == int(bmap[0]) == int(bmap[3 + 0]) != at["ing"]
    # a one-code-point string is its ordinal, with the prefix or without
    assert at["a"] == at["##a"] == 97 == canon.intern("a")
    # "##" strips to "": the WordPiece token "##", the BPE symbol "##" without the flag, and the empty string itself
    assert at["##"] == int(bmap[2]) == canon.intern("") >= native.SYM_BASE
    # ... while "##" + "##" (the flagged BPE symbol) strips to "##", another string
    assert int(bmap[3 + 2]) == canon.intern("##") != canon.intern("")
    # the two spellings of the unknown token (wordpiece.py:257 and :149) are different strings
    unk_sic, unk = int(wmap[len(tokens)]), int(wmap[len(tokens) + 1])
    assert unk_sic == canon.intern("['UNK']") and unk == canon.intern("[UNK]") and unk_sic != unk
    assert unk == at["[UNK]"]  # a vocabulary entry spelled "[UNK]" is the same string
    # every multi-character string has its own id
    multi = {"in", "ing", "", "##", "['UNK']", "[UNK]"}
    assert len({canon.intern(s) for s in multi}) == len(multi)


class _Table:
    """a tokenizer that only has `tokenize`"""

    def __init__(self, table):
        self.table = table

    def tokenize(self, text):
        return list(self.table[text])


def test_python_body_serves_objects_that_only_have_tokenize(swt):
    from subword_tokenizers_amd import metrics as M

    t1 = _Table({"ab cd": ["ab", "##c", "d"], "ab ab": ["ab", "ab"], "x": ["x"], "ab": ["ab"], "cd": ["##c", "d"]})
    t2 = _Table({"ab cd": ["ab", "c", "c", "d"], "ab ab": ["a", "##ab", "ab"], "x": [], "ab": ["a", "b"], "cd": ["c", "##d"]})
    # sentence 1: [ab c d] / [ab c c d]: 3 positions, 2 equal, multiset intersection ab + c + d = 3
    # sentence 2: [ab ab] / [a ab ab]:   2 positions, 1 equal, intersection min(2, 2) = 2
    # sentence 3: [x] / []:              0 positions
    # words ab, cd, ab, ab, x: only "cd" ({c, d} on both sides) shares a token
    want = (3, 5, 3 / 5 * 100, 5, 5 / 5 * 100, 1, 5, 1 / 5 * 100)
    assert M.token_sequence_equivalence(t1, t2, ["ab cd", "ab ab", "x"]) == want
    assert M.token_sequence_equivalence(t1, t2, []) == (0, 0, 0.0, 0, 0.0, 0, 0, 0.0)
