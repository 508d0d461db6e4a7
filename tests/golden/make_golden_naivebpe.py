#!/usr/bin/env python3
"""Golden vectors for NaiveBPE.tokenize (bpe.py:114-158: the merges applied in LIST order), made by IMPORTING THE REFERENCE
(build container only).

  naivebpe.json  {"texts": the hand-made inputs,
                  "shipped": {name: {"naive": path in the reference, "merges_ref": the FastBPE copy under ref/, "identical": bool}},
                  "cases": [{name, merges | merges_ref, texts_ref, index?, tokens | tokens_ref, whole?, differs_from_fastbpe}]}
                 tokens[i] = the reference's NaiveBPE token list for texts[i] (for texts[index[i]] where index is given).
                 A case with "whole" is one of the shipped tables, whose 19,876 merges make the literal loop slow: there the
                 reference's encode_word ran once per DISTINCT word and the sentences were put together from those, except the
                 sentences listed in "whole" (positions in the case's texts), on which tokenize() itself ran as well (asserted
                 equal).  Every other case is tokenize() on every text.  Where the result equals a token list that is already
                 under tests/golden/ (asserted here) the case stores "tokens_ref" instead of the tokens.
                 differs_from_fastbpe = on how many texts the reference's FastBPE.tokenize, on the same merges, gives other tokens.

Same shim recipe as make_golden.py.  Usage: python tests/golden/make_golden_naivebpe.py  (~3 min)
"""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, REF)
sys.path.insert(0, HERE)
from make_golden import dump, make_shim  # noqa: E402

# merge lists that tell list order (NaiveBPE) from lowest rank first (FastBPE), and the corners of the symbol naming
LISTS = {
    # a pair listed twice with merges between: the dict of bpe.py:257 keeps the LAST position, the list applies both
    "listed_twice": [("b", "c"), ("a", "b"), ("x", "y"), ("b", "c"), ("x", "x"), ("y", "x"), ("x", "y")],
    # the second position is the one that finds something (("ab", "ab") has nothing to merge before ("a", "b") ran), the third
    # is the one the dict keeps
    "listed_twice_second_applies": [("ab", "ab"), ("a", "b"), ("ab", "ab"), ("b", "ab"), ("ab", "ab"), ("c", "ab")],
    # a pair ranked below a merge that produces one of its symbols: it is passed before its symbol exists
    "below_its_producer": [("ab", "c"), ("a", "b"), ("bc", "a"), ("b", "c"), ("x", "xx"), ("x", "x")],
    # two pairs spelling the same string: one symbol by string identity (bpe.py:41)
    "same_string": [("a", "b"), ("b", "c"), ("a", "bc"), ("ab", "c"), ("abc", "abc"), ("abc", "a")],
    # pairs over strings no merge produces
    "not_producible": [("xy", "z"), ("q", "rs"), ("a", "b"), ("ab", "zz"), ("abc", "d"), ("b", "a")],
    "empty": [],
    "multibyte_punctuation": [("ż", "ó"), ("żó", "ł"), ("ł", "ć"), ("z", "a"), ("za", "żół"), ("za", "żół"), ("ę", "ś"), ("g", "ęś"),
                              ("!", "!"), ("€", "€"), ("中", "日"), ("😀", "😀"), ("ß", "e"), ("s", "s"), ("ο", "δ"), ("ο", "σ"),
                              ("ο", "ς"), (".", "."), ("a", "."), ("-", "b"), ("ź", "ń"), ("źń", "źń"), ("ja", "źń"), ("j", "a")],
    # long words: more than 32 symbols, merged in list order and against it
    "long": [("x", "x"), ("xx", "xx"), ("y", "y"), ("yy", "y"), ("x", "y"), ("xxxx", "xxxx"), ("a", "b"), ("ab", "ab"), ("b", "a"),
             ("abab", "abab"), ("yyy", "yyy"), ("y", "yyy")],
    "long_against_order": [("xxxx", "xxxx"), ("xx", "xx"), ("x", "x"), ("xx", "xx"), ("abab", "ab"), ("ab", "ab"), ("a", "b"),
                           ("ab", "ab"), ("y", "yy"), ("y", "y"), ("y", "yy")],
}
TEXTS = ["", " ", "a", "b", "ab", "abc", "abab", "a b", "ba", "aab", "bca", "bcab", "abcabc", "abcabcabc", "ababab", "abababab",
         "cab", "cabab", "babab", "bababab", "xyx", "xyxy yxyx", "abcd", "abzz", "xyz", "qrs", "xy xyz", "Abc ABC aBc", "x x", "xb", "axb", "xx", "xxx", "xxxx", "xxxxx",
         "aaa aaa", "abcabca", "abca", "bcbc", "abbc", "#", "##", "a#b", "a ## b",
         "zażółć gęślą jaźń", "ZAŻÓŁĆ GĘŚLĄ JAŹŃ", "zażółćż", "jaźńźń", "€€ 中日 😀😀", "straße STRASSE", "οδος ΟΔΟΣ", "öße",
         "a.b", "a.b.c", "(a)", "«ab»", "a—b", "a-b-c", "'ab'", "a,b!c?", "...", "!!", "a..",
         "x" * 45, "y" * 50, "xy" * 20, "ab" * 40, "abc" * 30, "xx xx xx", "a" * 33 + "b", "ab" * 16 + "c", "x" * 700,
         "a b", "a　b", "a\tb\nc", "İx", "ǅ", "ﬁ"]


def main():
    t0 = time.time()
    from source.bpe import FastBPE, NaiveBPE

    shim = make_shim()

    def naive(merges):
        tok = NaiveBPE(shim)
        tok.merges_list = [tuple(p) for p in merges]
        return tok

    def fast(merges):
        tok = FastBPE(shim)
        tok.merges_list = [tuple(p) for p in merges]
        tok._bpe_ranks = {pair: i for i, pair in enumerate(tok.merges_list)}  # bpe.py:257
        return tok

    def by_words(tok, texts, whole):
        """tokenize() put together from one encode_word per distinct word; tokenize() itself on the sentences in `whole`"""
        memo, out = {}, []
        for s in texts:
            toks = []
            for w, _ in tok.preprocessing([s])[0]:
                if w not in memo:
                    memo[w] = tok.encode_word(w)
                toks += memo[w]
            out.append(toks)
        for i in whole:
            assert tok.tokenize(texts[i]) == out[i]
        return out, len(memo)

    ref = os.path.join(HERE, "ref")
    shipped, merges_of = {}, {}
    for name in ("pretrained", "tests"):
        theirs = "resources/%s/NaiveBPE/merges.json" % name
        ours = "ref/resources/%s/FastBPE/merges.json" % name
        with open(os.path.join(REF, theirs), "rb") as a, open(os.path.join(HERE, ours), "rb") as b:
            identical = a.read() == b.read()
        # the reference ships byte-identical merges.json files for NaiveBPE and FastBPE: the copy under ref/ serves both
        assert identical, "%s differs from %s: it needs a copy of its own under ref/" % (theirs, ours)
        shipped[name] = {"naive": theirs, "merges_ref": ours, "identical": identical}
        merges_of[name] = json.load(open(os.path.join(HERE, ours), encoding="utf-8"))
    cases = []

    pan = json.load(open(os.path.join(ref, "data/pan_tadeusz.json"), encoding="utf-8"))
    author = json.load(open(os.path.join(ref, "data/pan_tadeusz.tokens.json"), encoding="utf-8"))["FastBPE"]
    whole = list(range(0, len(pan), 99))
    got, n_words = by_words(naive(merges_of["pretrained"]), pan, whole)
    assert got == author, "NaiveBPE on pan_tadeusz differs from the author's NaiveBPE list"
    cases.append({"name": "pan_tadeusz_pretrained", "merges_ref": shipped["pretrained"]["merges_ref"], "texts_ref": "ref/data/pan_tadeusz.json",
                  "tokens_ref": "ref/data/pan_tadeusz.tokens.json#FastBPE", "whole": whole, "differs_from_fastbpe": 0})
    print("pan_tadeusz: %d sentences, %d distinct words, %.1fs" % (len(pan), n_words, time.time() - t0), flush=True)

    fz = json.load(open(os.path.join(HERE, "fuzz_bpe.json"), encoding="utf-8"))["sentences"]
    fuzz = [c["text"] for c in fz]
    # a sample of the fuzz sentences: corpus sentences with insertions, random strings, then the hand-picked edge cases
    index = list(range(0, 40)) + list(range(300, 340)) + list(range(len(fuzz) - 66, len(fuzz)))
    texts = [fuzz[i] for i in index]
    got, n_words = by_words(naive(merges_of["pretrained"]), texts, list(range(0, len(texts), 12)))
    diff = sum(a != fz[i]["pretrained"] for a, i in zip(got, index))
    cases.append({"name": "fuzz_pretrained", "merges_ref": shipped["pretrained"]["merges_ref"], "texts_ref": "fuzz_bpe.json#sentences",
                  "index": index, "tokens": got, "whole": list(range(0, len(texts), 12)), "differs_from_fastbpe": diff})
    print("fuzz_pretrained: %d inputs, %d distinct words, %d differ from FastBPE, %.1fs" % (len(index), n_words, diff, time.time() - t0), flush=True)

    tok, ftok = naive(merges_of["tests"]), fast(merges_of["tests"])
    got = [tok.tokenize(s) for s in texts]
    cases.append({"name": "fuzz_tutorial", "merges_ref": shipped["tests"]["merges_ref"], "texts_ref": "fuzz_bpe.json#sentences",
                  "index": index, "tokens": got, "differs_from_fastbpe": sum(a != ftok.tokenize(s) for a, s in zip(got, texts))})
    got = [tok.tokenize(s) for s in pan[:60]]
    cases.append({"name": "pan_tadeusz_tutorial", "merges_ref": shipped["tests"]["merges_ref"], "texts_ref": "ref/data/pan_tadeusz.json",
                  "index": list(range(60)), "tokens": got, "differs_from_fastbpe": sum(a != ftok.tokenize(s) for a, s in zip(got, pan[:60]))})

    for name, merges in LISTS.items():
        tok, ftok = naive(merges), fast(merges)
        got = [tok.tokenize(s) for s in TEXTS]
        diff = sum(a != ftok.tokenize(s) for a, s in zip(got, TEXTS))
        cases.append({"name": name, "merges": [list(p) for p in merges], "texts_ref": "naivebpe.json#texts", "tokens": got,
                      "differs_from_fastbpe": diff})
        print("%s: %d merges, %d of %d texts differ from FastBPE" % (name, len(merges), diff, len(TEXTS)), flush=True)
    # without a case on which the two algorithms disagree the fixture says nothing about order
    assert any(c["differs_from_fastbpe"] for c in cases)
    for name in ("listed_twice", "listed_twice_second_applies", "below_its_producer", "long_against_order"):
        assert [c for c in cases if c["name"] == name][0]["differs_from_fastbpe"] > 0, name
    dump("naivebpe.json", {"texts": TEXTS, "shipped": shipped, "cases": cases})
    assert os.path.getsize(os.path.join(HERE, "naivebpe.json")) <= os.path.getsize(os.path.join(HERE, "fuzz_bpe.json"))
    print("done in %.1fs" % (time.time() - t0))


if __name__ == "__main__":
    main()
