#!/usr/bin/env python3
"""Golden vectors for NaiveWP.tokenize (wordpiece.py:132-179), made by IMPORTING THE REFERENCE (build container only).

  naivewp.json   {"texts": the hand-made inputs, "cases": [{name, vocab | vocab_ref, texts_ref, index?, tokens | tokens_ref}]}
                 tokens[i] = the reference's token list for texts[i] (for texts[index[i]] where index is given), or "TIMEOUT"
                 when it did not return within the alarm (the longest-prefix loop never ends on that input: SURVEY.md A.5).
                 The pan_tadeusz case stores no tokens: the reference's output equals the author's
                 ref/data/pan_tadeusz.tokens.json (asserted here), which the tests read.

Same shim recipe as make_golden.py.  Usage: python tests/golden/make_golden_naivewp.py  (~1 min)
"""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")
sys.path.insert(0, HERE)
from make_golden import Timeout, dump, make_shim, with_alarm  # noqa: E402

# vocabularies for the corners of the loop: '#' / '##' in or out, a word that is "[UNK]" after a matched first piece,
# multi-byte and punctuation tokens, long words
VOCABS = {
    "sharp_in_double_out": ["a", "b", "ab", "##b", "##c", "#", "x", "##x"],
    "double_in": ["a", "b", "##b", "##", "#", "c"],
    "double_in_sharp_out": ["a", "b", "##b", "##"],
    "no_sharps": ["a", "b", "##b", "ab", "##ab", "c"],
    "unk_after_first_piece": ["un", "##aff", "##able", "a", "##b", "x", "xy", "##z"],
    "triple_sharp_only": ["a", "##a", "#", "###", "b"],
    "multibyte": ["zażółć", "za", "##żółć", "##ż", "##ó", "##ł", "##ć", "gęślą", "gę", "##ślą", "jaźń", "ja", "##źń", "€", "中", "##日",
                  "😀", "ß", "straße", "ο", "##δ", "##ο", "##σ", "##ς", "ö"],
    "punctuation": [".", ",", "!", "?", "(", ")", "«", "»", "—", "-", "a", "b", "##b", "ab", "a.b", "##.", "'", "\""],
    "long": ["x", "##x", "xx", "##xx", "xxxx", "##xxxx", "y" * 40, "##" + "y" * 7, "y", "##y"],
    "empty": [],
}
TEXTS = ["", " ", "a", "b", "ab", "abc", "abab", "a b", "ba", "aab", "#", "##", "###", "a#b", "a ## b", "#a", "a#", "# #",
         "unaffable", "unaffab", "xyz", "xy xyz", "Unaffable ab", "c", "cab", "x x", "xb", "axb",
         "zażółć gęślą jaźń", "ZAŻÓŁĆ GĘŚLĄ JAŹŃ", "zażółćż", "jaźńźń", "€€ 中日 😀", "straße STRASSE", "οδος ΟΔΟΣ", "öß",
         "a.b", "a.b.c", "(a)", "«ab»", "a—b", "a-b-c", "'ab'", "\"a\"", "a,b!c?", "...",
         "x" * 45, "y" * 50, "xy" * 20, "xx xx xx",
         "a b", "a　b", "a\tb\nc", "İx", "ǅ", "ﬁ"]


def main():
    t0 = time.time()
    import source.wordpiece as W

    shim = make_shim()

    def naive(vocab):
        tok = W.NaiveWP(shim)
        tok.vocab = set(vocab)
        return tok

    def run(tok, s, seconds=0.3):
        try:  # the loop is quadratic in a word's length: long inputs get longer
            return with_alarm(lambda: tok.tokenize(s), seconds + len(s) * 0.004)
        except Timeout:
            return "TIMEOUT"

    ref = os.path.join(HERE, "ref")
    pre = json.load(open(os.path.join(ref, "resources/pretrained/FastWordPiece/vocab.json"), encoding="utf-8"))
    tut = json.load(open(os.path.join(ref, "resources/tests/FastWordPiece/vocab.json"), encoding="utf-8"))
    # the reference ships byte-identical vocab.json files for NaiveWordPiece and FastWordPiece
    assert pre == json.load(open("/root/reference/resources/pretrained/NaiveWordPiece/vocab.json", encoding="utf-8"))
    assert tut == json.load(open("/root/reference/resources/tests/NaiveWordPiece/vocab.json", encoding="utf-8"))
    cases = []

    pan = json.load(open(os.path.join(ref, "data/pan_tadeusz.json"), encoding="utf-8"))
    author = json.load(open(os.path.join(ref, "data/pan_tadeusz.tokens.json"), encoding="utf-8"))["FastWordPiece"]
    tok = naive(pre)
    got = [run(tok, s, 2.0) for s in pan]
    assert got == author, "NaiveWP on pan_tadeusz differs from the author's NaiveWordPiece list"
    cases.append({"name": "pan_tadeusz_pretrained", "vocab_ref": "ref/resources/pretrained/FastWordPiece/vocab.json",
                  "texts_ref": "ref/data/pan_tadeusz.json", "tokens_ref": "ref/data/pan_tadeusz.tokens.json#FastWordPiece"})
    print("pan_tadeusz: %d sentences, %.1fs" % (len(pan), time.time() - t0), flush=True)

    fuzz = [c["text"] for c in json.load(open(os.path.join(HERE, "fuzz_wp.json"), encoding="utf-8"))["sentences"]]
    # a sample of the fuzz sentences (random text over letters, then over punctuation and white space, then the hand-picked
    # edge cases); longer inputs are checked against the model of tests/test_naive_wp_encode.py on the device
    index = [i for i in list(range(0, 30)) + list(range(466, 496)) + list(range(len(fuzz) - 66, len(fuzz))) if len(fuzz[i]) < 80]
    for name, vocab, vref in (("fuzz_tutorial", tut, "ref/resources/tests/FastWordPiece/vocab.json"),
                              ("fuzz_pretrained", pre, "ref/resources/pretrained/FastWordPiece/vocab.json")):
        tok = naive(vocab)
        toks = [run(tok, fuzz[i]) for i in index]
        cases.append({"name": name, "vocab_ref": vref, "texts_ref": "fuzz_wp.json#sentences", "index": index, "tokens": toks})
        print("%s: %d inputs, %d timeouts, %.1fs" % (name, len(index), sum(t == "TIMEOUT" for t in toks), time.time() - t0), flush=True)

    for name, vocab in VOCABS.items():
        tok = naive(vocab)
        cases.append({"name": name, "vocab": sorted(vocab), "texts_ref": "naivewp.json#texts", "tokens": [run(tok, s) for s in TEXTS]})
    dump("naivewp.json", {"texts": TEXTS, "cases": cases})
    print("done in %.1fs" % (time.time() - t0))


if __name__ == "__main__":
    main()
