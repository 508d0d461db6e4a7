#!/usr/bin/env python3
"""Golden vectors for added and special tokens written in the text, made with the `tokenizers` wheel (0.22.2) of
the build container: its added vocabulary is what swt_added_find / swt_added_splice restate.

  added_tokens.json  {"tokenizers": version, "vocab": the sorted vocabulary the ids index,
                      "cases": [{"name", "added": [[content, special]], "texts", "tokens", "ids", "offsets", "word_ids"}]}
      the tokenizer: WordPiece over ref/resources/tests/FastWordPiece/vocab.json (ids = the index in the sorted vocabulary, as
      NaiveWP's and FastWP's; len "['UNK']", len + 1 "[UNK]"), normalizers.Lowercase(), BertPreTokenizer(), no post-processor.
      An ordinary token is added as AddedToken(content.lower(), normalized=True), a special one as the wheel's special token.
      Per text of a case: the wheel's token strings, their ids (-1 for an added token, whose id is the wheel's own), their
      (start, end) in code points of the text and their word ids.

The cases are tests/added_cases.golden_cases().  Asserted here, for every text with no token added: the wheel's pieces are
NaiveWP.tokenize's (the reference's loop as this package keeps it in Python; no device), so that the in-between pieces of the
cases are what the classes under test make of them.

Usage: python tests/golden/make_golden_added_tokens.py   (not run by the tests: the GPU machine needs no wheel)
"""
import json
import os
import sys

import tokenizers
from tokenizers import AddedToken, Tokenizer, normalizers, pre_tokenizers
from tokenizers.models import WordPiece

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import added_cases as A  # noqa: E402


def make(vocab, added=()):
    ids = {tok: i for i, tok in enumerate(vocab)}
    ids["['UNK']"], ids["[UNK]"] = len(vocab), len(vocab) + 1
    t = Tokenizer(WordPiece(ids, unk_token="[UNK]"))
    t.normalizer = normalizers.Lowercase()
    t.pre_tokenizer = pre_tokenizers.BertPreTokenizer()
    for content, special in added:
        if special:
            assert t.add_special_tokens([content]) == 1
        else:
            assert t.add_tokens([AddedToken(content.lower(), normalized=True)]) == 1
    return t


def main():
    import subword_tokenizers_amd as S

    with open(os.path.join(HERE, "ref", "resources", "tests", "FastWordPiece", "vocab.json"), encoding="utf-8") as f:
        vocab = sorted(set(json.load(f)))
    naive = S.NaiveWP()
    naive.vocab = set(vocab)
    plain = make(vocab)
    cases = []
    for name, added, texts in A.golden_cases():
        t = make(vocab, added)
        names = {content if special else content.lower() for content, special in added}
        rec = {"name": name, "added": [[c, bool(s)] for c, s in added], "texts": texts, "tokens": [], "ids": [], "offsets": [], "word_ids": []}
        for text in texts:
            assert "Σ" not in text and len(text.lower()) == len(text)
            assert plain.encode(text, add_special_tokens=False).tokens == naive.tokenize(text), text
            enc = t.encode(text, add_special_tokens=False)
            rec["tokens"].append(enc.tokens)
            rec["ids"].append([-1 if tok in names else i for tok, i in zip(enc.tokens, enc.ids)])
            rec["offsets"].append([list(o) for o in enc.offsets])
            rec["word_ids"].append(enc.word_ids)
        cases.append(rec)
    out = {"tokenizers": tokenizers.__version__, "vocab": vocab, "cases": cases}
    path = os.path.join(HERE, "added_tokens.json")
    with open(path, "w", encoding="utf-8") as f:
        json.dump(out, f, ensure_ascii=False, separators=(",", ":"))
    print(path, sum(len(c["texts"]) for c in cases), "texts", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
