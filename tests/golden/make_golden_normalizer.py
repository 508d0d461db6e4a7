#!/usr/bin/env python3
"""Golden vectors for the BERT normalizer, made with the `tokenizers` wheel (0.22.2): its
BertNormalizer is what swt_normalize_* restate.

  bert_normalizer.json  {"tokenizers": version,
                         "settings": {name: {"flags", "texts": tests/normalizer_cases.TEXTS without the dropped ones,
                                             "normalized": [str], "tokens", "ids", "offsets"}}}
      per setting -- all four flags, strip_accents off, lowercase (and with it strip_accents) off -- the wheel's normalised
      strings, and the tokens, ids and (start, end) in code points of the ORIGINAL text of a BertNormalizer + BertPreTokenizer
      + WordPiece encode over ref/resources/pretrained/FastWordPiece/vocab.json (ids = the index in the sorted vocabulary,
      which is FastWP's dense id; len + 1 "[UNK]").

Asserted here: tests/normalizer_cases.normalize gives the wheel's strings.  The wheel's Unicode tables are newer than the
device's, so the cases hold only code points assigned long before either.

Usage: python tests/golden/make_golden_normalizer.py   (not run by the tests: the GPU machine needs no wheel)
"""
import json
import os
import sys

import tokenizers
from tokenizers import Tokenizer, normalizers, pre_tokenizers
from tokenizers.models import WordPiece

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import normalizer_cases as M  # noqa: E402

SETTINGS = {"all": M.ALL, "no_strip": M.NO_STRIP, "no_lower": dict(M.NO_LOWER, strip_accents=False)}
# Dropped, by index in tests/normalizer_cases.TEXTS: the texts FastWP refuses under that setting -- it restates the reference's fast
# WordPiece walk, which never returns on some words the vocabulary does not cover (SWT_WP_NONTERMINATING, with or without a
# normalizer; found by encoding the cases on the device), where the wheel answers "[UNK]": the emoji text under every setting, the
# texts whose marks stay in the text where they stay ('İ' lowercases to 'i' + U+0307), and under the cased setting "[MASK] ... [SEP]",
# whose capitals the lowercase vocabulary lacks.  Model and wheel agree on the strings of all of them (asserted below).  Nothing
# had to be dropped for the order of marks: no setting here both decomposes and keeps them.
DROPPED = {"all": {10}, "no_strip": {8, 9, 10}, "no_lower": {9, 10, 16}}


def main():
    with open(os.path.join(HERE, "ref", "resources", "pretrained", "FastWordPiece", "vocab.json"), encoding="utf-8") as f:
        vocab = sorted(set(json.load(f)))
    ids = {tok: i for i, tok in enumerate(vocab)}
    ids["['UNK']"], ids["[UNK]"] = len(vocab), len(vocab) + 1
    out = {"tokenizers": tokenizers.__version__, "settings": {}}
    for name, flags in SETTINGS.items():
        norm = normalizers.BertNormalizer(**flags)
        t = Tokenizer(WordPiece(ids, unk_token="[UNK]"))
        t.normalizer, t.pre_tokenizer = norm, pre_tokenizers.BertPreTokenizer()
        for text in M.TEXTS:  # the strings of every case, the dropped ones too
            assert M.normalize(text, flags)[0] == norm.normalize_str(text), (name, text)
        texts = [t for i, t in enumerate(M.TEXTS) if i not in DROPPED[name]]
        rec = {"flags": flags, "texts": texts, "normalized": [], "tokens": [], "ids": [], "offsets": []}
        for text in texts:
            rec["normalized"].append(norm.normalize_str(text))
            enc = t.encode(text, add_special_tokens=False)
            rec["tokens"].append(enc.tokens)
            rec["ids"].append(enc.ids)
            rec["offsets"].append([list(o) for o in enc.offsets])
        out["settings"][name] = rec
    path = os.path.join(HERE, "bert_normalizer.json")
    with open(path, "w", encoding="utf-8") as f:
        json.dump(out, f, ensure_ascii=False, separators=(",", ":"))
    print(path, [len(r["texts"]) for r in out["settings"].values()], "texts", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
