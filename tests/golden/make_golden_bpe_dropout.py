#!/usr/bin/env python3
"""Recorded answers of the BPE-dropout model (tests/dropout_cases.py), so that the model itself cannot drift unnoticed.  The
reference has no dropout; nothing here imports it.

  bpe_dropout.json  {"texts_ref", "rows", "cases": [{"probability", "drop_below", "seed", "epoch", "tokens"}]}
                    tokens[j] = the model's tokens of sentence rows[j] of ref/data/pan_tadeusz.json under the pretrained FastBPE
                    merges (ref/resources/pretrained/FastBPE), sentence index j, for each of three (probability, seed, epoch).

Usage: python tests/golden/make_golden_bpe_dropout.py   (from the repository root; needs the built library for the split)
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

ROWS = list(range(0, 200, 10))  # twenty sentences
CASES = [(0.1, 0, 0), (0.5, (1 << 63) + 12345, 7), (0.02, 3, 0xFFFFFFFF)]


def main():
    from subword_tokenizers_amd.tokenizers import SubwordTokenizer
    from tests import dropout_cases as D

    ref = os.path.join(HERE, "ref")
    with open(os.path.join(ref, "resources/pretrained/FastBPE/merges.json"), encoding="utf-8") as f:
        table = D.Table(json.load(f))
    with open(os.path.join(ref, "data/pan_tadeusz.json"), encoding="utf-8") as f:
        pan = json.load(f)
    texts = [pan[r] for r in ROWS]
    cases = []
    for p, seed, epoch in CASES:
        below = D.drop_below(p)
        cases.append({"probability": p, "drop_below": below, "seed": seed, "epoch": epoch,
                      "tokens": D.tokenize(table, SubwordTokenizer._split, texts, below, seed, epoch)})
    out = {"texts_ref": "ref/data/pan_tadeusz.json", "rows": ROWS, "cases": cases}
    path = os.path.join(HERE, "bpe_dropout.json")
    with open(path, "w", encoding="utf-8") as f:
        json.dump(out, f, ensure_ascii=False, indent=0)
        f.write("\n")
    size = os.path.getsize(path)
    assert size < 100 * 1024, size
    print("%d sentences x %d cases, %d bytes" % (len(ROWS), len(CASES), size))


if __name__ == "__main__":
    main()
