#!/usr/bin/env python3
"""Recorded answers of the MaxMatch-Dropout model (tests/maxmatch_cases.py), so that the model itself cannot drift unnoticed.  The
reference has no dropout; nothing here imports it.

  maxmatch_dropout.json  {"texts_ref", "vocab_case", "rows", "cases": [{"probability", "drop_below", "seed", "epoch", "tokens"}]}
                         tokens[j] = the model's tokens of sentence rows[j] of ref/data/pan_tadeusz.json under the vocabulary of
                         naivewp.json's case `vocab_case`, sentence index j, for each of three (probability, seed, epoch).

Usage: python tests/golden/make_golden_maxmatch_dropout.py   (from the repository root; needs the built library for the split)
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

ROWS = list(range(0, 200, 10))  # twenty sentences
CASES = [(0.1, 0, 0), (0.5, (1 << 63) + 12345, 7), (0.02, 3, 0xFFFFFFFF)]
VOCAB_CASE = "pan_tadeusz_pretrained"


def main():
    from subword_tokenizers_amd.tokenizers import SubwordTokenizer
    from tests import maxmatch_cases as M
    from tests.test_naive_wp_encode import naivewp_cases

    (vocab, pan), = [(v, t) for name, v, t, _ in naivewp_cases() if name == VOCAB_CASE]
    model, texts = M.Model(vocab), [pan[r] for r in ROWS]
    cases = []
    for p, seed, epoch in CASES:
        below = M.drop_below(p)
        cases.append({"probability": p, "drop_below": below, "seed": seed, "epoch": epoch,
                      "tokens": model.tokenize(SubwordTokenizer._split, texts, below, seed, epoch)})
    out = {"texts_ref": "ref/data/pan_tadeusz.json", "vocab_case": VOCAB_CASE, "rows": ROWS, "cases": cases}
    path = os.path.join(HERE, "maxmatch_dropout.json")
    with open(path, "w", encoding="utf-8") as f:
        json.dump(out, f, ensure_ascii=False, indent=0)
        f.write("\n")
    size = os.path.getsize(path)
    assert size < 100 * 1024, size
    print("%d sentences x %d cases, %d bytes" % (len(ROWS), len(CASES), size))


if __name__ == "__main__":
    main()
