#!/usr/bin/env python3
"""Golden strings for decoding, made by IMPORTING THE REFERENCE's recover_sentence (utils.py:141-154; build container only).

  recover_sentence.json
    "alphabet", "exhaustive"   the reference's string for every row of length 0..3 over the alphabet, in itertools.product order
                               (length 0 first): 2,955 strings
    "fuzz_alphabet", "fuzz"    2,000 seeded rows of up to 12 tokens over the wider alphabet (the specials' strings and "['UNK']"
                               among it): [[indices into fuzz_alphabet], string]
    "pan_tadeusz"              {"FastBPE", "FastWordPiece"}: the reference's string for each of the 989 recorded rows of
                               ref/data/pan_tadeusz.tokens.json

The alphabets are those of tests/decode_cases.py.  Usage: python tests/golden/make_golden_recover.py
"""
import itertools
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import dump  # noqa: E402
from decode_cases import ALPHABET, FUZZ_ALPHABET  # noqa: E402
from source.utils import recover_sentence  # noqa: E402


def main():
    exhaustive = [recover_sentence(list(row)) for n in range(4) for row in itertools.product(ALPHABET, repeat=n)]
    rng = random.Random(20261020)
    fuzz = []
    for _ in range(2000):
        row = [rng.randrange(len(FUZZ_ALPHABET)) for _ in range(rng.randint(0, 12))]
        fuzz.append([row, recover_sentence([FUZZ_ALPHABET[i] for i in row])])
    with open(os.path.join(HERE, "ref", "data", "pan_tadeusz.tokens.json"), encoding="utf-8") as f:
        recorded = json.load(f)
    pan = {name: [recover_sentence(row) for row in rows] for name, rows in recorded.items()}
    dump("recover_sentence.json", {"alphabet": ALPHABET, "exhaustive": exhaustive, "fuzz_alphabet": FUZZ_ALPHABET, "fuzz": fuzz,
                                   "pan_tadeusz": pan})


if __name__ == "__main__":
    main()
