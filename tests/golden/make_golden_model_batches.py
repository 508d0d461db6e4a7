#!/usr/bin/env python3
"""Golden vectors for model-ready batches, made with the `tokenizers` wheel (0.22.2) of the build container: what
truncation with a stride, a [CLS] ... [SEP] template and padding to a fixed length give there is what swt_batch_rows must give.

  model_batches.json  {"tokenizers": version, "ids": {"pad", "unk", "cls", "sep", "first"},
                       "cases": {"width,stride,cls,sep,left": [slots of n = 0, slots of n = 1, ... n = 20]},
                       "batch": {"width", "stride", "cls", "sep", "left", "lengths", "slots", "sample"}}
      a case: a row of n tokens -- token i has the id first + i -- through a WordLevel tokenizer with
              TemplateProcessing (cls, sep: 0 / 1), enable_truncation(max_length=width, stride) and
              enable_padding(length=width, direction).  slots = the encoding and its overflowing encodings in order (k rows of
              `width`), one character per slot: chr(40 + id) where the attention mask is 1, chr(80 + id) where it is 0 (every id
              is below 40).  The first `width` slots are what plain truncation gives.
      widths 3, 4, 5, 8; every stride the wheel accepts (0 .. width - specials - 1); the four cls / sep combinations; both
      padding sides; n = 0 .. 20.
      batch:  one encode_batch of rows of `lengths` tokens; sample[row] = the index of the row's text.

Usage: python tests/golden/make_golden_model_batches.py   (not run by the tests: the GPU machine needs no wheel)
"""
import json
import os

import tokenizers
from tokenizers import Tokenizer
from tokenizers.models import WordLevel
from tokenizers.pre_tokenizers import WhitespaceSplit
from tokenizers.processors import TemplateProcessing

HERE = os.path.dirname(os.path.abspath(__file__))
PAD, UNK, CLS, SEP, FIRST = 0, 1, 2, 3, 10
N_MAX = 30
BATCH_LENGTHS = [0, 1, 5, 6, 7, 11, 12, 0, 30, 3, 13, 21]


def make(width, stride, cls, sep, left):
    vocab = {"[PAD]": PAD, "[UNK]": UNK, "[CLS]": CLS, "[SEP]": SEP}
    vocab.update(("t%d" % i, FIRST + i) for i in range(N_MAX))
    t = Tokenizer(WordLevel(vocab, unk_token="[UNK]"))
    t.pre_tokenizer = WhitespaceSplit()
    if cls or sep:
        single = " ".join((["[CLS]"] if cls else []) + ["$A"] + (["[SEP]"] if sep else []))
        t.post_processor = TemplateProcessing(single=single, special_tokens=[("[CLS]", CLS), ("[SEP]", SEP)])
    t.enable_truncation(max_length=width, stride=stride)
    t.enable_padding(length=width, pad_id=PAD, pad_token="[PAD]", direction="left" if left else "right")
    return t


def text(n):
    return " ".join("t%d" % i for i in range(n))


def slots(enc):
    out = ""
    for r in [enc] + list(enc.overflowing):
        assert all(0 <= i < 40 and m in (0, 1) for i, m in zip(r.ids, r.attention_mask))
        out += "".join(chr((40 if m else 80) + i) for i, m in zip(r.ids, r.attention_mask))
    return out


def main():
    cases = {}
    for width in (3, 4, 5, 8):
        for cls in (0, 1):
            for sep in (0, 1):
                for stride in range(width - cls - sep):
                    for left in (0, 1):
                        t = make(width, stride, cls, sep, left)
                        cases["%d,%d,%d,%d,%d" % (width, stride, cls, sep, left)] = [slots(t.encode(text(n))) for n in range(21)]
    width, stride, cls, sep, left = 8, 2, 1, 1, 0
    t = make(width, stride, cls, sep, left)
    rows, sample = "", []
    for s, enc in enumerate(t.encode_batch([text(n) for n in BATCH_LENGTHS])):
        rows += slots(enc)
        sample += [s] * (1 + len(enc.overflowing))
    out = {"tokenizers": tokenizers.__version__, "ids": {"pad": PAD, "unk": UNK, "cls": CLS, "sep": SEP, "first": FIRST}, "cases": cases,
           "batch": {"width": width, "stride": stride, "cls": cls, "sep": sep, "left": left, "lengths": BATCH_LENGTHS, "slots": rows,
                     "sample": sample}}
    path = os.path.join(HERE, "model_batches.json")
    with open(path, "w", encoding="utf-8") as f:
        json.dump(out, f, separators=(",", ":"))
    print(path, 21 * len(cases), "cases", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
