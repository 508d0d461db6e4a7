#!/usr/bin/env python3
"""Golden vectors for sentence-pair batches, made with the `tokenizers` wheel (0.22.2) of the build container:
what the pair template, truncation with a strategy and a stride, and padding to a fixed length give there is what
swt_batch_pair_rows must give.

  pair_batches.json  {"tokenizers": version, "ids": {"pad", "unk", "cls", "sep", "first_a", "first_b"}, "n_max": 8,
                      "cases": {"width,stride,strategy,left,specials": [entry of (na, nb) = (0, 0), (0, 1), ... (8, 8)]},
                      "batch": {"width", "stride", "strategy", "lengths": [[na, nb], ...], "slots", "sample"}}
      a case: a pair of na and nb tokens -- token i of A has the id first_a + i, token j of B first_b + j -- through a WordLevel
              tokenizer with TemplateProcessing("[CLS] $A [SEP]", "[CLS] $A [SEP] $B:1 [SEP]:1") (specials 1; no post-processor
              with specials 0), enable_truncation(max_length=width, stride, strategy) and enable_padding(length=width,
              direction).  strategy: 0 longest_first, 1 only_first, 2 only_second.
      an entry: "E" where the wheel refuses the pair ("Sequence to truncate too short ...", or the panic "`stride` must be
              strictly less than `max_len` ..."; any other exception fails this script); otherwise the encoding and its
              overflowing encodings in order (k rows of `width`), two characters per slot:
                chr(40 + id) where the attention mask is 1, chr(80 + id) where it is 0 (every id is below 40), then
                chr(48 + type_id + 2 * special_tokens_mask + 4 * (sequence_id + 1)), sequence_id None counting as -1.
              The first `width` slots are what plain truncation gives.  longest_first is recorded with stride 0 and its first
              row only: its overflowing encodings are out of scope (include/swt.h).
      widths 6, 7, 8, 9 with right padding, 8 with left padding too; every stride 0 .. width - 4; width 5 without specials,
      strides 0 .. 4; na, nb = 0 .. 8.
      batch:  one encode_batch of pairs of `lengths`; sample[row] = the index of the row's pair.

Usage: python tests/golden/make_golden_pair_batches.py   (not run by the tests: the GPU machine needs no wheel)
"""
import json
import os

import tokenizers
from tokenizers import Tokenizer
from tokenizers.models import WordLevel
from tokenizers.pre_tokenizers import WhitespaceSplit
from tokenizers.processors import TemplateProcessing

HERE = os.path.dirname(os.path.abspath(__file__))
PAD, UNK, CLS, SEP, FIRST_A, FIRST_B = 0, 1, 2, 3, 10, 20
N_MAX = 8
STRATEGIES = ("longest_first", "only_first", "only_second")
REFUSALS = ("Sequence to truncate too short", "`stride` must be strictly less than `max_len")
BATCH_LENGTHS = [[0, 0], [2, 3], [3, 8], [0, 7], [4, 1], [1, 8], [3, 2], [2, 4], [0, 0], [2, 8]]


def make(width, stride, strategy, left, specials):
    vocab = {"[PAD]": PAD, "[UNK]": UNK, "[CLS]": CLS, "[SEP]": SEP}
    vocab.update(("a%d" % i, FIRST_A + i) for i in range(N_MAX + 1))
    vocab.update(("b%d" % i, FIRST_B + i) for i in range(N_MAX + 1))
    t = Tokenizer(WordLevel(vocab, unk_token="[UNK]"))
    t.pre_tokenizer = WhitespaceSplit()
    if specials:
        t.post_processor = TemplateProcessing(single="[CLS] $A [SEP]", pair="[CLS] $A [SEP] $B:1 [SEP]:1",
                                              special_tokens=[("[CLS]", CLS), ("[SEP]", SEP)])
    t.enable_truncation(max_length=width, stride=stride, strategy=STRATEGIES[strategy])
    t.enable_padding(length=width, pad_id=PAD, pad_token="[PAD]", direction="left" if left else "right")
    return t


def text(side, n):
    return " ".join("%s%d" % (side, i) for i in range(n))


def slots(enc, first_only=False):
    out = ""
    for r in [enc] + ([] if first_only else list(enc.overflowing)):
        for i, m, ty, sp, sq in zip(r.ids, r.attention_mask, r.type_ids, r.special_tokens_mask, r.sequence_ids):
            assert 0 <= i < 40 and m in (0, 1) and ty in (0, 1) and sp in (0, 1) and sq in (None, 0, 1)
            out += chr((40 if m else 80) + i) + chr(48 + ty + 2 * sp + 4 * ((-1 if sq is None else sq) + 1))
    return out


def entry(t, na, nb, first_only):
    try:
        return slots(t.encode(text("a", na), text("b", nb)), first_only)
    except BaseException as e:  # the stride refusal is a Rust panic: pyo3's PanicException derives from BaseException
        if isinstance(e, (KeyboardInterrupt, SystemExit)) or not any(r in str(e) for r in REFUSALS):
            raise
        return "E"


def main():
    cases = {}
    geometries = [(w, 0, 1) for w in (6, 7, 8, 9)] + [(8, 1, 1), (5, 0, 0)]
    for width, left, specials in geometries:
        cap = width - 3 * specials
        for strategy in range(3):
            for stride in range(1 if strategy == 0 else cap):
                t = make(width, stride, strategy, left, specials)
                cases["%d,%d,%d,%d,%d" % (width, stride, strategy, left, specials)] = [
                    entry(t, na, nb, strategy == 0) for na in range(N_MAX + 1) for nb in range(N_MAX + 1)]
    width, stride, strategy = 8, 1, 2
    t = make(width, stride, strategy, 0, 1)
    rows, sample = "", []
    for s, enc in enumerate(t.encode_batch([(text("a", na), text("b", nb)) for na, nb in BATCH_LENGTHS])):
        rows += slots(enc)
        sample += [s] * (1 + len(enc.overflowing))
    out = {"tokenizers": tokenizers.__version__,
           "ids": {"pad": PAD, "unk": UNK, "cls": CLS, "sep": SEP, "first_a": FIRST_A, "first_b": FIRST_B}, "n_max": N_MAX, "cases": cases,
           "batch": {"width": width, "stride": stride, "strategy": strategy, "lengths": BATCH_LENGTHS, "slots": rows, "sample": sample}}
    path = os.path.join(HERE, "pair_batches.json")
    with open(path, "w", encoding="utf-8") as f:
        json.dump(out, f, separators=(",", ":"))
    size = os.path.getsize(path)
    assert size < 512 * 1024, size
    print(path, (N_MAX + 1) ** 2 * len(cases), "cases", sum(e == "E" for c in cases.values() for e in c), "refused", size, "bytes")


if __name__ == "__main__":
    main()
