#!/usr/bin/env python3
"""Golden vectors for token spans, made by IMPORTING THE REFERENCE (build container only).

  spans.json  {"pan": {"texts_ref", "n", "offsets", "FastBPE", "NaiveWP"}, "fuzz": {"texts", "offsets", "FastBPE", "NaiveWP",
               "dropped"}}
              offsets[i] = SubwordTokenizer.preprocessing's (start, end) of every word of text i, flattened (utils.py:15-29:
              code points of text.lower()); MODEL[i] = the model's tokens of text i, one list per word (encode_word of the
              preprocessing words, which is what tokenize concatenates: bpe.py:245-249, wordpiece.py:160-179).
              pan:  the first 200 sentences of ref/data/pan_tadeusz.json; FastBPE with the pretrained merges, NaiveWP with the
                    pretrained vocabulary.
              fuzz: seeded sentences over Polish letters, digits, ASCII and other punctuation, multi-byte White_Space, 4-byte
                    code points, 'İ' and combining marks; FastBPE with the pretrained merges, NaiveWP with the tutorial
                    vocabulary (resources/tests: it holds no '#', so out-of-vocabulary words become "[UNK]").  Every NaiveWP
                    call runs under an alarm; a sentence on which it does not return is dropped ("dropped" counts them).

Same shim recipe as make_golden.py.  Usage: python tests/golden/make_golden_spans.py
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")
sys.path.insert(0, HERE)
from make_golden import Timeout, dump, make_shim, with_alarm  # noqa: E402

N_PAN, N_FUZZ = 200, 110
LETTERS = list("aąbcćdeęfghijklłmnńoóprsśtuwyzźż") + list("ĄĆĘŁŃÓŚŹŻABC")
TUTORIAL = list("exampleaistexam.")
DIGITS = list("0123456789")
PUNCT = list(".,;:!?-()\"'") + list("«»—")
SPACES = [" ", " ", " ", "\t", "\u00a0", "\u2028", "\u3000"]
WIDE = ["\U0001F600", "\U00010400", "\U00010428", "\U0001D7D8"]
MARKS = ["\u0130", "\u0301", "\u0307", "\u0328"]  # 'İ' and three combining marks


def fuzz(rng):
    out = []
    for k in range(N_FUZZ):
        words = []
        for _ in range(rng.randint(1, 9)):
            # four words in ten over the tutorial vocabulary's own letters, so that NaiveWP yields more than "[UNK]"
            pool = TUTORIAL if rng.random() < 0.4 else LETTERS * 6 + DIGITS + PUNCT + WIDE + MARKS
            words.append("".join(rng.choice(pool) for _ in range(rng.randint(1, 9))))
        s = ""
        for w in words:
            s += w + "".join(rng.choice(SPACES) for _ in range(rng.randint(0, 2) or 1))
        out.append(s if k % 5 else rng.choice(SPACES) + s)
    out += ["İstanbul x€y", "", " ", "　 ", "!", "a"]
    return out


def main():
    import source.bpe as B
    import source.wordpiece as W

    shim = make_shim()
    ref = os.path.join(HERE, "ref")
    bpe = B.FastBPE(shim)
    bpe.load_resources(os.path.join(ref, "resources/pretrained/FastBPE"))
    wp_pre, wp_tut = W.NaiveWP(shim), W.NaiveWP(shim)
    wp_pre.vocab = set(json.load(open(os.path.join(ref, "resources/pretrained/FastWordPiece/vocab.json"), encoding="utf-8")))
    wp_tut.vocab = set(json.load(open(os.path.join(ref, "resources/tests/FastWordPiece/vocab.json"), encoding="utf-8")))
    assert not any("#" in t[2:] if t.startswith("##") else "#" in t for t in wp_tut.vocab)  # no '#' of its own: no endless loop

    def rows(texts, wp):
        """-> kept texts, offsets, FastBPE tokens per word, NaiveWP tokens per word, dropped"""
        kept, offsets, t_bpe, t_wp, dropped = [], [], [], [], 0
        for s in texts:
            pre = bpe.preprocessing([s])[0]
            try:
                per_word = with_alarm(lambda: [wp.encode_word(w) for w, _ in pre], 1.0 + len(s) * 0.01)
                assert [t for ws in per_word for t in ws] == with_alarm(lambda: wp.tokenize(s), 1.0 + len(s) * 0.01)
            except Timeout:
                dropped += 1
                continue
            b_words = [bpe.encode_word(w) for w, _ in pre]
            assert [t for ws in b_words for t in ws] == bpe.tokenize(s)
            kept.append(s)
            offsets.append([x for _, se in pre for x in se])
            t_bpe.append(b_words)
            t_wp.append(per_word)
        return kept, offsets, t_bpe, t_wp, dropped

    pan = json.load(open(os.path.join(ref, "data/pan_tadeusz.json"), encoding="utf-8"))[:N_PAN]
    kept, off, tb, tw, dropped = rows(pan, wp_pre)
    assert kept == pan and dropped == 0, "the reference timed out on a pan_tadeusz sentence"
    out = {"pan": {"texts_ref": "ref/data/pan_tadeusz.json", "n": N_PAN, "offsets": off, "FastBPE": tb, "NaiveWP": tw}}
    texts = fuzz(random.Random(20240917))
    kept, off, tb, tw, dropped = rows(texts, wp_tut)
    assert dropped * 10 <= len(texts), "more than 10 %% of the fuzz inputs timed out (%d of %d)" % (dropped, len(texts))
    assert any("[UNK]" in ws for row in tw for ws in row)
    out["fuzz"] = {"texts": kept, "offsets": off, "FastBPE": tb, "NaiveWP": tw, "dropped": dropped}
    dump("spans.json", out)
    size = os.path.getsize(os.path.join(HERE, "spans.json"))
    assert size < 300 * 1024, size
    print("pan %d, fuzz %d kept, %d dropped, %d bytes" % (N_PAN, len(kept), dropped, size))


if __name__ == "__main__":
    main()
