#!/usr/bin/env python3
"""Golden vectors for FastWP token spans, made by IMPORTING THE REFERENCE (build container only).

  fastwp_spans.json  {"pan": {"texts_ref", "n", "rows"}, "fuzz": {"alphabet", "vocab", "rows", "dropped", "counts"}}
                     rows[i] = {"text", "tokens", "spans", "word"}: FastWP.tokenize(text) (wordpiece.py:233-270), the
                     (start, end) of every token in code points of text.lower(), flattened, and the index of its segment
                     among those of the sentence that emit a token.

The reference returns no positions.  They are derived here from what its own matchloop returns: matchloop is wrapped ON THE
INSTANCE to record (i0, tokens, node, i1) of every pass of the loop at wordpiece.py:251 while the reference's own tokenize runs,
and the spans follow by this rule, checked on every row against the text (the tiling assertions below):
  valid segment    its tokens cover a prefix of s[i0:i1] one after the other; the first covers len(token) code points, every
                   later one (it begins with '##') len(token) - 2.  The prefix may be shorter than i1 - i0 (utils.py:136-137
                   drops the path of a redirected failure link): a short cover.
  invalid segment  the one "['UNK']" covers (i0, b), b the first iswdbndry position at or after i1 (the reference's own
                   iswdbndry)
  the '##' corner  every token of NaiveWP.encode_word("##") covers (i0, i0 + 2)
  word index       the segments that emit at least one token, numbered from 0

  pan:  the first 200 sentences of ref/data/pan_tadeusz.json, the pretrained vocabulary.
  fuzz: 400 seeded strings of 0..24 characters over a closed alphabet and a handmade vocabulary (both stored), then hand cases.
        Every character that can occur after .lower() is a plain single-character token, so every segment moves on and the
        reference terminates; 'q' and the 4-byte character have no '##' form, so inside a word they make "['UNK']"; 'a.b', 'x-y'
        and '.q' make short covers and segments that end behind a static boundary.  Every call runs under an alarm; a dropped row
        is counted (cap: 10 %).

Same shim recipe as make_golden.py.  Usage: python tests/golden/make_golden_fastwp_spans.py
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")
sys.path.insert(0, HERE)
from make_golden import Timeout, dump, make_shim, with_alarm  # noqa: E402

N_PAN, N_FUZZ = 200, 400
UNK = "['UNK']"
LETTERS = list("abxyingkmz") + ["q", "ξ"]  # 'q' has no '##q'
DIGITS = list("52")
PUNCT = [".", "-", "#", "×"]
SPACES = [" ", " ", " ", "\t", " ", "　"]
CAPITALS = ["A", "B", "X", "İ"]  # 'İ'.lower() is 'i' + U+0307
WIDE = ["\U0001F600"]  # four bytes, no '##' form
ALPHABET = LETTERS + DIGITS + PUNCT + SPACES[2:] + CAPITALS + WIDE
SINGLES = LETTERS + DIGITS + PUNCT + ["̇"] + WIDE
VOCAB = sorted(set(
    SINGLES + ["##" + c for c in LETTERS + DIGITS if c != "q"] + ["##"]
    # '##.' and '##-' give the nodes 'a.' and 'x-' a failure link to lose: with them "a. " keeps the pop 'a' and drops the '.'
    + ["##.", "##-"]
    + ["a.b", "x-y", ".q", "##ing", "5×2km", "ab", "##ba", "xyx", "ing", "##ng", "km", "##km"]))
HAND = ["x- y", "ab##ing", "zzξ.a", "x-yx", "x-yq", "a. ", "a.", " a", "　 a b", ".", ". .q", "##", "## a", "a ##", "a##",
        "İ", "İİx", "5×2km", "5×2k", "5×2kmq", "##ing", "a.b", "a.bq", "a.ba", ".q", "q.q", "aq", "qa",
        "\U0001F600", "a\U0001F600", "\U0001F600a", "", " ", "\t ", "AB X-Y", "xingq-a.b ##ing"]


def fuzz(rng):
    out = []
    for k in range(N_FUZZ):
        n = rng.randint(0, 24)
        pool = LETTERS * 3 + DIGITS + PUNCT * 2 + SPACES * 2 + CAPITALS + WIDE
        s = "".join(rng.choice(pool) for _ in range(n))
        # one string in four gets a vocabulary entry that runs through punctuation dropped into it
        if k % 4 == 0 and n:
            at = rng.randrange(n)
            s = (s[:at] + rng.choice(["a.b", "x-y", ".q", "##ing", "5×2km", "##"]) + s[at:])[:24]
        out.append(s)
    return out


def row_of(wp, corner, text, counts):
    """FastWP.tokenize(text) by the reference, with spans and word indices by the rule of the module docstring."""
    seen = []
    orig = type(wp).matchloop

    def recording(seq, i):
        tokens, node, i1 = orig(wp, seq, i)
        seen.append((i, list(tokens), node, i1))
        return tokens, node, i1

    wp.matchloop = recording  # on the instance: tokenize's self.matchloop finds it first
    try:
        out = wp.tokenize(text)
    finally:
        del wp.matchloop
    s = text.lower() + " "
    trie = wp.vocab_trie
    roots = (trie.root, trie.root_sharp, trie.root_p)
    spans, word, k, nw = [], [], 0, 0
    for n_seg, (i0, tokens, node, i1) in enumerate(seen):
        if not wp.iswdbndry(s, i1) or not any(node is r for r in roots):
            assert out[k] == UNK, (text, k)
            b = i1
            while not wp.iswdbndry(s, b):
                b += 1
            assert i0 < b <= len(text.lower()), (text, i0, b)
            spans += [i0, b]
            word.append(nw)
            k += 1
            nw += 1
            counts["unk"] += 1
            if any(wp.iswdbndry(s, j) for j in range(i0 + 1, b)):
                counts["unk_behind_boundary"] += 1
        elif node is trie.root_sharp and not tokens:
            assert out[k:k + len(corner)] == corner and s[i0:i0 + 2] == "##", (text, k)
            for _ in corner:
                spans += [i0, i0 + 2]
                word.append(nw)
            k += len(corner)
            nw += 1
            counts["corner"] += 1
        else:
            assert out[k:k + len(tokens)] == tokens, (text, k)
            p = i0
            for j, tok in enumerate(tokens):
                body = tok[2:] if j else tok
                assert j == 0 or tok.startswith("##"), (text, tok)
                assert s[p:p + len(body)] == body and p + len(body) <= i1, (text, tok, p)  # the tiling
                spans += [p, p + len(body)]
                word.append(nw)
                p += len(body)
            k += len(tokens)
            if tokens:
                nw += 1
                if p < i1:
                    counts["short_cover"] += 1
                if len(tokens) > 1:
                    counts["multi_token"] += 1
            else:
                counts["empty_segment"] += 1
                if n_seg == 0:
                    counts["empty_leading"] += 1
    assert k == len(out), (text, k, len(out))
    return {"text": text, "tokens": out, "spans": spans, "word": word}


def rows_of(wp, corner, texts, counts):
    rows, dropped = [], 0
    for t in texts:
        try:
            rows.append(with_alarm(lambda: row_of(wp, corner, t, counts), 1.0 + len(t) * 0.01))
        except Timeout:
            dropped += 1
    return rows, dropped


def new_counts():
    return {"unk": 0, "unk_behind_boundary": 0, "corner": 0, "short_cover": 0, "multi_token": 0, "empty_segment": 0, "empty_leading": 0}


def main():
    import source.utils as U
    import source.wordpiece as W

    shim = make_shim()
    ref = os.path.join(HERE, "ref")

    wp = W.FastWP(shim)
    wp.load_resources(os.path.join(ref, "resources/pretrained/FastWordPiece"))
    try:
        corner = with_alarm(lambda: W.NaiveWP.encode_word(wp, "##"), 2.0)
    except Timeout:  # the reference never returns from the corner with this vocabulary, nor from a text that reaches it
        corner = None
    pan = json.load(open(os.path.join(ref, "data/pan_tadeusz.json"), encoding="utf-8"))[:N_PAN]
    c_pan = new_counts()
    rows, dropped = rows_of(wp, corner, pan, c_pan)
    assert dropped == 0 and len(rows) == N_PAN, "the reference timed out on a pan_tadeusz sentence"
    out = {"pan": {"texts_ref": "ref/data/pan_tadeusz.json", "n": N_PAN, "counts": c_pan,
                   "rows": [{k: v for k, v in r.items() if k != "text"} for r in rows]}}

    fz = W.FastWP(shim)
    fz.vocab = set(VOCAB)
    fz.vocab_trie = U.WPTrie_E2E(VOCAB)
    corner = with_alarm(lambda: W.NaiveWP.encode_word(fz, "##"), 2.0)
    texts = fuzz(random.Random(20250311)) + HAND
    for t in texts:  # the closed alphabet: nothing but single-character tokens and white space after lower()
        assert all(c in fz.vocab or c.isspace() for c in t.lower()), t
    c_fz = new_counts()
    rows, dropped = rows_of(fz, corner, texts, c_fz)
    assert dropped * 10 <= len(texts), "more than 10 %% of the fuzz inputs timed out (%d of %d)" % (dropped, len(texts))
    for need in ("unk", "short_cover", "corner", "empty_leading", "unk_behind_boundary"):
        assert c_fz[need] > 0, need
    out["fuzz"] = {"alphabet": ALPHABET, "vocab": VOCAB, "rows": rows, "dropped": dropped, "counts": c_fz}
    dump("fastwp_spans.json", out)
    size = os.path.getsize(os.path.join(HERE, "fastwp_spans.json"))
    assert size < 300 * 1024, size
    print("pan %s\nfuzz %d rows, %d dropped, %s\n%d bytes" % (c_pan, len(rows), dropped, c_fz, size))


if __name__ == "__main__":
    main()
