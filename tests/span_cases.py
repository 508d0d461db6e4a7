"""Inputs and expectations for the token-span kernel (csrc/swt_spans.hip).  No GPU and no library call: the split comes from
codepoint_cases.class_table() (the fixture), the spans from walking the tokens over it.  tests/test_span_cases.py checks what
is built here on the CPU, tests/test_gpu_spans.py runs it.

A token is described by (length in code points, continues its word); length 0 = the whole word (NaiveWP's "[UNK]").  The raw
ABI tests make ids for such tokens in either table convention of include/swt.h:
  flagged    len_base = SYM_BASE: a one-code-point token is its code point, a longer one SYM_BASE + length over the table
             [0, 1, 2, ...] (entry 0 = the whole word); continuation = bit 31 of the id
  unflagged  len_base = 0: id = 2 * length + continues over the table [0, CONT, 1, 1 | CONT, 2, ...]
so a token edge can be put anywhere."""
import random

import numpy as np

from tests import codepoint_cases as K

SYM_BASE = 0x110000
CONT = 0x80000000
OK, MISMATCH = 0, 1
MAX_LEN = 4096  # longest token the hand-made tables know
OFFSETS = K.OFFSETS


def word_spans(lowered):
    """[(start, end)] in code points: SubwordTokenizer.preprocessing's offsets (utils.py:27-29) from the class table alone"""
    tab = K.class_table()
    out, i, n = [], 0, len(lowered)
    while i < n:
        c = tab[ord(lowered[i])]
        if c & K.WS:
            i += 1
            continue
        j = i + 1
        if not c & K.PUNCT:
            while j < n and not tab[ord(lowered[j])] & (K.WS | K.PUNCT):
                j += 1
        out.append((i, j))
        i = j
    return out


def spans_from_lengths(lowered, toks):
    """toks = [(length, continues)] of one sentence -> ([(start, end)] in code points, [word index]), or None when the tokens do
    not tile the text (the five cases of include/swt.h; a token without a length is length None)"""
    words = word_spans(lowered)
    groups = []
    for length, cont in toks:
        if length is None:
            return None
        if not cont:
            groups.append([])
        elif not groups:
            return None
        groups[-1].append(length)
    if len(groups) != len(words):
        return None
    spans, wid = [], []
    for k, ((s, e), g) in enumerate(zip(words, groups)):
        if 0 in g:
            if len(g) != 1:
                return None
            g = [e - s]
        if sum(g) != e - s:
            return None
        for length in g:
            spans.append((s, s + length))
            wid.append(k)
            s += length
    return spans, wid


def token_body(tok):
    return tok[2:] if tok.startswith("##") and len(tok) > 2 else tok


def expected_spans(text, token_strings, unk=None):
    """text (lowercase already) and its tokens as strings -> ([(start, end)], [word index]) or None; a token covers the code
    points of its string after the '##', `unk` its whole word"""
    return spans_from_lengths(text, [(0, False) if tok == unk else (len(token_body(tok)), tok.startswith("##") and len(tok) > 2)
                                     for tok in token_strings])


def to_bytes(lowered, spans):
    """code-point spans -> byte spans of the sentence's UTF-8"""
    at = np.zeros(len(lowered) + 1, dtype=np.int64)
    np.cumsum([K.utf8_len(ord(c)) for c in lowered], out=at[1:])
    return [(int(at[s]), int(at[e])) for s, e in spans]


# ------------------------------------------------------------------------------------------------------ ids and tables

def length_table(flagged):
    if flagged:
        return np.arange(MAX_LEN + 1, dtype=np.uint32), SYM_BASE
    t = np.repeat(np.arange(MAX_LEN + 1, dtype=np.uint32), 2)
    t[1::2] |= CONT
    return t, 0


def make_ids(lowered, toks, flagged):
    """ids of one sentence's tokens [(length, continues)] in the given convention; a one-code-point token of the flagged
    convention is spelled by the code point it covers, so the text is needed"""
    if not flagged:
        return [2 * length + int(cont) for length, cont in toks]
    got = spans_from_lengths(lowered, toks)
    ids = []
    for i, (length, cont) in enumerate(toks):
        if length == 1 and got is not None:
            sym = ord(lowered[got[0][i][0]])
        else:
            sym = SYM_BASE + length
        ids.append(sym | (CONT if cont else 0))
    return ids


def segment(lowered, rng, mode=None):
    """a tiling of every word of the sentence: per word one of
      one      a single token of the word's length        whole    the zero-length token
      singles  one token per code point                   pairs    tokens of two code points (and a last one of one)
    chosen by rng, or `mode` for all"""
    toks = []
    for s, e in word_spans(lowered):
        m = mode or rng.choice(("one", "whole", "singles", "pairs"))
        n = e - s
        if n > MAX_LEN and m == "one":
            m = "pairs"
        if m == "one":
            sizes = [n]
        elif m == "whole":
            sizes = [0]
        elif m == "singles":
            sizes = [1] * n
        else:
            sizes = [2] * (n // 2) + [1] * (n % 2)
        toks += [(z, i > 0) for i, z in enumerate(sizes)]
    return toks


class Batch:
    """sentences (lowercase), their tokens, and what the kernel must say about them"""

    def __init__(self, name, texts, toks):
        self.name, self.texts, self.toks = name, texts, toks

    def packed(self, flagged):
        """-> (text uint8, sent_off, ids uint32, tok_off) of the raw ABI"""
        text, off = K.pack(self.texts)
        ids = [make_ids(t, k, flagged) for t, k in zip(self.texts, self.toks)]
        tok_off = np.zeros(len(ids) + 1, dtype=np.uint64)
        if ids:
            np.cumsum([len(x) for x in ids], out=tok_off[1:])
        flat = np.array([x for row in ids for x in row], dtype=np.uint32)
        return text, off, flat, tok_off

    def expected(self, codepoints=True):
        """-> (spans int64[n, 2], word int64[n], status uint8[n_sent]); a sentence that does not tile is all zeros"""
        spans, word, status = [], [], []
        for t, k in zip(self.texts, self.toks):
            got = spans_from_lengths(t, k)
            if got is None:
                spans += [(0, 0)] * len(k)
                word += [0] * len(k)
                status.append(MISMATCH)
            else:
                spans += got[0] if codepoints else to_bytes(t, got[0])
                word += got[1]
                status.append(OK)
        return (np.array(spans, dtype=np.int64).reshape(-1, 2), np.array(word, dtype=np.int64), np.array(status, dtype=np.uint8))


# ------------------------------------------------------------------------------------------------------------ the seams

ROLES = ("sentence", "word", "token", "whole")


def seam_characters():
    """one representative of each UTF-8 length and of each (class, length) pair of codepoint_cases P -> [(name, character)]"""
    out = [("letter1", "a"), ("bert_ws1", " "), ("bert_punct1", ".")]
    out += [("%s%d" % key, chr(cp)) for key, cp in sorted(K.representatives().items())]
    assert {K.utf8_len(ord(c)) for _, c in out} == {1, 2, 3, 4}
    return out


def seam_positions(block, chunk, tile):
    """the byte positions at which the kernel changes form, from swt_token_spans_capacity's numbers: the first two of each"""
    return sorted({block, 2 * block, chunk, 2 * chunk, tile, 2 * tile})


def _filler(n_bytes, rng):
    """short words, n_bytes exactly, ends with a space"""
    return K.fill(K.SHORT, n_bytes, rng) if n_bytes > 0 else ""


def _cut(text, rng):
    """sentences of up to about 40 bytes, cut behind spaces"""
    out, pos = [], 0
    while pos < len(text):
        i = text.find(" ", pos + rng.randint(8, 40)) + 1
        if i <= 0:
            i = len(text)
        out.append(text[pos:i])
        pos = i
    return out


def seam_batch(role, ch, d, positions, seed=0):
    """One batch with the lead byte of `ch` at every position + d of the batch's bytes, in one of four roles:
      sentence  first character of a sentence (short sentences in front: sentence starts on both sides of every tile seam)
      word      first character of a word                         )  all in ONE sentence from byte 0, so the position
      token     first character of a token inside a word          )  is also the distance from the sentence's first byte
      whole     last character of a word under a zero-length token)  (the block and chunk seams)
    What the character does to the split depends on its class; the expectation follows the class table either way.
    -> Batch, with the byte positions that were placed in .leads"""
    rng = random.Random("%s/%s/%d/%d" % (role, ch, d, seed))
    text, cur, leads, forced = "", 0, [], {}
    sents = []
    for p in positions:
        at = p + d
        front = {"sentence": 0, "word": 1, "token": 2, "whole": 3}[role]  # bytes of the placement in front of the character
        if at - front < cur:
            continue
        fill_bytes = at - front - cur
        piece = _filler(fill_bytes, rng)
        if role == "sentence":
            sents += _cut(piece, rng)
            sents.append(ch + "ab cd ")
            cur = at + K.nbytes(ch) + 6
        else:
            text += piece
            if role == "word":
                text += " " + ch + "ab "
            elif role == "token":
                text += "ab" + ch + "ab "
            else:
                text += " ab" + ch + " "
            cur = at + K.nbytes(ch) + {"word": 3, "token": 3, "whole": 1}[role]
        leads.append(at)
    if role == "sentence":
        sents += _cut(_filler(60, rng), rng)
        texts = sents
    else:
        texts = [text + _filler(100, rng)] + _cut(_filler(60, rng), rng)
    toks = []
    for t in texts:
        if role == "token":
            # tokens of two code points: "ab" + ch + "ab" is cut right in front of ch (when ch is a letter; otherwise ch is a
            # word start or dropped, and the expectation says so)
            toks.append(segment(t, rng, "pairs"))
        elif role == "whole":
            toks.append(segment(t, rng, "whole"))
        else:
            toks.append(segment(t, rng))
    b = Batch("%s-%+d" % (role, d), texts, toks)
    b.leads = leads
    return b


def long_word_batch(n=40000):
    """one word of n one-byte letters with 3- and 4-byte letters mixed in, as one-code-point tokens; short sentences around it"""
    l3, l4 = K.giant_letters()
    word = ("abcdefg" * 9 + l3 + "xyz" + l4) * (n // 70)
    texts = ["ab cd ", word, "cd ab. "]
    toks = [segment(texts[0], None, "pairs"), segment(word, None, "singles"), segment(texts[2], None, "one")]
    return Batch("long-word", texts, toks)


def punct_words_batch(n=40000):
    """n one-character punctuation words (one, two and three bytes) in one sentence; short sentences around it"""
    sent = (".,!?" * 4 + "«»" + "-" * 3 + "—") * (n // 22)
    texts = ["ab cd ", sent, "cd ab. "]
    toks = [segment(texts[0], None, "one"), segment(sent, None, "one"), segment(texts[2], None, "singles")]
    return Batch("punct-words", texts, toks)


def long_tokens_batch(chunk):
    """words longer than a chunk under one token, under two-code-point tokens and under the whole-word token"""
    rng = random.Random(7)
    texts = [K.giant(chunk + 300) + " ab " + K.giant(2 * chunk + 77) + ". " + "q" * (chunk + 5), "ab", K.giant(chunk + 1)]
    modes = ("one", "one", "whole", "pairs", "whole", "pairs")
    return Batch("long-tokens", texts * 2, [segment(t, rng, m) for t, m in zip(texts * 2, modes)])


# ------------------------------------------------------------------------------------------------------------ mismatches

def mismatch_batches():
    """[(case, Batch)]: one bad sentence of each kind of include/swt.h in the middle of good ones, short and longer than a block
    of 64 tokens (the sentence that is walked twice)"""
    rng = random.Random(5)
    good = ["ab cd. abcd ", "a", "dcab ba, cab ", "", "ab "]
    out = []
    for size in ("short", "long"):
        body = "ab cd abcd " if size == "short" else "ab cd abcd " * 40
        base = segment(body, rng, "singles")
        cases = {
            "more_groups": base + [(1, False)],
            "fewer_groups": base[:-4],
            "sum_short": base[:-1],
            "sum_long": base + [(1, True)],
            "sum_shifted": [(2, False)] + base[1:],
            "whole_with_company": [(0, False), (1, True)] + base[2:],
            "whole_as_continuation": base[:1] + [(0, True)] + base[2:],
            "first_continues": [(1, True)] + base[1:],
            "no_length": base[:3] + [(None, False)] + base[4:],
            "no_tokens": [],
        }
        for case, toks in cases.items():
            texts = good[:3] + [body] + good[3:]
            tk = [segment(t, rng) for t in good[:3]] + [toks] + [segment(t, rng) for t in good[3:]]
            out.append(("%s-%s" % (case, size), Batch(case, texts, tk)))
    return out


NO_LENGTH_ID = {True: SYM_BASE + MAX_LEN + 1, False: 2 * (MAX_LEN + 1)}  # the first id beyond each hand-made table


def packed_with_holes(batch, flagged):
    """Batch.packed for a batch whose tokens may have length None: those get the first id beyond the table"""
    fixed = [[(1, c) if z is None else (z, c) for z, c in k] for k in batch.toks]
    text, off, ids, tok_off = Batch(batch.name, batch.texts, fixed).packed(flagged)
    flat = [x for k in batch.toks for x in k]
    for i, (z, c) in enumerate(flat):
        if z is None:
            ids[i] = NO_LENGTH_ID[flagged] | (CONT if (c and flagged) else 0)
    return text, off, ids, tok_off
