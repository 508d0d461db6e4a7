"""Inputs that send every code point, and every (class, UTF-8 length) pair at every seam, through the device code that decodes a
character, classifies it and spreads the class over its continuation bytes.  Inputs only: no GPU, fixed seeds, nothing read outside
the repository.  tests/test_codepoint_cases.py checks what is built here on the CPU, tests/test_gpu_codepoints.py runs it.

Everything is well-formed UTF-8 as the library itself produces it: a Python str encoded with `surrogatepass`, as
_native.join_texts does.  Malformed byte strings through the raw C ABI are out of scope.

  S1   "ab" + chr(cp) + "ab" for every cp in U+0001 .. U+10FFFF, surrogates included.  U+0000 is left out (a text that holds it
       goes by code-point lengths); NUL has the small batch for swt_utf8_prepare.
  S16  "a" + "a".join(sixteen consecutive code points) + "a": 69,632 sentences (the first starts at U+0001); every character's
       byte alignment differs from S1's.
  E    the code points at which something changes: both sides of every range edge of the four classes, every source and target
       of the lowercase pairs, the 26 code points left to the host, the UTF-8 length edges, the LDS cut-off, the surrogate edges.
  P    one representative of every (class, UTF-8 length) pair of the fixtures, its lead byte at every offset from 4 bytes before
       to 1 byte after every seam of the kernels, among short words and inside a word longer than any chunk.

The classes and the lowercase mapping come from tests/golden/unicode_classes.json and tests/golden/unicode_lower.json alone; the
26 host code points are never lowered here (lower() leaves them as they are), so nothing depends on this interpreter's
str.lower()."""
import functools
import json
import os
import random
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CSRC = os.path.join(ROOT, "subword-tokenizers_amd", "csrc")

N_CP = 0x110000
CONT = 0x80000000
WS, PUNCT, SPACE, ALNUM = 1, 2, 4, 8
CLASS_NAMES = (("bert_ws", WS), ("bert_punct", PUNCT), ("py_space", SPACE), ("py_alnum", ALNUM))


@functools.lru_cache(maxsize=None)
def fixture(name):
    with open(os.path.join(GOLDEN, name), encoding="utf-8") as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def class_table():
    """uint8[0x110000]: WS | PUNCT | SPACE | ALNUM of every code point, from the fixture's ranges"""
    t = np.zeros(N_CP, dtype=np.uint8)
    fx = fixture("unicode_classes.json")
    for name, bit in CLASS_NAMES:
        for lo, hi in fx[name]:
            t[lo:hi + 1] |= bit
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def lower_table():
    """uint32[0x110000]: the lowercase of every code point by the fixture's pairs; the host code points map to themselves"""
    t = np.arange(N_CP, dtype=np.uint32)
    for src, dst in fixture("unicode_lower.json")["pairs"]:
        t[src] = dst
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def host_cps():
    return frozenset(fixture("unicode_lower.json")["host"])


@functools.lru_cache(maxsize=None)
def _translation():
    return {src: dst for src, dst in fixture("unicode_lower.json")["pairs"]}


def lower(text):
    """the fixture's lowercase of a text; a host code point stays as it is"""
    return text.translate(_translation())


def utf8(text):
    return text.encode("utf-8", "surrogatepass")


def nbytes(text):
    return len(utf8(text))


def utf8_len(cp):
    return 1 if cp < 0x80 else 2 if cp < 0x800 else 3 if cp < 0x10000 else 4


def pack(texts):
    """list[str] -> (uint8 bytes, uint64 offsets[n + 1]), surrogatepass"""
    enc = [utf8(t) for t in texts]
    off = np.zeros(len(enc) + 1, dtype=np.uint64)
    if enc:
        np.cumsum(np.fromiter(map(len, enc), dtype=np.uint64, count=len(enc)), out=off[1:])
    buf = np.frombuffer(b"".join(enc), dtype=np.uint8)
    if buf.size == 0:
        buf = np.zeros(1, dtype=np.uint8)[:0]
    return buf, off


def join(texts):
    """the separator form: one zero byte between neighbours"""
    return np.frombuffer(utf8("\x00".join(texts)), dtype=np.uint8)


def split_words(lowered):
    """the BERT pre-tokenizer's words of one lowercase sentence, from the class table alone (utils.py:27)"""
    tab = class_table()
    words, i, n = [], 0, len(lowered)
    while i < n:
        c = tab[ord(lowered[i])]
        if c & WS:
            i += 1
            continue
        j = i + 1
        if not c & PUNCT:
            while j < n and not tab[ord(lowered[j])] & (WS | PUNCT):
                j += 1
        words.append(lowered[i:j])
        i = j
    return words


def has_host(text):
    h = host_cps()
    return any(ord(c) in h for c in text)


# ------------------------------------------------------------------------------------------------------------ the sweeps

@functools.lru_cache(maxsize=None)
def s1():
    return ["ab" + chr(cp) + "ab" for cp in range(1, N_CP)]


def s1_cp(i):
    """the code point of sentence i of S1"""
    return i + 1


@functools.lru_cache(maxsize=None)
def s16():
    return ["a" + "a".join(map(chr, range(max(b, 1), b + 16))) + "a" for b in range(0, N_CP, 16)]


@functools.lru_cache(maxsize=None)
def nul_batch():
    """texts with U+0000 inside, at the start and at the end, beside multi-byte characters and a cased 4-byte letter: the
    code-point form (swt_utf8_prepare) is the only one that takes them"""
    reps = representatives()
    out = []
    for (_kind, _n), cp in sorted(reps.items()):
        c = chr(cp)
        out += ["\x00", "A\x00" + c, c + "\x00B", "\x00" + c + "\x00", "", c + "A" + c + "\x00\x00" + c]
    return out


@functools.lru_cache(maxsize=None)
def edge_set():
    fx = fixture("unicode_classes.json")
    lw = fixture("unicode_lower.json")
    e = set()
    for name, _bit in CLASS_NAMES:
        for lo, hi in fx[name]:
            e.update((lo - 1, lo, hi, hi + 1))
    for src, dst in lw["pairs"]:
        e.update((src, dst))
    e.update(lw["host"])
    e.update((0x7F, 0x80, 0x7FF, 0x800, 0xFFFF, 0x10000, 0x10FFFF, 0x3FF, 0x400, 0xD7FF, 0xD800, 0xDFFF, 0xE000))
    return tuple(sorted(c for c in e if 1 <= c < N_CP))


KINDS = ("letter", "cased", "bert_ws", "bert_punct", "py_space")


def kind_member(kind, cp):
    """does cp belong to a kind of the position family (by the fixtures alone)"""
    c = int(class_table()[cp])
    if kind == "letter":
        return c == ALNUM and int(lower_table()[cp]) == cp and cp not in host_cps()
    if kind == "cased":
        return c == ALNUM and int(lower_table()[cp]) != cp
    if kind == "bert_ws":
        return bool(c & WS)
    if kind == "bert_punct":
        return bool(c & PUNCT)
    return bool(c & SPACE)


@functools.lru_cache(maxsize=None)
def kind_lengths():
    """every (kind, UTF-8 length >= 2) pair the fixtures hold -> its first code point"""
    tab, low = class_table(), lower_table()
    cps = np.arange(N_CP)
    sur = (cps >= 0xD800) & (cps <= 0xDFFF)
    host = np.zeros(N_CP, dtype=bool)
    host[list(host_cps())] = True
    member = {"letter": (tab == ALNUM) & (low == cps) & ~host, "cased": (tab == ALNUM) & (low != cps),
              "bert_ws": (tab & WS) != 0, "bert_punct": (tab & PUNCT) != 0, "py_space": (tab & SPACE) != 0}
    out = {}
    for kind in KINDS:
        for n, (lo, hi) in ((2, (0x80, 0x800)), (3, (0x800, 0x10000)), (4, (0x10000, N_CP))):
            idx = np.flatnonzero(member[kind][lo:hi] & ~sur[lo:hi])
            if idx.size:
                out[(kind, n)] = lo + int(idx[0])
    return out


def representatives():
    """kind_lengths() without the pairs whose code point an earlier pair has already (the first py_space characters of two and
    three bytes are the bert_ws ones)"""
    out, seen = {}, set()
    for key, cp in kind_lengths().items():
        if cp not in seen:
            out[key] = cp
            seen.add(cp)
    return out


# ------------------------------------------------------------------------------------------------------------ the seams

def _const(src, pattern):
    return int(re.search(pattern, src).group(1))


@functools.lru_cache(maxsize=None)
def constants():
    """the kernels' own limits, read from their sources"""
    def read(name):
        with open(os.path.join(CSRC, name), encoding="utf-8") as f:
            return f.read()
    bpe, dd, words, wp, low = (read(n) for n in ("swt_bpe_encode.hip", "swt_dedup.hip", "swt_words.hip", "swt_wp.hip", "swt_lower.hip"))
    return {"SWT_LANE_CAP": _const(bpe, r"#define SWT_LANE_CAP (\d+)"), "SWT_LANE_TILE": _const(bpe, r"#define SWT_LANE_TILE (\d+)"),
            "kDCap": _const(dd, r"#define SWT_DCAP (\d+)"), "kDTile": _const(dd, r"#define SWT_DTILE (\d+)"),
            "kClsLds": _const(dd, r"\bkClsLds = (\d+)\b"), "kWCap": _const(words, r"\bkWCap = (\d+)\b"),
            "kWTile": _const(words, r"\bkWTile = (\d+)\b"), "kWpCap": _const(wp, r"\bkWpCap = (\d+)\b"),
            "kWpTile": _const(wp, r"\bkWpTile = (\d+)\b"), "kWpClsLds": _const(wp, r"\bkWpClsLds = (\d+)\b"),
            "kOffBlock": _const(low, r"\bkOffBlock = (\d+)\b"),
            "kDirectBytes": _const(bpe, r"\bkDirectBytes = (\d+)\b"), "kDirectSents": _const(bpe, r"\bkDirectSents = (\d+)\b"),
            "kWpDirectBytes": _const(wp, r"\bkWpDirectBytes = (\d+)\b"), "kWpDirectSents": _const(wp, r"\bkWpDirectSents = (\d+)\b")}


# what this file was written against; test_codepoint_cases.py asserts that constants() still says so
EXPECTED_CONSTANTS = {"SWT_LANE_CAP": 512, "SWT_LANE_TILE": 384, "kDCap": 1536, "kDTile": 1024, "kClsLds": 1024, "kWCap": 1024,
                      "kWTile": 512, "kWpCap": 1024, "kWpTile": 512, "kWpClsLds": 1024, "kOffBlock": 1024,
                      "kDirectBytes": 1024, "kDirectSents": 64, "kWpDirectBytes": 2048, "kWpDirectSents": 64}

OFFSETS = (-4, -3, -2, -1, 0, 1)  # the lead byte against the seam
LEVEL2 = 1024 * 1024              # 1,024 blocks of kOffBlock: the second level of the scan in swt_lower.hip


@functools.lru_cache(maxsize=None)
def seams():
    """name -> byte position in a batch whose first chunk starts at byte 0 (every chunk starts at a multiple of 16 of the batch,
    the first at 0; tiles and the 1-KiB blocks are counted from the batch's first byte)"""
    k = EXPECTED_CONSTANTS
    return {"group16": 16, "block64": 64, "SWT_LANE_TILE": k["SWT_LANE_TILE"], "SWT_LANE_CAP": k["SWT_LANE_CAP"],
            "kWTile": k["kWTile"], "kWCap": k["kWCap"], "kDTile": k["kDTile"], "kDCap": k["kDCap"], "kOffBlock": k["kOffBlock"]}


def seam_positions():
    return tuple(sorted(set(seams().values())))


SHORT = ("ab", "abc", "cd", "abcd", "ba", "dcab", "a", "cab")  # lowercase ASCII: the merges of the tests' tables apply to them
GIANT_TAIL = 1700                                               # bytes of long word behind the character: more than any chunk


def fill(words, n_bytes, rng):
    """words separated by single spaces, n_bytes of UTF-8 exactly (ends with a space; 'q' runs make up the remainder)"""
    out = []
    left = n_bytes
    while left > 0:
        w = rng.choice(words)
        b = nbytes(w) + 1
        if b > left:
            w = "q" * (left - 1)
            b = left
        out.append(w)
        left -= b
    return " ".join(out) + " " if out else ""


def giant_letters():
    """the 3- and the 4-byte letter that long words are made of"""
    reps = representatives()
    return chr(reps[("letter", 3)]), chr(reps[("letter", 4)])


def giant(n_bytes):
    """one word of exactly n_bytes (>= 6) of 3- and 4-byte letters, one to three ASCII letters making up the remainder"""
    l3, l4 = giant_letters()
    k, r = divmod(n_bytes, 7)
    return (l3 + l4) * k + ("", "b", "bb", l3, l4, l4 + "b", l3 + l3)[r]


class Placement:
    """one batch of P: its sentences, and where the character's lead byte lies in the batch's bytes (no separators counted)"""

    def __init__(self, kind, length, cp, surrounding, layout, offset, texts, leads):
        self.kind, self.length, self.cp, self.surrounding, self.layout, self.offset = kind, length, cp, surrounding, layout, offset
        self.texts, self.leads = texts, leads
        self.name = "%s%d-%s-%s%+d" % (kind, length, surrounding, layout, offset)


def _cut(text, every, rng):
    """sentences of about `every` bytes, cut behind spaces (a text without spaces stays whole)"""
    sents, pos = [], 0
    while pos < len(text):
        i = text.find(" ", pos + rng.randint(every // 2, every)) + 1
        if i <= 0:
            i = len(text)
        sents.append(text[pos:i])
        pos = i
    return sents


def _short_text(ch, targets, d, rng, tail=40):
    """short words; `ch` between two letters with its lead byte at every target + d"""
    text, leads, cur = "", [], 0
    for t in targets:
        at = t + d
        if at - cur < 3:
            continue
        piece = fill(SHORT, at - cur - 2, rng) + "ab"
        text += piece + ch + "ab "
        leads.append(at)
        cur = at + nbytes(ch) + 3
    text += fill(SHORT, tail, rng)
    return text, leads


@functools.lru_cache(maxsize=None)
def position_family():
    """the batches of P.  Three layouts:
      sentences  short words in short sentences, the character at every seam position + offset: sentence starts on both sides of
                 every tile boundary, no sentence longer than a chunk
      long       the same text as ONE sentence (and a few short ones behind it): every chunk is cut at a word boundary, and the
                 staged end of the first chunk of each kernel lies at its Cap
      giant      one placement per batch: a word of 3- and 4-byte letters from byte 0 to the character, and GIANT_TAIL bytes of it
                 behind: at a Cap seam both sides are longer than the chunk, so the one-lane walks over global memory run"""
    rng = random.Random(110000)
    reps = representatives()
    pos = seam_positions()
    out = []
    for (kind, length), cp in sorted(reps.items()):
        ch = chr(cp)
        for d in OFFSETS:
            text, leads = _short_text(ch, pos, d, rng)
            out.append(Placement(kind, length, cp, "short", "sentences", d, _cut(text, 48, rng), leads))
            text, leads = _short_text(ch, pos, d, rng, tail=200)
            out.append(Placement(kind, length, cp, "short", "long", d, [text] + [fill(SHORT, 30, rng) for _ in range(3)], leads))
            for t in pos:
                at = t + d
                head = giant(at) if at >= 12 else "b" * at
                text = head + ch + giant(GIANT_TAIL)
                p = Placement(kind, length, cp, "giant", "giant", d, [text, "ab cd "], [at])
                p.name += "@%d" % t
                out.append(p)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def level2_batch():
    """one batch above 1 MiB for the second scan level of swt_lower.hip (1,024 blocks of kOffBlock): short sentences up to the
    seam, then every representative six times with one letter between them, the first lead byte 4 bytes before byte 1,048,576,
    and short sentences behind.  -> (sentences, lead byte positions)"""
    rng = random.Random(1048576)
    unit = _cut(fill(SHORT, 4096, rng), 64, rng)
    texts = unit * (LEVEL2 // 4096 - 1)
    cur = sum(map(nbytes, texts))
    sent = fill(SHORT, LEVEL2 - 4 - cur - 2, rng) + "ab"
    at, leads = LEVEL2 - 4, []
    for (_kind, _n), cp in sorted(representatives().items()):
        for _ in OFFSETS:
            sent += chr(cp) + "a"
            leads.append(at)
            at += utf8_len(cp) + 1
    return texts + [sent + " "] + unit * 4, leads


# ------------------------------------------------------------------------------------------- the oracle on lowercase text
# oracle.OracleBPE.tokenize_batch_ids and its kin call str.lower() of this interpreter first; the sweeps are lowered by the
# fixture instead (lower()), so these hand the text to the same C functions as it is.

@functools.lru_cache(maxsize=None)
def s1_lowered():
    return ["ab" + chr(c) + "ab" for c in lower_table()[1:].tolist()]


def oracle_bpe(O, orc, lowered):
    """OracleBPE.tokenize_batch_ids without its str.lower()"""
    blob, off = O.pack(lowered)
    out = np.zeros(max(blob.size, 1), dtype=np.uint32)
    out_off = np.zeros(len(lowered) + 1, dtype=np.uint64)
    O.lib().orc_bpe_tokenize_batch(orc._h, O._p32(blob), O._p64(off), len(lowered), O._p32(out), O._p64(out_off))
    return out[:int(out_off[-1])], out_off


def oracle_wp(O, orc, lowered):
    """OracleWP.tokenize_batch_ids without its str.lower()"""
    blob, off = O.pack(lowered)
    ids, out_off, status = orc.tokenize_packed_mt(blob, off, 1)
    return ids, out_off, status


def oracle_census(O, lowered, wordpiece=False):
    """OracleBPETrainer / OracleWPTrainer over text that is lowercase already"""
    cls = O.OracleWPTrainer if wordpiece else O.OracleBPETrainer
    tr = cls.__new__(cls)
    blob, off = O.pack(lowered)
    tr._h = (O.lib().orc_wptrain_new if wordpiece else O.lib().orc_train_new)(O._p32(blob), O._p64(off), len(lowered))
    return tr
