"""Generators for the seams of the FastBPE word-dedup path (csrc/swt_dedup.hip: wordref_kernel<kDedupBpe>, ureg_kernel,
refcount_kernel, refwrite_kernel) and a Python model of the walk that says which seam a batch reaches.  Needs no GPU and no
library; tests/test_dedup_seam_cases.py checks every construction against the model, tests/test_gpu_dedup_seams.py runs them.

The walk (BPE mode).  Tile t holds the sentences that START in [1024 t, 1024 (t + 1)) (the last tile also those at the end of the
text); its span runs from its first sentence's start to the start of the next tile's first sentence.  One wave walks the span in
chunks: abase = cb & ~15, off0 = cb - abase, staged = min(span_end - abase, 1536), last = the span ends inside.  A chunk that is
not the last is cut at the highest boundary p (relative to abase) with off0 < p and p + 4 <= staged; a boundary is the lead byte
of a whitespace or punctuation character or a sentence start.  The four bytes of room keep a character the staged end clips (it is
decoded from fewer bytes than it has) behind the cut.  Without such a p one lane reads global memory from cb: a whitespace or
punctuation character alone, or a word up to the next whitespace, punctuation or sentence end.  The next chunk starts at the cut,
or behind what the one lane took.  Every word is a record: its code point when it is one symbol, else a slot of the hash table
(8-bit tag, 8-bit length, 40-bit offset of the representative); a word of 255 bytes or more, or one that finds neither itself nor
a free slot in 24 probes, gets a slot of its own at (1 << bits) + (position >> 1) and is never matched.  The tile lists the words it
inserted behind newlist[span_base >> 1].

What this geometry allows and what it does not: the docstring of tests/test_gpu_dedup_seams.py."""
import functools
import random
import unicodedata
from typing import NamedTuple

import numpy as np

TILE = 1024           # bytes of sentence starts per tile: SWT_DTILE
CAP = 1536            # staged bytes per chunk: SWT_DCAP
CUT_ROOM = 4          # p + 4 <= staged
MAX_PROBES = 24       # kDdMaxProbes
OWN_LEN = 255         # a word of this many bytes or more is never tabled: len >= 255u
U_MAX_TILES = 8192    # workgroups of the unique-word launch: kUMaxTiles
U_TILES = (64, 128, 256)  # tile of the unique-word launch under SWT_OPT_UNIQUE_TILE 64, 128, anything else
SCAN_BLOCK = 1024     # tiles per block of the two scans: t >> 10
DIRECT_BYTES = 1024   # kDirectBytes
DIRECT_SENTS = 64     # kDirectSents

SYM, WS, PN = 0, 1, 2

CHAIN = "abcdabcdabcd"  # twelve letters, one token under HANDMADE
STUBBORN = "bdbdbd"     # six tokens under HANDMADE: no merge has b and d next to each other
# proper: every pair ranks above the merges that make its symbols
HANDMADE = [("a", "b"), ("c", "d"), ("ab", "cd"), ("x", "y"), ("ż", "ó"), ("żó", "ł"), ("q", "q"), ("abcd", "abcd"), ("qq", "qq"),
            ("abcdabcd", "abcd"), ("xy", "xy"), ("ó", "ł")]
WORDS = ["ab", "abc", "abcd", "cd", "xy", "xyxy", "dab", "abab", "żół", "żółżół", "óż", "łłł", "qa", "aaaa", STUBBORN, CHAIN, "a", "b",
         "ż", "słowo", "nie", "wiem", "zażółć", ",", "x,y", "d.", "—", "¿co?"]
LETTERS = "abcdxyq"
ALNUM = "abcdefghijklmnopqrstuvwxyz0123456789"


def nbytes(t):
    return len(t.encode("utf-8"))


def is_proper(merges):
    """no pair twice, and every pair ranks above every merge that makes one of its symbols"""
    made = {}
    for i, (l, r) in enumerate(merges):
        made[l + r] = max(made.get(l + r, -1), i)
    return len(set(merges)) == len(merges) and all(made.get(l, -1) < i and made.get(r, -1) < i for i, (l, r) in enumerate(merges))


def classify(cp):
    """the pre-tokenizer's class of a code point: white space, punctuation, or part of a word"""
    ch = chr(cp)
    if ch in " \t\n\r" or unicodedata.category(ch) == "Zs":
        return WS
    if 33 <= cp <= 47 or 58 <= cp <= 64 or 91 <= cp <= 96 or 123 <= cp <= 126 or unicodedata.category(ch).startswith("P"):
        return PN
    return SYM


_ASCII = np.array([classify(c) if c < 128 else -1 for c in range(256)], dtype=np.int8)

_M = (1 << 64) - 1


def dd_hash(w):
    """dd_hash of swt_dedup.hip over the bytes of a word -> (the 64-bit hash, its 8-bit tag)"""
    n = len(w)
    p8 = lambda b: int.from_bytes(b[:8], "little")  # noqa: E731
    h = ((p8(w) ^ 0x9E3779B97F4A7C15) * 0xff51afd7ed558ccd) & _M
    h ^= h >> 32
    h = ((h ^ (p8(w[8:16]) if n > 8 else 0) ^ ((n << 56) & _M)) * 0xc4ceb9fe1a85ec53) & _M
    for i in range(16, n, 8):
        h ^= h >> 29
        h = ((h ^ p8(w[i:i + 8])) * 0x9E3779B97F4A7C15) & _M
    h ^= h >> 29
    h = (h * 0x94d049bb133111eb) & _M
    h ^= h >> 32
    return h, (h >> 40) & 0xFF


# ------------------------------------------------------------------------------------------------- the model

class Walk:
    """what wordref_kernel<kDedupBpe> does with a batch, from sentence offsets and bytes: chunks(t) = the trips of tile t's chunk
    loop, each {abase, off0, staged, last, cb, cut} or {.., giant: (kind, first byte, end)} with kind "ws", "punct", "symbol" (a
    one-symbol word) or "word"; n_words(t), sent_word(s), tabled(t) (the words of the tile that go through the table, in text
    order), n_new(t) (how many the tile lists, when no other tile holds one of them: else None, the race decides)."""

    def __init__(self, sents):
        raw = [s.encode("utf-8") for s in sents]
        self.text = b"".join(raw)
        n = self.n = len(self.text)
        self.off = np.concatenate([[0], np.cumsum([len(r) for r in raw], dtype=np.int64)]).astype(np.int64)
        self.n_sent = len(raw)
        a = np.frombuffer(self.text, dtype=np.uint8)
        self.cpos = cpos = np.flatnonzero((a & 0xC0) != 0x80).astype(np.int64)
        self.cnext = np.append(cpos[1:], n)
        cls = _ASCII[a[cpos]].copy()
        known = {}
        for i in np.flatnonzero(cls < 0):
            ch = self.text[cpos[i]:self.cnext[i]]
            if ch not in known:
                known[ch] = classify(ord(ch.decode("utf-8")))
            cls[i] = known[ch]
        self.cls = cls
        ss = np.zeros(cpos.size, dtype=bool)
        starts = self.off[:-1]
        ss[np.searchsorted(cpos, starts[starts < n])] = True
        prev = np.concatenate([[WS], cls[:-1]])
        wstart = (cls != WS) & ((cls == PN) | (prev != SYM) | ss)
        self.bnd = cpos[(cls != SYM) | ss]
        self.seps = cpos[cls != SYM]
        self.wpos = cpos[wstart]
        stops = np.append(cpos[(cls == WS) | wstart], n)
        self.wend = stops[np.searchsorted(stops, self.wpos, side="right")]
        self.single = (self.wend - self.wpos) <= self.cnext[wstart] - self.wpos
        self.n_tiles = max(1, -(-n // TILE))
        self.plan = np.append(np.searchsorted(starts, np.arange(self.n_tiles) * TILE, side="left"), self.n_sent)

    def span(self, t):
        lo, hi = int(self.plan[t]), int(self.plan[t + 1])
        return None if lo == hi else (int(self.off[lo]), int(self.off[hi]))

    @functools.lru_cache(maxsize=None)
    def chunks(self, t):
        sp = self.span(t)
        if sp is None:
            return []
        cb, end = sp
        out = []
        while True:
            abase = cb & ~15
            off0, avail = cb - abase, end - abase
            last = avail <= CAP
            staged = avail if last else CAP
            c = {"abase": abase, "off0": off0, "staged": staged, "last": last, "cb": cb, "cut": None, "giant": None}
            out.append(c)
            if last:
                return out
            j = int(np.searchsorted(self.bnd, abase + staged - CUT_ROOM, side="right")) - 1
            if j >= 0 and self.bnd[j] > cb:
                cb = c["cut"] = int(self.bnd[j])
                continue
            send = int(self.off[np.searchsorted(self.off, cb, side="right")])
            ci = int(np.searchsorted(self.cpos, cb))
            clen = int(self.cnext[ci]) - cb
            if self.cls[ci] != SYM:
                e, kind = cb + clen, ("ws" if self.cls[ci] == WS else "punct")
            else:
                k = int(np.searchsorted(self.seps, cb, side="right"))
                e = min(int(self.seps[k]) if k < self.seps.size else self.n, send)
                kind = "symbol" if e - cb <= clen else "word"
            c["giant"] = (kind, cb, e)
            cb = e
            if cb >= end:
                return out

    def _words(self, t):
        b, e = self.span(t)
        return int(np.searchsorted(self.wpos, b)), int(np.searchsorted(self.wpos, e))

    def n_words(self, t):
        if self.span(t) is None:
            return 0
        lo, hi = self._words(t)
        return hi - lo

    def sent_word(self, s):
        """words of sentence s's tile before the sentence"""
        t = int(np.searchsorted(self.plan, s, side="right")) - 1
        return int(np.searchsorted(self.wpos, self.off[s])) - self._words(t)[0]

    @functools.lru_cache(maxsize=None)
    def tabled(self, t):
        if self.span(t) is None:
            return ()
        lo, hi = self._words(t)
        return tuple(self.text[self.wpos[i]:self.wend[i]] for i in range(lo, hi) if not self.single[i])

    def records(self, t):
        """(one-symbol records, table records) of tile t"""
        if self.span(t) is None:
            return 0, 0
        lo, hi = self._words(t)
        one = int(np.count_nonzero(self.single[lo:hi]))
        return one, hi - lo - one

    def n_new(self, t):
        mine = self.tabled(t)
        distinct = set(mine)
        for u in range(self.n_tiles):
            if u != t and distinct & set(self.tabled(u)):
                return None
        return len({w for w in mine if len(w) < OWN_LEN}) + sum(len(w) >= OWN_LEN for w in mine)

    def unique_words(self):
        """the unique-word text in the order ureg_kernel writes it, when no word lives in two tiles (tiles in order, a tile's
        words in text order, a word of 255 bytes or more once per occurrence)"""
        out, seen = [], set()
        for t in range(self.n_tiles):
            for w in self.tabled(t):
                if len(w) >= OWN_LEN or w not in seen:
                    seen.add(w)
                    out.append(w)
        return out

    def tile2(self, utile):
        """(tiles of the unique-word launch, the tile size the device settles on)"""
        tmin = utile if utile in (64, 128) else 256
        n2 = min(max(1, -(-self.n // tmin)), U_MAX_TILES)
        ub = sum(map(len, self.unique_words()))
        return n2, max(-(-ub // n2), tmin)

    def crossings(self, utile):
        """per unique word: the boundaries of the unique-word launch's tiles inside (start, end]"""
        t2 = self.tile2(utile)[1]
        out, pos = [], 0
        for w in self.unique_words():
            out.append((pos + len(w)) // t2 - pos // t2)
            pos += len(w)
        return out


# ------------------------------------------------------------------------------------------------- batches

class Batch(NamedTuple):
    name: str
    sents: list
    bits: int = 0      # SWT_OPT_DEDUP_TABLE_BITS
    utile: int = 0     # SWT_OPT_UNIQUE_TILE
    expect: tuple = () # what the model must show: see holds()


def holds(batch, walk=None):
    """asserts that the model shows every event the batch is named for; -> the model"""
    w = walk or Walk(batch.sents)
    for ex in batch.expect:
        kind, tag = ex[0], "%s: %r" % (batch.name, ex)
        if kind == "chunk":      # trip idx of tile t stages from abase with off0
            _, t, idx, abase, off0 = ex
            ch = w.chunks(t)
            assert len(ch) > idx and ch[idx]["abase"] == abase and ch[idx]["off0"] == off0 and ch[idx]["giant"] is None, tag
        elif kind == "last":     # ... and is the last one (or not)
            _, t, idx, last = ex
            assert w.chunks(t)[idx]["last"] == last, tag
        elif kind == "cut":      # ... and is cut at the absolute byte p
            _, t, idx, p = ex
            assert w.chunks(t)[idx]["cut"] == p, tag
        elif kind == "giant":    # some tile hands (kind, first byte, end) to one lane
            assert any(c["giant"] == ex[1:] for t in range(w.n_tiles) for c in w.chunks(t)), tag
        elif kind == "no giant":
            assert not any(c["giant"] for t in range(w.n_tiles) for c in w.chunks(t)), tag
        elif kind == "n_new":
            assert w.n_new(ex[1]) == ex[2], tag + " model %r" % (w.n_new(ex[1]),)
        elif kind == "words over":  # the tile has more word records than this, of both kinds
            one, tab = w.records(ex[1])
            assert one + tab > ex[2] and one >= 100 and tab >= 100, tag
        elif kind == "residues":    # the word occurs at this many residues mod 16
            word = ex[1].encode("utf-8")
            res = {int(p) % 16 for p, e in zip(w.wpos, w.wend) if w.text[p:e] == word}
            assert len(res) >= ex[2], tag
        elif kind == "crossings":   # the unique-word launch has words that cross exactly these numbers of tile boundaries
            got = set(w.crossings(batch.utile))
            assert set(ex[1]) <= got and max(got) >= ex[2], tag + " model %r" % sorted(got)
        elif kind == "tile2":
            assert w.tile2(batch.utile) == ex[1:], tag + " model %r" % (w.tile2(batch.utile),)
        elif kind == "tiles":
            assert w.n_tiles == ex[1], tag
        elif kind == "rep in tail":  # the word occurs twice, and first inside the last 16 bytes of the text
            word = ex[1].encode("utf-8")
            at = [int(p) for p, e in zip(w.wpos, w.wend) if w.text[p:e] == word]
            assert len(at) == 2 and at[0] + 16 > w.n, tag
        else:
            raise AssertionError("unknown expectation " + tag)
    return w


def fill(n, rng, words=WORDS):
    """words separated by single spaces, n bytes of UTF-8 exactly (ends with a space; 'q' runs make up the remainder)"""
    out, left = [], n
    while left > 0:
        w = rng.choice(words)
        b = nbytes(w) + 1
        if b > left:
            w, b = "q" * (left - 1), left
        out.append(w)
        left -= b
    return " ".join(out) + " " if out else ""


def tail(rng):
    return [fill(rng.randrange(20, 70), rng) for _ in range(3)]


def word_of(n, salt=0):
    """a word of n letters that no other (n, salt) gives"""
    k = (n * 7 + salt * 3) % len(LETTERS)
    body = (LETTERS[k:] + LETTERS[:k]) * (n // len(LETTERS) + 1)
    return (LETTERS[salt % len(LETTERS)] + body)[:n]


def counter(i, n):
    """the i-th word of n letters of a base-26 counter"""
    out = []
    for _ in range(n):
        out.append(chr(97 + i % 26))
        i //= 26
    return "".join(out)


STRADDLERS = [("an ASCII word", CHAIN), ("ż", "ż"), ("€", "€"), ("an emoji", "\U0001F600"), (",", ","), ("—", "—"), ("¿", "¿"),
              ("U+00A0", "\u00a0"), ("U+3000", "\u3000"), ("three spaces", "   "),
              ("a word around U+2800", "ab\u2800cd"),  # E2 A0 80, not a boundary; cut off behind two bytes it decodes as U+00A0, which is one
              ("a sentence start", None), ("empty sentences", None)]
OFF0 = (0, 1, 7, 8, 15)


def chunk_end_batches(rng, which, p):
    """a straddler whose first byte lands on abase + 1,536 + d, d = -8 .. 2, at one off0 of OFF0: at the end of a tile's first
    chunk (the tile opens at 1,024 + off0: cb is a span start) and of its second (the first is cut at a space whose place gives the
    off0: cb is a cut).  The tile is tile 1; a sentence start as the straddler ends its span there."""
    out = []
    B = TILE + (p if which == 0 else 3)
    c1 = (2544 if p <= 12 else 2528) + p  # second chunk: the space the first chunk is cut at (the q-run behind it hides 2,556)
    E = (TILE if which == 0 else c1 & ~15) + CAP
    for sname, s in STRADDLERS:
        for d in range(-8, 3):
            X = E + d
            body = "" if which == 0 else fill(c1 + 1 - B, rng) + "q" * 16 + " "
            body += fill(X - B - nbytes(body), rng)
            if s is not None and rng.random() < 0.5:
                body = body[:-1] + "a"  # no space in front of the straddler
            expect = [("chunk", 1, which, E - CAP, p)]
            if which == 1:
                expect.append(("cut", 1, 0, c1))
            if s is None:
                mid = [body] + ([""] * 5 if sname == "empty sentences" else []) + [fill(150, rng)]
                expect.append(("last", 1, which, d <= 0))
            else:
                mid = [body + s + " " + fill(120, rng)]
                assert mid[0].encode("utf-8")[X - B:].startswith(s.encode("utf-8"))
            out.append(Batch("chunk end %d: %s at end %+d, off0 %d" % (which + 1, sname, d, p),
                             [fill(B, rng)] + mid + tail(rng), expect=tuple(expect)))
    return out


def giant_batches(rng):
    """words that no chunk holds, with neighbours before and after: see the names"""
    out = []
    G = word_of(2000)
    for p in (0, 15):
        B = TILE + p
        for n in range(1512, 1541):
            for kind in ("ascii", "ż"):
                w = word_of(n, n) if kind == "ascii" else ("a" if n % 2 else "") + "ż" * (n // 2)
                ev = ("giant", "word", B, B + n) if n > CAP - CUT_ROOM - p else ("no giant",)
                out.append(Batch("giant: %s word of %d bytes opens a span at off0 %d" % (kind, n, p),
                                 [fill(B, rng), w + " " + fill(40, rng)] + tail(rng), expect=(ev,)))
                # behind "ab " the first chunk is cut at the space, one lane takes the space and then the word
                ev = (("giant", "ws", B + 2, B + 3), ("giant", "word", B + 3, B + 3 + n)) if n > CAP - CUT_ROOM - 3 else (("no giant",),)
                if p == 0:
                    out.append(Batch("giant: %s word of %d bytes behind a short word" % (kind, n),
                                     [fill(B, rng), "ab " + w + " ab " + fill(40, rng)] + tail(rng), expect=ev))
    for p in (0, 15):
        B = TILE + p
        lead = lambda: [fill(B, rng)]  # noqa: E731
        for sep, kind in ((",", "punct"), (" ", "ws"), ("—", "punct")):
            k = nbytes(sep)
            out.append(Batch("giant: a lone %r opens a span in front of a giant word, off0 %d" % (sep, p),
                             lead() + [sep + G + " " + fill(30, rng)] + tail(rng),
                             expect=(("giant", kind, B, B + k), ("giant", "word", B + k, B + k + 2000))))
            out.append(Batch("giant: a lone %r between a short word and a giant one, off0 %d" % (sep, p),
                             lead() + ["ab" + sep + G + " " + fill(30, rng)] + tail(rng),
                             expect=(("cut", 1, 0, B + 2), ("giant", kind, B + 2, B + 2 + k), ("giant", "word", B + 2 + k, B + 2 + k + 2000))))
        out.append(Batch("giant: ',' directly behind a giant word, off0 %d" % p, lead() + [G + ", ab " + fill(30, rng)] + tail(rng),
                         expect=(("giant", "word", B, B + 2000),)))
        out.append(Batch("giant: ends with its sentence, off0 %d" % p, lead() + [G, fill(40, rng)] + tail(rng),
                         expect=(("giant", "word", B, B + 2000),)))
        out.append(Batch("giant: ends the text, off0 %d" % p, lead() + [fill(30, rng), "ab " + G],
                         expect=(("giant", "word", B + 33, B + 2033),)))
        out.append(Batch("giant: two equal giant words and a third, off0 %d" % p, lead() + [G + " " + G + " ab", G] + tail(rng),
                         expect=(("giant", "word", B, B + 2000), ("giant", "word", B + 2001, B + 4001), ("giant", "word", B + 4004, B + 6004))))
        out.append(Batch("giant: 70 empty sentences behind a giant word, off0 %d" % p, lead() + [G] + [""] * 70 + [fill(40, rng)] + tail(rng),
                         expect=(("giant", "word", B, B + 2000),)))
        out.append(Batch("giant: made of ż, 3,000 bytes, off0 %d" % p, lead() + ["ż" * 1500 + " " + fill(30, rng)] + tail(rng),
                         expect=(("giant", "word", B, B + 3000),)))
    ones = " ".join(rng.choice("abcdxyż") if i % 7 else rng.choice(("ab", "xy", "cd", "żó")) for i in range(4000))
    twos = " ".join(rng.choice(("ab", "xy", "cd", "qa", "óż", "dd")) if i % 5 else rng.choice("abż") for i in range(2000))
    lead = fill(TILE + 7, rng)
    t2 = (nbytes(lead) + nbytes(ones)) // TILE
    out.append(Batch("giant: a sentence of 4,000 words, most of one letter, one of 2,000, most of two, empty sentences behind",
                     [lead, ones] + [""] * 3 + [twos] + [""] * 70 + tail(rng), expect=(("words over", 1, 2 * CAP), ("words over", t2, CAP))))
    return out


LENGTHS = list(range(2, 41)) + [253, 254, 255, 256, 300]
COMPARE_L = (9, 16, 17, 24, 25, 40, 254)
COMPARE_K = (0, 7, 8, 15, 16, 17, -1)


def aligned(words, rng, residues):
    """each word once per residue: a sentence in which the word's first byte lies at that residue mod 16 (q runs shift it)"""
    text = ""
    for r in residues:
        for w in words:
            pad = (r - nbytes(text)) % 16
            text += ("q" * (pad - 1) + " " if pad else "") + w + " "
    return text


@functools.lru_cache(maxsize=None)
def colliding(L, k):
    """two words of L bytes that differ at byte k only and have the same tag and, in a table of sixteen slots, the same home slot:
    the second finds the first's slot with an equal head, so the byte compare alone tells them apart.  None where 300 random
    stems give no such pair: byte k is then the top byte of the last eight bytes the hash takes in, which the few steps behind it
    spread over tag and slot without a collision (L = 16, 24, 40 with k = L - 1)."""
    rng = random.Random(1000 * L + k)
    for _ in range(300):
        base = [rng.choice("abcdxyq") for _ in range(L)]
        seen = {}
        for c in "abcdefghijklmnopqrstuvwxyz":
            base[k] = c
            w = "".join(base)
            h, tag = dd_hash(w.encode())
            if (tag, h & 15) in seen:
                return seen[tag, h & 15], w
            seen[tag, h & 15] = w
    return None


def compare_sets():
    """[(L, k, three words that differ at byte k only, whether the first two collide on tag and home slot)]"""
    out = []
    for L in COMPARE_L:
        for k in sorted({kk % L for kk in COMPARE_K if kk < L}):
            pair = colliding(L, k)
            a = pair[0] if pair else word_of(L, 5)
            b = pair[1] if pair else a[:k] + ("m" if a[k] != "m" else "n") + a[k + 1:]
            c = a[:k] + next(x for x in "zwv" if x not in (a[k], b[k])) + a[k + 1:]
            out.append((L, k, (a, b, c), pair is not None))
    return out


def length_batches(rng):
    out = []
    words = [word_of(n, 1) for n in LENGTHS]
    for lo in range(0, len(words), 11):
        part = words[lo:lo + 11]
        out.append(Batch("lengths: words of %d .. %d bytes at three alignments" % (nbytes(part[0]), nbytes(part[-1])),
                         [fill(60, rng), aligned(part, rng, (3, 8, 15)), aligned(part[::-1], rng, (0,))] + tail(rng),
                         expect=tuple(("residues", w, 3) for w in part)))
    for L, k, trio, _ in compare_sets():
        for bits in (4, 0):
            # the colliding pair first, so that under sixteen slots both are tabled; few other distinct words
            few = ["ab", "xy", "abcd", "żół", "a", ","]
            out.append(Batch("compare: words of %d bytes that differ at byte %d, table bits %d" % (L, k, bits),
                             [" ".join(trio[:2] * 2), " ".join(trio) + " " + fill(40, rng, few), fill(TILE + 60, rng, few), " ".join(trio[::-1])],
                             bits=bits))
    stem = word_of(40, 2)
    pre = [stem[:n] for n in (7, 8, 15, 16, 17, 40)]
    out.append(Batch("compare: words that are prefixes of one another", [fill(60, rng), " ".join(pre * 2), aligned(pre, rng, (5, 12))] + tail(rng)))
    for extra in range(16):
        for pair in (("xyx", "xyx"), ("abcdx", "abcdy"), ("xyxy", "xyxy")):
            sents = [fill(TILE + 200 + extra, rng, ["ab", "abc", "żół", "cd", "a"]), "ab cd " + pair[0] + " " + pair[1]]
            ev = (("rep in tail", pair[0], 2),) if pair[0] == pair[1] else ()
            out.append(Batch("compare: %r and %r in the last 16 bytes, text of %d bytes" % (pair + (sum(map(nbytes, sents)),)), sents, expect=ev))
    return out


ONE_SYMBOL = ["a", "ż", "€", "\U0001F600", ",", "—"]
TWO_SYMBOL = ["ab", "aż", "ża", "a€", "€a", "żż"]


def one_symbol_batches(rng):
    out = []
    mix = ONE_SYMBOL + TWO_SYMBOL
    out.append(Batch("one symbol: next to two-symbol words of the same length",
                     [fill(80, rng)] + [" ".join(rng.choice(mix) for _ in range(60)) for _ in range(12)] + tail(rng)))
    out.append(Batch("one symbol: no spaces between the punctuation", [fill(80, rng), ",—,a—ż,€—ab,aż—", "a,ż,€,\U0001F600,ab,ża" * 40, "—" * 200 + "," * 300] + tail(rng)))
    for s in ONE_SYMBOL:
        k = nbytes(s)
        # tile 1 holds this sentence alone: the symbol and white space up to the next tile
        out.append(Batch("one symbol: %r is a tile's only word" % s, [fill(TILE, rng), s + " " * (TILE - k), fill(TILE + 30, rng)] + tail(rng)))
        out.append(Batch("one symbol: %r alone in a small call" % s, [s]))
        for d in range(-k - 4, 1):
            # ends d bytes short of the first chunk's staged end of tile 1, and of where its cut may lie
            body = fill(CAP + d - k, rng)
            out.append(Batch("one symbol: %r ends %d bytes before a chunk end" % (s, -d),
                             [fill(TILE, rng), body + s + " " + rng.choice(TWO_SYMBOL) + " " + fill(200, rng)] + tail(rng),
                             expect=(("chunk", 1, 0, TILE, 0), ("last", 1, 0, False))))
    return out


def dense(n, first=0):
    """n distinct two-letter words"""
    return [ALNUM[i // 36] + ALNUM[i % 36] for i in range(first, first + n)]


def density_batches(rng):
    """tiles whose sentences are distinct two-letter words back to back: sentence starts are the only word boundaries"""
    out = []
    q3 = ["qqq"]
    for bits in (0, 4, 16):
        out.append(Batch("density: 512 + 512 two-letter words, even span_base, table bits %d" % bits,
                         [fill(TILE, rng, q3)] + dense(1024) + [fill(50, rng, q3)], bits=bits,
                         expect=(("n_new", 1, 512), ("n_new", 2, 512))))
        out.append(Batch("density: 512 + 512 two-letter words, odd span_base, table bits %d" % bits,
                         ["a", fill(TILE, rng, q3)] + dense(1024) + [fill(50, rng, q3)], bits=bits,
                         expect=(("n_new", 1, 512), ("n_new", 2, 512))))
    for n in (64, 65, 129):
        out.append(Batch("density: a tile with %d new words" % n,
                         [fill(TILE, rng, q3), (" ".join(dense(n, 200)) + " " + " ".join(dense(n // 2, 200))).ljust(TILE), fill(30, rng, q3)],
                         expect=(("n_new", 1, n),)))
    return out


UNIQUE_LENGTHS = (63, 64, 65, 130, 257, 600, 1100)


def unique_batches(rng):
    out = []
    short = iter(counter(i, 3) for i in range(0, 4000, 37))
    sents = [" ".join([next(short), next(short), word_of(n, 3), next(short), next(short)]) for n in UNIQUE_LENGTHS]
    for ut in (64, 128, 0):
        ev = (("crossings", (1, 2), 8),) if ut == 64 else ()
        out.append(Batch("unique pass: words of 63 .. 1,100 bytes between short ones, unique tile %d" % ut, sents, utile=ut, expect=ev))
    return out


def counter_batch():
    """76,000 distinct seven-letter words: 532,000 unique bytes exceed 8,192 tiles of 64, so the device settles on tiles of 65"""
    words = [counter(i * 7919, 7) for i in range(76000)]
    assert len(set(words)) == len(words)
    sents = [" ".join(words[i:i + 25]) + " " for i in range(0, len(words), 25)]
    return [Batch("unique pass: 76,000 distinct seven-letter words, unique tile 64", sents, utile=64, expect=(("tile2", U_MAX_TILES, 65),))]


def scan_batches(rng):
    """the same forty short sentences over and over, a handful of new words in the last tiles: 1,023, 1,024 and 1,025 tiles"""
    forty = [fill(rng.randrange(20, 44), rng) for _ in range(40)]
    block = sum(map(nbytes, forty))
    out = []
    for tiles in (SCAN_BLOCK - 1, SCAN_BLOCK, SCAN_BLOCK + 1):
        total = tiles * TILE - 100
        sents = forty * (total // block - 1)
        sents += [" ".join(counter(i + tiles, 5) for i in range(6)) for _ in range(2)]
        left = total - sum(map(nbytes, sents))
        sents += [fill(left - 40, rng), "nowe " + counter(tiles, 6) + " " + fill(27, rng)]
        out.append(Batch("scan blocks: %d tiles" % tiles, sents, expect=(("tiles", tiles),)))
    return out


def small_batches(rng):
    """calls of at most 1,024 bytes and 64 sentences: under DEDUP_ALWAYS the dedup runs over the pinned host block"""
    return [Batch("small: one sentence of 40 bytes", [fill(40, rng)]),
            Batch("small: 64 sentences, 1,024 bytes", [fill(16, rng) for _ in range(64)]),
            Batch("small: empty sentences and one word", ["", "", CHAIN, ""])]


CHUNK_END = {"chunk end %d, off0 %d" % (which + 1, p): (which, p) for which in (0, 1) for p in OFF0}
FAMILIES = {**{f: (lambda rng, wp=wp: chunk_end_batches(rng, *wp)) for f, wp in CHUNK_END.items()}, "giant": giant_batches, "lengths": length_batches, "one symbol": one_symbol_batches,
            "density": density_batches, "unique": unique_batches, "scan": scan_batches, "small": small_batches}
SEEDS = {**{f: CAP * (which + 1) + p for f, (which, p) in CHUNK_END.items()}, "giant": 2000, "lengths": 255, "one symbol": 1, "density": 512, "unique": 8192, "scan": 1025, "small": 64}
# every k-th batch of a family is one GPU test (measured: the docstring of tests/test_gpu_dedup_seams.py)
PARTS = {"giant": 6, "scan": 3}
CASES = [(f, k) for f in FAMILIES for k in range(PARTS.get(f, 1))] + [("counter", 0)]


@functools.lru_cache(maxsize=None)
def batches(family):
    if family == "counter":
        return counter_batch()
    return FAMILIES[family](random.Random(SEEDS[family]))


def part(family, k):
    return batches(family)[k::PARTS.get(family, 1)]
