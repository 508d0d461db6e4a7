"""Generators and Python models for the seams of the three device Counters: the training word census (csrc/swt_words.hip:
census_kernel, word_insert, collect, sort, measure, emit), the token histogram (token_hist_kernel in csrc/swt_metrics.hip) and the
token-sequence equivalence (token_equiv_wave_kernel, token_equiv_block_kernel, same file).  Needs no GPU, no torch and no library;
tests/test_counter_cases.py checks on the CPU that every construction reaches the seam it is named for,
tests/test_gpu_counters.py runs them on the device.

The census walk.  Tile t holds the sentences that START in [512 t, 512 (t + 1)) (the last tile also those at the end of the text);
its span runs from its first sentence's start to the start of the next tile's first sentence.  One wave walks the span in chunks:
abase = cb & ~15, off0 = cb - abase, staged = min(span_end - abase, 1024), last = the span ends inside.  A chunk that is not the
last is cut at the highest boundary p (relative to abase) with p > off0 and p + 4 <= staged; a boundary is the lead byte of a
whitespace or punctuation character, or a sentence start.  Without such a p one lane walks global memory from cb: a whitespace
character alone (no word), a punctuation character alone (a word), or a word up to the next whitespace, punctuation or `send`.
Every word occurrence is hashed (FNV-1a, two multiplies) and found or inserted in one open-addressing table of 1 << bits slots,
bits = the smallest >= 10 with 1 << bits >= 2 * n_occ + 16; a slot is [tag:16 | length:8 | offset:40], and a word of 255 bytes or
more (length field 255) never matches anything: every occurrence of it is an entry of its own with frequency 1.

What this geometry allows (worked out from the kernel, so nobody looks for more).  The one-lane walk runs only when the chunk has
no boundary in (off0, staged - 4], so every sentence of the tile that starts behind cb is done with and its `send` is ALWAYS the
span end: `s` always runs to `s_hi`.  "Ended by the sentence end" and "ended by the span end" are therefore one exit of the loop,
reached by a long word that ends its sentence with other sentences behind it and by one that ends the text.  For the same reason
a sentence start cannot be the only boundary in a chunk's tail: a sentence that starts 1,019 bytes or more behind abase belongs to
a later tile, the span ends there and the chunk is the last one (staged = the span's rest), unless it starts more than 1,024 bytes
behind abase, in which case the chunk sees no boundary at all.  The sentence-start column of the cut-rule sweep shows exactly that
in the model and so sits on the `avail <= kWCap` seam instead.

The histogram.  A wave counts a stretch of 64 * kMhPerLane = 4,096 ids in a 1,024-slot LDS table (home slot (idx * 2654435761)
>> 22 of the 32-bit product, 8 linear probes, then the global array), flushes it, and takes the stretch n_waves * 4,096 further
on; the grid is capped at 2,048 blocks of 4 waves.

The equivalence.  token_equiv_wave_kernel: min(n_rows / 4, 8 * n_cu) blocks of 4 waves, wave w takes rows w, w + n_waves, ...;
token_equiv_block_kernel: min(tiles, n_cu) workgroups, workgroup g takes the 1,024-row tiles g, g + n_cu, ..."""
import functools
import os
import random
import re
from collections import Counter
from typing import NamedTuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "subword-tokenizers_amd", "csrc")

# what this file was written against; constants() reads the kernels' own values and tests/test_counter_cases.py compares
TILE = 512            # kWTile
CAP = 1024            # kWCap
CUT_ROOM = 4          # p + 4 <= staged
LONG = 255            # len < 255u ? len : 255u
OFF_BITS = 40         # (1ull << 40) - 1ull
TAG_SHIFT = 48        # (h >> 48) << 48: a 16-bit tag
MIN_BITS = 10         # uint32_t bits = 10
OCC_MUL, OCC_ADD = 2, 16  # 2 * n_occ + 16
MH_THREADS, MH_SLOTS, MH_PER_LANE, MH_PROBES, MH_MAX_BLOCKS = 256, 1024, 64, 8, 2048
MH_MUL, MH_SHIFT = 2654435761, 22
TE_THREADS, TE_WAVE_CAP, TE_BLOCK_THREADS, TE_BLOCK_CAP = 256, 256, 1024, 2048
TE_WAVE_BLOCKS_PER_CU, TE_BLOCK_BLOCKS_PER_CU = 8, 1
EXPECTED_CONSTANTS = {
    "kWTile": TILE, "kWCap": CAP, "cut_room": CUT_ROOM, "long": LONG, "off_bits": OFF_BITS, "tag_shift": TAG_SHIFT, "min_bits": MIN_BITS,
    "occ_mul": OCC_MUL, "occ_add": OCC_ADD, "kMhThreads": MH_THREADS, "kMhSlots": MH_SLOTS, "kMhPerLane": MH_PER_LANE, "mh_probes": MH_PROBES,
    "mh_max_blocks": MH_MAX_BLOCKS, "mh_mul": MH_MUL, "mh_shift": MH_SHIFT, "kTeThreads": TE_THREADS, "kTeWaveCap": TE_WAVE_CAP,
    "kTeBlockThreads": TE_BLOCK_THREADS, "kTeBlockCap": TE_BLOCK_CAP, "te_wave_blocks_per_cu": TE_WAVE_BLOCKS_PER_CU,
    "te_block_blocks_per_cu": TE_BLOCK_BLOCKS_PER_CU}

MH_STRETCH = 64 * MH_PER_LANE                   # ids a wave counts before it flushes: 4,096
MH_BLOCK = MH_THREADS * MH_PER_LANE             # ids of a block's four stretches: 16,384
MH_SECOND = MH_MAX_BLOCKS * MH_BLOCK            # the first id of wave 0's second stretch: 33,554,432

WP_CONT = 0x110000    # _native.WP_CONT: '##c' = WP_CONT + ord(c)
SYM, WS, PN = 0, 1, 2


def _read(name):
    with open(os.path.join(CSRC, name), encoding="utf-8") as f:
        return f.read()


def _one(src, pattern):
    found = re.findall(pattern, src)
    assert len(found) == 1, "%r: %d matches" % (pattern, len(found))
    return found[0]


@functools.lru_cache(maxsize=None)
def constants():
    """every constant a construction here depends on, parsed from the kernels' sources (each pattern must match exactly once)"""
    w, m = _read("swt_words.hip"), _read("swt_metrics.hip")
    occ = _one(w, r"while \(\(1ull << bits\) < (\d+) \* n_occ \+ (\d+)\) bits\+\+;")
    _one(w, r"const uint32_t lf = len < (\d+)u \? len : \1u;")
    _one(w, r"if \(lf != (255)u && \(v & ~kOffMask\) == head\)")
    _one(w, r"if \(lf == (255)u\) T\.biglen\[idx\] = len;")
    _one(m, r"uint64_t blocks = \(n \+ \(uint64_t\)kMhThreads \* kMhPerLane - (1)\) / \(\(uint64_t\)kMhThreads \* kMhPerLane\);")
    _one(m, r"for \(uint64_t base = wave_id \* (64) \* kMhPerLane; base < n; base \+= n_waves \* 64 \* kMhPerLane\)")
    _one(m, r"for \(uint64_t row = wave_id; row < n_rows; row \+= (n_waves)\)")
    _one(m, r"for \(uint64_t tile = blockIdx\.x; tile \* kTeBlockThreads < n_rows; tile \+= (gridDim\.x)\)")
    _one(m, r"uint64_t blocks = \(n_rows \+ kTeThreads / 64 - 1\) / \(kTeThreads / (64)\), cap")
    _one(m, r"blocks = \(n_rows \+ kTeBlockThreads - (1)\) / kTeBlockThreads;")
    return {
        "kWTile": int(_one(w, r"constexpr int kWTile = (\d+);")), "kWCap": int(_one(w, r"constexpr int kWCap = (\d+);")),
        "cut_room": int(_one(w, r"__ballot\(inr && p > off0 && p \+ (\d+) <= staged\)")),
        "long": int(_one(w, r"const uint32_t lf = len < (\d+)u \? len : \d+u;")),
        "off_bits": int(_one(w, r"constexpr unsigned long long kOffMask = \(1ull << (\d+)\) - 1ull;")),
        "tag_shift": int(_one(w, r"const unsigned long long head = \(\(h >> (\d+)\) << \1\) \| \(\(unsigned long long\)lf << 40\);")),
        "min_bits": int(_one(w, r"uint32_t bits = (\d+);\n\s+while \(\(1ull << bits\)")),
        "occ_mul": int(occ[0]), "occ_add": int(occ[1]),
        "kMhThreads": int(_one(m, r"constexpr int kMhThreads = (\d+);")), "kMhSlots": int(_one(m, r"constexpr int kMhSlots = (\d+);")),
        "kMhPerLane": int(_one(m, r"constexpr int kMhPerLane = (\d+);")),
        "mh_probes": int(_one(m, r"for \(int probe = 0; probe < (\d+) && !done; probe\+\+\)")),
        "mh_max_blocks": int(_one(m, r"if \(blocks > (\d+)\) blocks = \1;")),
        "mh_mul": int(_one(m, r"uint32_t h = \(idx \* (\d+)u\) >> \d+;")), "mh_shift": int(_one(m, r"uint32_t h = \(idx \* \d+u\) >> (\d+);")),
        "kTeThreads": int(_one(m, r"constexpr int kTeThreads = (\d+);")), "kTeWaveCap": int(_one(m, r"constexpr uint32_t kTeWaveCap = (\d+);")),
        "kTeBlockThreads": int(_one(m, r"constexpr int kTeBlockThreads = (\d+);")),
        "kTeBlockCap": int(_one(m, r"constexpr uint32_t kTeBlockCap = (\d+);")),
        "te_wave_blocks_per_cu": int(_one(m, r"cap = \(uint64_t\)device_cus\(\) \* (\d+);")),
        "te_block_blocks_per_cu": len(re.findall(r"\n  cap = \(uint64_t\)device_cus\(\);\n", m))}


def nbytes(t):
    return len(t.encode("utf-8"))


# ============================================================================================================ the census

ALPHABET = frozenset("abcdefghijklmnopqrstuvwxyz0123456789 \t!\"#$%&'()*+,-./:;<=>?@[\\]^_`{|}~żół\u2800")


def classify(cp):
    """the pre-tokenizer's class of a character of ALPHABET (tests/test_counter_cases.py holds it against the oracle's split)"""
    if cp in (32, 9, 10, 13):
        return WS
    if 33 <= cp <= 47 or 58 <= cp <= 64 or 91 <= cp <= 96 or 123 <= cp <= 126:
        return PN
    return SYM


_CLS = np.array([classify(c) if c < 128 else SYM for c in range(256)], dtype=np.int8)
_M = (1 << 64) - 1


def word_hash(w):
    """word_hash of swt_words.hip over the bytes of a word"""
    h = 0xcbf29ce484222325
    for b in w:
        h = ((h ^ b) * 0x100000001b3) & _M
    h ^= h >> 29
    h = (h * 0x9E3779B97F4A7C15) & _M
    return h ^ (h >> 32)


def word_hash_np(words):
    """the same over uint8[n, L]: n words of one length -> uint64[n]"""
    h = np.full(words.shape[0], 0xcbf29ce484222325, dtype=np.uint64)
    for i in range(words.shape[1]):
        h = (h ^ words[:, i].astype(np.uint64)) * np.uint64(0x100000001b3)
    h ^= h >> np.uint64(29)
    h *= np.uint64(0x9E3779B97F4A7C15)
    return h ^ (h >> np.uint64(32))


def table_bits(n_occ):
    bits = MIN_BITS
    while (1 << bits) < OCC_MUL * n_occ + OCC_ADD:
        bits += 1
    return bits


class Insert(NamedTuple):
    word: bytes
    home: int
    slot: int
    new: bool       # claimed an empty slot
    foreign: int    # slots passed whose tag or length differ (255-byte entries not counted)
    compared: int   # slots passed after a byte compare that failed: same tag, same length, another word
    long: int       # slots passed that hold a 255-byte entry
    wrapped: bool   # the probe went from the last slot to slot 0


def table_model(occurrences, bits=None):
    """word_insert over the occurrences in text order (the device's order is a race; the entries are the same, their slots need
    not be) -> (bits, [Insert per occurrence])"""
    bits = table_bits(len(occurrences)) if bits is None else bits
    mask = (1 << bits) - 1
    slots, out = {}, []
    for w in occurrences:
        h = word_hash(w)
        lf = min(len(w), LONG)
        head = (h >> TAG_SHIFT, lf)
        idx = home = h & mask & 0xFFFFFFFF
        foreign = compared = long = 0
        wrapped = False
        while True:
            v = slots.get(idx)
            if v is None:
                slots[idx] = (head, w)
                new = True
                break
            if lf != LONG and v[0] == head:
                if v[1] == w:
                    new = False
                    break
                compared += 1
            elif v[0][1] == LONG:
                long += 1
            else:
                foreign += 1
            wrapped |= idx == mask
            idx = (idx + 1) & mask
        out.append(Insert(w, home, idx, new, foreign, compared, long, wrapped))
    return bits, out


class Stream(NamedTuple):
    """the trainer's initial state: the unique-word stream, the initial vocabulary, the pair histogram"""
    syms: np.ndarray   # uint32
    woff: np.ndarray   # uint64[n_words + 1]
    freq: np.ndarray   # uint32[n_words]
    base: np.ndarray   # uint32, sorted
    hist: dict         # (left << 32 | right) -> count

    @property
    def n_words(self):
        return int(self.freq.size)


def _stream(entries, cont=0):
    syms, woff, freq, hist = [], [0], [], Counter()
    for w, f in entries:
        cps = [ord(c) for c in w]
        cps = cps[:1] + [c + cont for c in cps[1:]]
        syms += cps
        woff.append(len(syms))
        freq.append(f)
        for a, b in zip(cps[:-1], cps[1:]):
            hist[(a << 32) | b] += f
    syms = np.array(syms, dtype=np.uint32)
    return Stream(syms, np.array(woff, dtype=np.uint64), np.array(freq, dtype=np.uint32), np.unique(syms).astype(np.uint32), dict(hist))


def census_entries(sent_words):
    """the device's rule over the words of every sentence in text order: a word under 255 UTF-8 bytes is one entry at its first
    occurrence, its frequency its occurrence count; a word of 255 bytes or more is a new entry with frequency 1 at every
    occurrence -> [(word, frequency)] in entry order"""
    entries, at = [], {}
    for words in sent_words:
        for w in words:
            if nbytes(w) >= LONG:
                entries.append([w, 1])
            elif w in at:
                entries[at[w]][1] += 1
            else:
                at[w] = len(entries)
                entries.append([w, 1])
    return [(w, f) for w, f in entries]


def fold(entries):
    """what a Counter makes of the entries: duplicates folded into their first one (the oracle's export)"""
    out, at = [], {}
    for w, f in entries:
        if w in at:
            out[at[w]][1] += f
        else:
            at[w] = len(out)
            out.append([w, f])
    return [(w, f) for w, f in out]


def census_model(O, sents, wordpiece=False, folded=False):
    """the stream the device must export for these (lowercase) sentences; O = the oracle module, for pretokenize"""
    entries = census_entries([O.pretokenize(s) for s in sents])
    return _stream(fold(entries) if folded else entries, WP_CONT if wordpiece else 0)


class Walk:
    """what census_kernel does with a batch, from sentence offsets and bytes (the text is of ALPHABET): chunks(t) = the trips of
    tile t's chunk loop, each {cb, abase, off0, staged, last, cut, nw, giant}: cut = the absolute byte the chunk is cut at,
    nw = the word starts the chunk lists (behind the cut too), giant = (how the one-lane walk is entered: "ws", "punct" or
    "word", how it ends: "first", "ws", "punct" or "send", first byte, end)"""

    def __init__(self, sents):
        raw = [s.encode("utf-8") for s in sents]
        self.text = b"".join(raw)
        n = self.n = len(self.text)
        self.n_sent = len(raw)
        self.off = np.concatenate([[0], np.cumsum([len(r) for r in raw], dtype=np.int64)]).astype(np.int64)
        a = np.frombuffer(self.text, dtype=np.uint8)
        self.cpos = cpos = np.flatnonzero((a & 0xC0) != 0x80).astype(np.int64)
        self.cnext = np.append(cpos[1:], n)
        self.cls = cls = _CLS[a[cpos]]
        ss = np.zeros(cpos.size, dtype=bool)
        starts = self.off[:-1]
        ss[np.searchsorted(cpos, starts[starts < n])] = True
        prev = np.concatenate([[WS], cls[:-1]])[:cls.size]
        wstart = (cls != WS) & ((cls == PN) | (prev != SYM) | ss)
        self.bnd = cpos[(cls != SYM) | ss]
        self.wpos = cpos[wstart]
        stops = np.append(cpos[(cls == WS) | wstart], n)
        self.wend = stops[np.searchsorted(stops, self.wpos, side="right")]
        self.n_tiles = max(1, -(-n // TILE))
        self.plan = np.append(np.searchsorted(starts, np.arange(self.n_tiles) * TILE, side="left"), self.n_sent)

    def words(self):
        """[(first byte, bytes)] of every word occurrence, in text order"""
        return [(int(p), self.text[p:e]) for p, e in zip(self.wpos, self.wend)]

    def tile_of_sentence(self, s):
        return int(np.searchsorted(self.plan, s, side="right")) - 1

    def span(self, t):
        lo, hi = int(self.plan[t]), int(self.plan[t + 1])
        return None if lo == hi else (int(self.off[lo]), int(self.off[hi]))

    @functools.lru_cache(maxsize=None)
    def chunks(self, t):
        sp = self.span(t)
        if sp is None or self.n == 0:
            return []
        cb, end = sp
        out = []
        while True:
            abase = cb & ~15
            off0, avail = cb - abase, end - abase
            last = avail <= CAP
            staged = avail if last else CAP
            nw = int(np.searchsorted(self.wpos, abase + staged) - np.searchsorted(self.wpos, cb))
            c = {"t": t, "cb": cb, "abase": abase, "off0": off0, "staged": staged, "last": last, "cut": None, "nw": nw, "giant": None}
            out.append(c)
            if last:
                return out
            j = int(np.searchsorted(self.bnd, abase + staged - CUT_ROOM, side="right")) - 1
            if j >= 0 and self.bnd[j] > cb:
                cb = c["cut"] = int(self.bnd[j])
                continue
            c["nw"] = 0  # the word list is not used
            send = min(int(self.off[np.searchsorted(self.off, cb, side="right")]), end)
            assert send == end, "a sentence of the tile starts behind cb in a chunk without a boundary"
            ci = int(np.searchsorted(self.cpos, cb))
            if self.cls[ci] != SYM:
                c["giant"] = ("ws" if self.cls[ci] == WS else "punct", "first", cb, int(self.cnext[ci]))
            else:
                k = ci
                while k < self.cpos.size and self.cpos[k] < send and self.cls[k] == SYM:
                    k += 1
                if k < self.cpos.size and self.cpos[k] < send:
                    c["giant"] = ("word", "ws" if self.cls[k] == WS else "punct", cb, int(self.cpos[k]))
                else:
                    c["giant"] = ("word", "send", cb, send)
            cb = c["giant"][3]
            if cb >= end:
                return out

    def all_chunks(self):
        return [c for t in range(self.n_tiles) for c in self.chunks(t)]

    def counted(self):
        """the words the chunk walk inserts, in text order: [(first byte, end, "lds" or "lane")] -- the model of the walk stands
        or falls with this being words()"""
        out = []
        for c in self.all_chunks():
            if c["giant"]:
                kind, _how, b, e = c["giant"]
                if kind != "ws":
                    out.append((b, e, "lane"))
                continue
            ce = c["abase"] + c["staged"] if c["last"] else c["cut"]
            lo, hi = np.searchsorted(self.wpos, c["cb"]), np.searchsorted(self.wpos, ce)
            out += [(int(self.wpos[i]), min(int(self.wend[i]), ce), "lds") for i in range(lo, hi)]
        return out


class Batch(NamedTuple):
    name: str
    sents: list
    expect: tuple = ()  # what the models must show: see holds()


PAD_SENTENCES = 65


def padding():
    """65 one-word sentences, none of them a word of any construction (every one starts with "zq")"""
    return ["zq" + chr(97 + i // 26) + chr(97 + i % 26) for i in range(PAD_SENTENCES)]


def padded(sents):
    """the batch as the joined constructor gets it: with fewer than 65 sentences, 65 one-word sentences appended"""
    return list(sents) + (padding() if len(sents) < PAD_SENTENCES else [])


def word_of(n, salt=0, letters="abcdxyq"):
    """a word of n letters that no other (n, salt) gives"""
    k = (n * 7 + salt * 3) % len(letters)
    body = (letters[k:] + letters[:k]) * (n // len(letters) + 1)
    return (letters[salt % len(letters)] + body)[:n]


def counter_word(i, n):
    """the i-th word of n letters of a base-26 counter"""
    out = []
    for _ in range(n):
        out.append(chr(97 + i % 26))
        i //= 26
    return "".join(out)


SHORT = ("ab", "abc", "cd", "abcd", "ba", "dcab", "a", "cab", "żół", "xy")


def fill(n, rng, words=SHORT):
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


def holds(batch, walk=None, table=None):
    """asserts that the models show every event the batch is named for; -> (walk, (bits, inserts))"""
    w = walk or Walk(batch.sents)
    table = table or table_model([b for _p, b in w.words()])
    bits, ins = table
    chunks = w.all_chunks()
    for ex in batch.expect:
        kind, tag = ex[0], "%s: %r" % (batch.name, ex)
        if kind == "entries":      # the word has this many entries, each of this frequency
            _, word, n, f = ex
            got = [fr for wd, fr in census_entries([[b.decode("utf-8") for _p, b in w.words()]]) if wd == word]
            assert got == [f] * n, tag + " model %r" % (got,)
        elif kind == "chunk":      # trip idx of tile t starts at cb with off0
            _, t, idx, cb, off0 = ex
            ch = w.chunks(t)
            assert len(ch) > idx and ch[idx]["cb"] == cb and ch[idx]["off0"] == off0, tag + " model %r" % (ch[:idx + 1],)
        elif kind == "cut":        # ... and is cut at the absolute byte p
            _, t, idx, p = ex
            assert w.chunks(t)[idx]["cut"] == p and not w.chunks(t)[idx]["giant"], tag + " model %r" % (w.chunks(t)[idx],)
        elif kind == "last":       # ... and is the last one, with this many bytes staged
            _, t, idx, staged = ex
            c = w.chunks(t)[idx]
            assert c["last"] and c["staged"] == staged, tag + " model %r" % (c,)
        elif kind == "giant":      # some chunk hands (entered as, ended by, first byte, end) to one lane
            assert any(c["giant"] == ex[1:] for c in chunks), tag + " model %r" % ([c["giant"] for c in chunks if c["giant"]],)
        elif kind == "no giant":
            assert not any(c["giant"] for c in chunks), tag
        elif kind == "route":      # the word at this byte goes through LDS ("lds") or the one-lane walk ("lane")
            assert (ex[1], ex[3]) in {(b, how) for b, _e, how in w.counted()} and w.text[ex[1]:].startswith(ex[2].encode("utf-8")), tag
        elif kind == "nw":         # trip idx of tile t lists this many word starts
            _, t, idx, n = ex
            assert w.chunks(t)[idx]["nw"] == n, tag + " model %d" % w.chunks(t)[idx]["nw"]
        elif kind == "tile":       # sentence s belongs to tile t
            assert w.tile_of_sentence(ex[1]) == ex[2], tag + " model %d" % w.tile_of_sentence(ex[1])
        elif kind == "empty tiles":
            assert sum(w.span(t) is None for t in range(w.n_tiles)) >= ex[1], tag
        elif kind == "n_occ":
            assert len(ins) == ex[1], tag + " model %d" % len(ins)
        elif kind == "bits":
            assert bits == ex[1], tag + " model %d" % bits
        elif kind == "insert":     # an occurrence of the word: home slot, final slot, compares failed, long entries passed, wrapped
            _, word, home, slot, compared, long, wrapped = ex
            got = [i for i in ins if i.word == word.encode("utf-8") and i.new]
            assert len(got) == 1 and (got[0].home, got[0].slot, got[0].compared, got[0].long, got[0].wrapped) == (home, slot, compared, long, wrapped), \
                tag + " model %r" % (got,)
        elif kind == "foreign":    # some occurrence passes a slot of another tag or length
            assert any(i.foreign for i in ins), tag
        else:
            raise AssertionError("unknown expectation " + tag)
    return w, table


# ---------------------------------------------------------------------------------------------- 1. the length threshold

def threshold_batches():
    out = []
    lens = (253, 254, 255, 256)
    ws = {n: word_of(n, n) for n in lens}
    ev = tuple(("entries", ws[n], 1 if n < LONG else 3, 3 if n < LONG else 1) for n in lens)
    out.append(Batch("threshold: words of 253 .. 256 bytes, three times each, one sentence",
                     [" ".join(ws[n] for n in lens for _ in range(3)) + " ab"], expect=ev))
    out.append(Batch("threshold: words of 253 .. 256 bytes, three times each, across sentences",
                     ["ab " + " ".join(ws[n] for n in lens), " ".join(ws[n] for n in lens[::-1]) + " cd", ws[255] + " " + ws[253] + " " + ws[256] + " " + ws[254]],
                     expect=ev))
    z = {253: "a" + "ż" * 126, 254: "ż" * 127, 255: "a" + "ż" * 127, 256: "ż" * 128}
    assert all(nbytes(v) == k for k, v in z.items())
    out.append(Batch("threshold: 127 and 128 two-byte letters, and the odd lengths beside them, three times each",
                     [" ".join(z[n] for n in lens), ",".join(z[n] for n in lens), " ".join(z[n] for n in lens[::-1])],
                     expect=tuple(("entries", z[n], 1 if n < LONG else 3, 3 if n < LONG else 1) for n in lens)))
    many, exact = "ż" * 200, word_of(254, 9)  # 400 bytes in 200 code points: long; 254 code points in 254 bytes: not
    out.append(Batch("threshold: more than 254 bytes in fewer than 255 code points; 254 code points of one byte",
                     [many + " " + exact + " " + many, exact + " " + many + " " + exact],
                     expect=(("entries", many, 3, 1), ("entries", exact, 1, 3))))
    u = word_of(254, 3)
    out.append(Batch("threshold: a 254-byte word and a 255-byte word that share their first 254 bytes",
                     [u + " " + u + "x " + u, u + "x", u + "x " + u], expect=(("entries", u, 1, 3), ("entries", u + "x", 3, 1))))
    return out


# ---------------------------------------------------------------- 2. long words inside a chunk and beyond it

def long_batches():
    out = []
    for n in (400, 1000, 1020, 1021, 1022, 1023, 1024, 3000):
        w = word_of(n, n)
        # the first word opens the span at off0 0: 1,020 bytes and the space behind them are the last cut the chunk can take
        ev = [("entries", w, 2, 1), ("route", 0, w, "lds" if n <= CAP - CUT_ROOM else "lane")]
        if n > CAP - CUT_ROOM:
            ev += [("giant", "word", "ws", 0, n), ("giant", "ws", "first", n, n + 1), ("giant", "word", "ws", n + 1, 2 * n + 1)]
        elif 2 * n + 4 <= CAP:
            ev += [("last", 0, 0, 2 * n + 4), ("no giant",)]
        else:
            ev += [("cut", 0, 0, n)]
        out.append(Batch("long: a word of %d bytes, twice" % n, [w + " " + w + " ab", "cd ab"], expect=tuple(ev)))
    G, H = word_of(1500, 1), word_of(1500, 2)
    out.append(Batch("long: the walk ends at white space", ["ab cd", G + " ab"], expect=(("giant", "word", "ws", 5, 1505),)))
    out.append(Batch("long: the walk ends at punctuation", ["ab cd", G + ",ab"], expect=(("giant", "word", "punct", 5, 1505),)))
    out.append(Batch("long: the walk ends with its sentence, sentences behind it", ["ab cd", G, "ab cd", "ba"], expect=(("giant", "word", "send", 5, 1505),)))
    out.append(Batch("long: the walk ends with the tile's last sentence and the text", ["ab cd", "cd " + G],
                     expect=(("giant", "word", "send", 8, 1508),)))
    for sep, kind in ((",", "punct"), (" ", "ws")):
        out.append(Batch("long: the walk entered at a lone %r that opens the span" % sep, [sep + G + " ab", "cd"],
                         expect=(("giant", kind, "first", 0, 1), ("giant", "word", "ws", 1, 1501))))
        out.append(Batch("long: the walk entered at a lone %r behind a short word" % sep, ["ab" + sep + G + sep + "ab", "cd"],
                         expect=(("cut", 0, 0, 2), ("giant", kind, "first", 2, 3), ("giant", "word", kind, 3, 1503))))
    out.append(Batch("long: a long word followed directly by the next sentence", ["ab", G, H + " ab", G + H, "cd"],
                     expect=(("giant", "word", "send", 2, 1502), ("giant", "word", "ws", 1502, 3002), ("giant", "word", "send", 3005, 6005),
                             ("entries", G, 1, 1), ("entries", G + H, 1, 1))))
    return out


# ------------------------------------------------------------------------------------------------------ 3. the cut rule

CUT_BACK = (5, 4, 3, 1)          # the boundary at staged - d
CUT_OFF0 = (0, 1, 15)
CUT_STRADDLERS = (1, 2, 64, 300)
BRAILLE_BACK = (5, 4, 3, 2, 1)
SENT_BACK = (5, 4, 3, 1, 0, -1)  # a sentence start at staged - d: on both sides of `avail <= kWCap`


def cut_batches():
    """tile 1 opens at 512 + off0 with one word up to the boundary at abase + 1,024 - d, the straddling word behind it"""
    rng = random.Random(1024)
    out = []
    for off0 in CUT_OFF0:
        lead = fill(TILE + off0, rng)
        cb, abase = TILE + off0, TILE
        for n in CUT_STRADDLERS:
            s = word_of(n, n + off0, "xyq")
            for d in CUT_BACK:
                p = abase + CAP - d
                head = word_of(p - cb, d + off0)
                for sep, kind in ((" ", "ws"), (",", "punct")):
                    ev = [("chunk", 1, 0, cb, off0)]
                    if d >= CUT_ROOM:
                        ev += [("cut", 1, 0, p), ("route", cb, head, "lds")]
                    else:
                        ev += [("giant", "word", kind, cb, p), ("route", cb, head, "lane")]
                    out.append(Batch("cut: %s at staged - %d, off0 %d, a word of %d behind it" % (kind, d, off0, n),
                                     [lead, head + sep + s + " ab cd " + s, "ab"], expect=tuple(ev)))
            for d in SENT_BACK:
                p = abase + CAP - d
                head = word_of(p - cb, d + off0)
                # the sentence at p belongs to a later tile: the span ends there.  Up to abase + 1,024 the chunk is the last one;
                # one byte further it is not, sees no boundary and goes to the one-lane walk, which ends at the span end
                ev = [("chunk", 1, 0, cb, off0), ("last", 1, 0, CAP - d) if d >= 0 else ("giant", "word", "send", cb, p)]
                out.append(Batch("cut: a sentence start at staged - %d, off0 %d, a word of %d behind it" % (d, off0, n),
                                 [lead, head, s + " ab cd " + s, "ab"], expect=tuple(ev)))
        for d in BRAILLE_BACK:
            # U+2800 (E2 A0 80) is part of a word; staged after two of its bytes it decodes as U+00A0, white space.  The four bytes
            # of room keep that false boundary from becoming the cut: the chunk is cut at the space in front of the word
            p = abase + CAP - d
            body = fill(p - 2 - cb, rng)
            out.append(Batch("cut: a word around U+2800, its lead byte at staged - %d, off0 %d" % (d, off0),
                             [lead, body + "ab\u2800cd ab cd", "ab"], expect=(("chunk", 1, 0, cb, off0), ("cut", 1, 0, p - 3), ("entries", "ab\u2800cd", 1, 1))))
        G = word_of(1500, off0)
        for sep, kind in ((" ", "ws"), (",", "punct"), (None, "sentence start")):
            mid = ["a", G + " ab"] if sep is None else ["a" + sep + G + " ab"]
            nxt = ("giant", "word", "ws", cb + 1, cb + 1501) if sep is None else ("giant", kind, "first", cb + 1, cb + 2)
            out.append(Batch("cut: the last boundary (%s) at off0 + 1, off0 %d" % (kind, off0), [lead] + mid + ["cd"],
                             expect=(("chunk", 1, 0, cb, off0), ("cut", 1, 0, cb + 1), nxt)))
    return out


# --------------------------------------------------------------------------- 4. more than 64 word starts in a chunk

def many_words_batches():
    out = []
    for n in (65, 128, 129, 512):
        words = [chr(97 + (i * 7 + i // 26) % 26) for i in range(n)]
        out.append(Batch("k0: %d one-letter words in one chunk" % n, [" ".join(words), "ab cd"] if n < 512 else [" ".join(words)],
                         expect=(("nw", 0, 0, n + (2 if n < 512 else 0)),)))
    out.append(Batch("k0: 1,024 punctuation characters in a row", ["".join("!?.,;:-"[(i * 3 + i // 7) % 7] for i in range(CAP)) + " ab", "cd"],
                     expect=(("nw", 0, 0, CAP), ("cut", 0, 0, CAP - CUT_ROOM))))
    return out


# -------------------------------------------------------------------------------------------------------------- 5. tiles

def tile_batches():
    rng = random.Random(512)
    out = []
    for at in (511, 512, 513):
        out.append(Batch("tiles: a sentence starts at byte %d" % at, [fill(at, rng), "ab cd ab", "cd"],
                         expect=(("tile", 1, 0 if at < TILE else 1), ("tile", 2, 1))))
    out.append(Batch("tiles: one sentence spans four tiles", [fill(100, rng), fill(2100, rng), "ab cd", "ba"],
                     expect=(("tile", 1, 0), ("tile", 2, 4), ("empty tiles", 3))))
    G = word_of(1500, 5)
    out.append(Batch("tiles: empty sentences at a tile edge", [fill(TILE, rng)] + [""] * 5 + ["ab cd"] + [""] * 3 + [fill(TILE - 5, rng)] + [""] * 4 + ["ba"],
                     expect=(("tile", 1, 1), ("tile", 5, 1), ("tile", 6, 1), ("tile", 11, 2))))
    out.append(Batch("tiles: empty sentences at a chunk cut", ["ab cd"] + [""] * 5 + [G + " x"] + [""] * 2 + ["cd"],
                     expect=(("cut", 0, 0, 5), ("giant", "word", "ws", 5, 1505))))
    out.append(Batch("tiles: empty sentences at the very end", ["ab cd", "ba ab"] + [""] * 7))
    out.append(Batch("tiles: only empty and blank sentences", ["", " ", "\t", "", "  "] * 14, expect=(("n_occ", 0),)))
    out.append(Batch("tiles: one sentence with one word", ["ab"], expect=(("n_occ", 1),)))
    return out


# ----------------------------------------------------------------------------------------------------- 6. collisions

N_CANDIDATES = 1 << 20  # 2^17 give pairs (26 bits agree); a chain of three needs the 52 bits of two more words: 2^20 give about 40
CANDIDATE_LEN = 5


@functools.lru_cache(maxsize=None)
def collisions():
    """five-letter words that agree in length, tag (h >> 48) and home slot of a 1,024-slot table (h & 1023)
    -> {"pair": (a, b), "triple": (a, b, c), "wrap": (a, b) with home slot 1,023, slots: word -> home slot}"""
    i = np.arange(N_CANDIDATES, dtype=np.int64)
    words = np.stack([97 + (i // 26 ** k) % 26 for k in range(CANDIDATE_LEN)], axis=1).astype(np.uint8)
    h = word_hash_np(words)
    key = ((h >> np.uint64(TAG_SHIFT)) << np.uint64(MIN_BITS)) | (h & np.uint64((1 << MIN_BITS) - 1))
    order = np.argsort(key, kind="stable")
    ks = key[order]
    run_start = np.flatnonzero(np.concatenate([[True], ks[1:] != ks[:-1]]))
    run_len = np.diff(np.append(run_start, ks.size))

    def spell(j):
        return bytes(words[order[j]]).decode("ascii")

    groups = [tuple(spell(s + k) for k in range(n)) for s, n in zip(run_start[run_len >= 2], run_len[run_len >= 2])]
    home = lambda w: word_hash(w.encode()) & ((1 << MIN_BITS) - 1)  # noqa: E731
    pair = next(g for g in groups if len(g) == 2 and 8 < home(g[0]) < 1000)
    triple = next(g for g in groups if len(g) >= 3 and 8 < home(g[0]) < 1000 and home(g[0]) != home(pair[0]))[:3]
    wrap = next(g for g in groups if home(g[0]) == (1 << MIN_BITS) - 1)[:2]
    return {"pair": pair, "triple": triple, "wrap": wrap, "n_groups": len(groups), "slots": {w: home(w) for g in (pair, triple, wrap) for w in g}}


@functools.lru_cache(maxsize=None)
def first_byte_pair():
    """two six-letter words that differ at byte 0 ONLY and agree in tag and home slot of a 1,024-slot table: nothing but the
    compare of byte 0 tells them apart.  65,536 stems of five letters at a time, each under all 26 first letters, until one
    stem has two (325 pairs per stem, 26 bits to agree: one stem in 200,000)"""
    n_bits = np.uint64(MIN_BITS)
    for chunk in range(64):
        i = np.arange(chunk << 16, (chunk + 1) << 16, dtype=np.int64)
        stems = np.stack([97 + (i // 26 ** k) % 26 for k in range(5)], axis=1).astype(np.uint8)
        words = np.concatenate([np.repeat(np.arange(97, 123, dtype=np.uint8)[None, :, None], stems.shape[0], axis=0),
                                np.repeat(stems[:, None, :], 26, axis=1)], axis=2)
        h = word_hash_np(words.reshape(-1, 6)).reshape(-1, 26)
        key = ((h >> np.uint64(TAG_SHIFT)) << n_bits) | (h & np.uint64((1 << MIN_BITS) - 1))
        order = np.argsort(key, axis=1, kind="stable")
        ks = np.take_along_axis(key, order, axis=1)
        hit = np.argwhere((ks[:, 1:] == ks[:, :-1]) & ((ks[:, 1:] & np.uint64(1023)) > np.uint64(8)) & ((ks[:, 1:] & np.uint64(1023)) < np.uint64(1000)))
        if hit.size:
            s, j = map(int, hit[0])
            stem = bytes(stems[s]).decode("ascii")
            return chr(97 + int(order[s, j])) + stem, chr(97 + int(order[s, j + 1])) + stem
    raise AssertionError("no such pair among 4,194,304 stems")


def word_with_home(slot, n, avoid=()):
    """an ASCII word of n letters whose home slot in a 1,024-slot table is `slot`"""
    for i in range(1 << 16):
        w = counter_word(i, 4) + word_of(n - 4, i)
        if word_hash(w.encode()) & ((1 << MIN_BITS) - 1) == slot and w not in avoid:
            return w
    raise AssertionError("no word of %d letters with home slot %d" % (n, slot))


def collision_batches():
    c = collisions()
    home = c["slots"]
    out = []
    a, b = c["pair"]
    out.append(Batch("collision: two words of one tag, length and home slot", [a + " " + b + " " + a, b + " ab " + b + " " + a],
                     expect=(("bits", MIN_BITS), ("insert", a, home[a], home[a], 0, 0, False), ("insert", b, home[b], home[b] + 1, 1, 0, False),
                             ("entries", a, 1, 3), ("entries", b, 1, 3))))
    a, b = first_byte_pair()
    ha = word_hash(a.encode()) & 1023
    out.append(Batch("collision: two such words that differ at byte 0 only", [a + " " + b + " " + a, b + " ab " + b + " " + a],
                     expect=(("bits", MIN_BITS), ("insert", a, ha, ha, 0, 0, False), ("insert", b, ha, ha + 1, 1, 0, False),
                             ("entries", a, 1, 3), ("entries", b, 1, 3))))
    a, b, d = c["triple"]
    out.append(Batch("collision: a chain of three such words", [a + " " + b + " " + d, d + " " + b + " " + a + " " + d],
                     expect=(("bits", MIN_BITS), ("insert", b, home[a], home[a] + 1, 1, 0, False), ("insert", d, home[a], home[a] + 2, 2, 0, False),
                             ("entries", d, 1, 3))))
    a, b = c["wrap"]
    out.append(Batch("collision: a pair at home slot 1,023, the probe wraps to slot 0", [a + " " + b, b + " " + a + " " + b],
                     expect=(("bits", MIN_BITS), ("insert", a, 1023, 1023, 0, 0, False), ("insert", b, 1023, 0, 1, 0, True), ("entries", b, 1, 3))))
    slot = 700
    big, small, other = word_with_home(slot, LONG), word_with_home(slot, 6), word_with_home(slot, 7)
    out.append(Batch("collision: a short word whose home slot a 255-byte entry took first",
                     [big + " " + small, other + " " + small + " " + big + " " + other],
                     expect=(("bits", MIN_BITS), ("insert", small, slot, slot + 1, 0, 1, False), ("insert", other, slot, slot + 2, 0, 1, False),
                             ("foreign",), ("entries", big, 2, 1), ("entries", small, 1, 2))))
    return out


# ----------------------------------------------------------------------------------------------------- 7. table size

def table_batches():
    out = []
    for n in (504, 505):
        words = [counter_word(i * 37, 4) for i in range(n)]
        assert len(set(words)) == n
        sents = [" ".join(words[i:i + 7]) for i in range(0, n, 7)]
        out.append(Batch("table: %d occurrences, all distinct" % n, sents, expect=(("n_occ", n), ("bits", 10 if n == 504 else 11))))
        half = [counter_word(i * 41 + 5, 4) for i in range(252)]
        occ = half + half[::-1] + (["solo"] if n == 505 else [])
        sents = [" ".join(occ[i:i + 7]) for i in range(0, len(occ), 7)]
        out.append(Batch("table: %d occurrences, every word twice%s" % (n, " but one" if n == 505 else ""), sents,
                         expect=(("n_occ", n), ("bits", 10 if n == 504 else 11), ("entries", half[0], 1, 2))))
    assert all(len(b.sents) >= PAD_SENTENCES for b in out)  # no padding: the joined form sits on the same step
    return out


# ------------------------------------------------------------------------------------------ 8. contention and order

def contention_batch():
    """about 64 KB: 300 distinct words in a few thousand shuffled sentences; "the" holds half of all occurrences, and half of the
    other words occur only in the last quarter of the text"""
    rng = random.Random(300)
    words = [counter_word(i * 53 + 11, 3 + i % 6) for i in range(299)]
    assert len(set(words)) == 299 and "the" not in words
    early, late = words[:150], words[150:]
    sents = []
    for k in range(3000):
        pool = early if k < 2250 else words
        sent = []
        for _ in range(rng.randrange(2, 7)):
            sent.append("the" if rng.random() < 0.52 else rng.choice(pool))
        sents.append(" ".join(sent))
    for i, w in enumerate(early):  # every word occurs
        sents[i] += " " + w
    for i, w in enumerate(late):
        sents[2250 + i] += " " + w
    head, tail = sents[:2250], sents[2250:]
    rng.shuffle(head)
    rng.shuffle(tail)
    return Batch("contention: 300 words, one of them half of all occurrences, half of them first seen in a late tile", head + tail), late


CENSUS_FAMILIES = {"threshold": threshold_batches, "long": long_batches, "cut": cut_batches, "many words": many_words_batches,
                   "tiles": tile_batches, "collisions": collision_batches, "table": table_batches,
                   "contention": lambda: [contention_batch()[0]]}
MERGE_FAMILIES = ("threshold", "long")  # NaiveBPE.train to 30 merges over these


@functools.lru_cache(maxsize=None)
def census_batches(family):
    return tuple(CENSUS_FAMILIES[family]())


def has_long(sents):
    return any(len(b) >= LONG for _p, b in Walk(sents).words())


# ======================================================================================================= the histogram

def mh_bucket(idx):
    """home slot of a counter index in a wave's table: the top 10 bits of the 32-bit product"""
    return ((np.asarray(idx, dtype=np.uint64) * np.uint64(MH_MUL)) & np.uint64(0xFFFFFFFF)) >> np.uint64(MH_SHIFT)


def mh_stretch_model(idx):
    """one wave's table over one stretch of counter indexes, in order (the device's order is a race; with every key in ONE home
    slot the outcome is not: the first 8 keys take the 8 slots the probes reach) -> (slots in use, ids given up to the global
    array, whether a probe went from slot 1,023 to slot 0)"""
    keys, given_up, wrapped = {}, 0, False
    for x in map(int, idx):
        h = int(mh_bucket(x))
        for _ in range(MH_PROBES):
            if keys.setdefault(h, x) == x:
                break
            wrapped |= h == MH_SLOTS - 1
            h = (h + 1) & (MH_SLOTS - 1)
        else:
            given_up += 1
    return len(keys), given_up, wrapped


class HistCase(NamedTuple):
    name: str
    ids: np.ndarray   # uint32, BPE_CONT = bit 31
    id_cap: int
    given_up: object = None  # None: not modelled; else (at least this many ids go straight to the global array, a probe wraps or None)


CONT = 0x80000000


def _ids_of(idx, id_cap):
    idx = np.asarray(idx, dtype=np.int64)
    return np.where(idx >= id_cap, (idx - id_cap) | CONT, idx).astype(np.uint32)


def hist_want(ids, id_cap):
    """(counts uint64[2 * id_cap], out of range) by np.bincount over sym + id_cap * flag"""
    ids = np.asarray(ids, dtype=np.uint32)
    sym = (ids & np.uint32(0x7FFFFFFF)).astype(np.int64)
    ok = sym < id_cap
    idx = sym[ok] + id_cap * (ids[ok] >> np.uint32(31)).astype(np.int64)
    return np.bincount(idx, minlength=2 * id_cap).astype(np.uint64), int(ids.size - np.count_nonzero(ok))


HIST_LENGTHS = (1, 63, 64, 65, MH_STRETCH - 1, MH_STRETCH, MH_STRETCH + 1, MH_BLOCK - 1, MH_BLOCK, MH_BLOCK + 1)
BUCKET_CAP = 1 << 20  # id_cap of the crowded stretches: 2^21 counter indexes, 2,048 per home slot


def bucket_members(bucket, k):
    """k counter indexes below 2 * BUCKET_CAP whose home slot is `bucket`, from both halves of the counter array"""
    idx = np.arange(2 * BUCKET_CAP, dtype=np.int64)
    m = idx[mh_bucket(idx) == bucket]
    lo, hi = m[m < BUCKET_CAP], m[m >= BUCKET_CAP]
    assert lo.size >= k and hi.size >= k
    return np.concatenate([lo[:k - k // 2], hi[:k // 2]])


@functools.lru_cache(maxsize=None)
def hist_cases():
    rng = np.random.default_rng(4096)
    out = []
    for n in HIST_LENGTHS:
        ids = rng.integers(0, 3000, size=n).astype(np.uint32) | np.where(rng.random(n) < 0.3, CONT, 0).astype(np.uint32)
        out.append(HistCase("length %d" % n, ids, 3000))
    idx = rng.permutation(2 * 5000)[:MH_STRETCH]
    out.append(HistCase("one stretch of 4,096 distinct ids", _ids_of(idx, 5000), 5000, (MH_STRETCH - MH_SLOTS, None)))
    for bucket in (5, 1020):
        for k in (8, 9, 40):
            members = bucket_members(bucket, k)
            idx = np.concatenate([members, members[rng.integers(0, k, size=MH_STRETCH - k)]])
            out.append(HistCase("a stretch of %d distinct ids, all of home slot %d" % (k, bucket), _ids_of(idx, BUCKET_CAP), BUCKET_CAP,
                                (0 if k <= MH_PROBES else 1, bucket + MH_PROBES > MH_SLOTS)))
    out.append(HistCase("one symbol with and without the flag", np.array([7, 7 | CONT, 7, 7 | CONT, 7 | CONT, 3], dtype=np.uint32), 10))
    out.append(HistCase("id_cap 1", np.array([0, CONT, 0, 0, CONT], dtype=np.uint32), 1))
    out.append(HistCase("sym == id_cap - 1 on both halves", np.array([999, 999 | CONT, 0, CONT, 999, 999 | CONT, 999 | CONT], dtype=np.uint32), 1000))
    ids = rng.integers(0, 1001, size=5000).astype(np.uint32) | np.where(rng.random(5000) < 0.5, CONT, 0).astype(np.uint32)
    out.append(HistCase("id_cap 1,001, not a power of two", ids, 1001))
    return tuple(out)


def hist_out_of_range_case():
    """sym == id_cap among valid ids, with and without the flag, and larger ones: (ids, id_cap, how many are out of range)"""
    rng = np.random.default_rng(77)
    ids = rng.integers(0, 600, size=9000).astype(np.uint32) | np.where(rng.random(9000) < 0.5, CONT, 0).astype(np.uint32)
    bad = np.array([600, 600 | CONT, 601, 0x7FFFFFFF, 0xFFFFFFFF, 600, 600], dtype=np.uint32)
    at = np.array([0, 63, 64, 4095, 4096, 8191, 8999])
    ids[at] = bad
    return ids, 600, int(bad.size)


SECOND_STRETCH_N = MH_SECOND + MH_STRETCH + 1
SECOND_STRETCH_CAP = 1 << 16


def second_stretch_ids():
    """33,558,529 ids, heavy-headed (the product of two uniform 16-bit numbers, its top 16 bits): wave 0 takes a second stretch of
    4,096 ids and wave 1 one of a single id.  134 MB: built once, by the one test that needs it"""
    rng = np.random.default_rng(2048)
    x = rng.integers(0, 1 << 32, size=SECOND_STRETCH_N, dtype=np.uint32)
    ids = ((x >> np.uint32(16)) * (x & np.uint32(0xFFFF))) >> np.uint32(16)
    ids |= (x & np.uint32(0x100)) << np.uint32(23)  # the flag on about half of them
    return ids


def hist_waves(n):
    """(blocks, waves, stretches of the busiest wave) of a histogram call over n ids"""
    blocks = min(-(-n // MH_BLOCK), MH_MAX_BLOCKS)
    waves = blocks * (MH_THREADS // 64)
    stretches = -(-n // MH_STRETCH)
    return blocks, waves, -(-stretches // waves) if n else 0


# ===================================================================================================== the equivalence

# period 7.  Kinds 0 and 3 sit at 0, 3, 5 and kind 1 at 1, 2, 6: the differences cover 1 .. 6, so whatever the number of waves is
# modulo 7, some wave goes from a row that inserted X to a row that probes for it
TE_KINDS = (0, 1, 1, 3, 2, 0, 1)
TE_V = 6000                       # ids of both sides; canonical id = id + TE_CANON
TE_CANON = 1000


def te_wave_keys(ra, rb, n_waves):
    """the most distinct tokens the rows of one wave insert between them (the shorter side, A when they tie): under 512, a
    wave's table has an empty slot even if nothing ever cleared it"""
    worst = 0
    for w in range(min(n_waves, len(ra))):
        keys = set()
        for r in range(w, len(ra), n_waves):
            keys.update(map(int, ra[r] if len(ra[r]) <= len(rb[r]) else rb[r]))
        worst = max(worst, len(keys))
    return worst


def te_side(rows):
    """rows of ids -> the side tuple of _native.token_equivalence: (ids, offsets, map, map_base, flagged)"""
    off = np.zeros(len(rows) + 1, dtype=np.uint64)
    np.cumsum([len(r) for r in rows], out=off[1:])
    ids = np.concatenate([np.asarray(r, dtype=np.uint32) for r in rows]) if rows else np.zeros(0, dtype=np.uint32)
    return ids.astype(np.uint32), off, (np.arange(TE_V) + TE_CANON).astype(np.uint32), 0, False


def te_brute(a, b):
    """benchmarks.py:148-156 and :166 for one row (the Counter restatement of tests/test_gpu_equivalence.py; the canonical map
    is a shift, so the ids themselves are compared)"""
    n = min(len(a), len(b))
    f1, f2 = Counter(map(int, a)), Counter(map(int, b))
    return (n, sum(1 for i in range(n) if a[i] == b[i]), sum(min(f1[t], f2[t]) for t in f1.keys() & f2.keys()), 1 if f1.keys() & f2.keys() else 0)


def te_wave_geometry(n_rows, n_cu):
    blocks = min(-(-n_rows // (TE_THREADS // 64)), TE_WAVE_BLOCKS_PER_CU * n_cu)
    return blocks, blocks * (TE_THREADS // 64)


def te_wave_rows(n_cu):
    """2 * 32 * n_cu + 5 rows whose kinds cycle with period 7: a wave's second and third row are of another kind than the one
    before.  Every row draws on the same eight tokens X: kind 0 has X on both sides (A rotated by the row number), kind 1 the
    same B side and a disjoint A side, kind 2 an empty A side, kind 3 256 tokens (X among them) against 300.  The last five rows,
    the third of waves 0 .. 4, leave the cycle: kind 1 behind a kind 0 or 3, else kind 3.
    -> (rows of A, rows of B, kinds, want int64[n_rows, 4])"""
    n_waves = 32 * n_cu
    n_rows = 2 * n_waves + 5
    rng = np.random.default_rng(7)
    X = np.array([11, 12, 13, 14, 15, 16, 17, 11], dtype=np.uint32)  # 11 twice: a multiset
    Y = np.arange(100, 108, dtype=np.uint32)
    big_a = [np.concatenate([X, rng.permutation(np.arange(200, 2000))[:TE_WAVE_CAP - 8].astype(np.uint32)]) for _ in range(3)]
    big_b = [np.concatenate([rng.permutation(a)[:150], X[:4], rng.integers(2000, 3000, size=146).astype(np.uint32)]) for a in big_a]
    ra, rb, kinds, want, memo = [], [], [], [], {}
    for r in range(n_rows):
        k = TE_KINDS[r % len(TE_KINDS)]
        if r >= 2 * n_waves:  # the five third rows: probe for X where the wave's second row inserted it, insert it elsewhere
            k = 1 if kinds[r - n_waves] in (0, 3) else 3
        if k == 0:
            key, a, b = (0, r % 8), np.roll(X, r % 8), X
        elif k == 1:
            key, a, b = (1, r % 3), Y[:8 - r % 3], X
        elif k == 2:
            key, a, b = (2, 0), Y[:0], X
        else:
            key, a, b = (3, r % 3), big_a[r % 3], big_b[r % 3]
        if key not in memo:
            memo[key] = te_brute(a, b)
        ra.append(a)
        rb.append(b)
        kinds.append(k)
        want.append(memo[key])
    return ra, rb, np.array(kinds), np.array(want, dtype=np.int64)


def te_small_want(A, la, B, lb, universe):
    """the four values of rows of at most two tokens, vectorised: A, B int64[n, 2], la, lb their lengths"""
    m = np.minimum(la, lb)
    pm = ((A[:, 0] == B[:, 0]) & (m >= 1)).astype(np.int64) + ((A[:, 1] == B[:, 1]) & (m >= 2))
    un = np.zeros(A.shape[0], dtype=np.int64)
    for v in universe:
        ca = ((A[:, 0] == v) & (la >= 1)).astype(np.int64) + ((A[:, 1] == v) & (la >= 2))
        cb = ((B[:, 0] == v) & (lb >= 1)).astype(np.int64) + ((B[:, 1] == v) & (lb >= 2))
        un += np.minimum(ca, cb)
    return np.stack([m, pm, un, (un > 0).astype(np.int64)], axis=1)


def te_first_parts(ids, depth):
    """distinct keys per part of the first partition of a row: the top `depth` bits of te_hash (canonical id * 2654435761)"""
    c = np.unique(np.asarray(ids, dtype=np.uint64)) + np.uint64(TE_CANON)
    h = (c * np.uint64(MH_MUL)) & np.uint64(0xFFFFFFFF)
    return np.bincount((h >> np.uint64(32 - depth)).astype(np.int64), minlength=1 << depth)


def te_block_long_positions(n_cu):
    """rows of the long ones: in-tile positions 0, 1 and 1,023 of tile 0, positions 0 and 1,023 of tile n_cu (the second tile of
    workgroup 0), and one in the last, partial tile"""
    T = TE_BLOCK_THREADS
    return [0, 1, T - 1, n_cu * T, n_cu * T + T - 1, (n_cu + 1) * T + 3]


def te_block_rows(n_cu):
    """1,024 * n_cu + 1,030 rows of 0 to 2 tokens of six, and six long rows (te_block_long_positions), the fourth of them with
    4,096 distinct keys on its shorter side (te_first_parts: one of its two first parts holds more than 2,048) -> (side a, side b, want int64[n_rows, 4], the long rows)"""
    n_rows = TE_BLOCK_THREADS * n_cu + 1030
    rng = np.random.default_rng(1030)
    universe = np.arange(20, 26)
    A, B = rng.choice(universe, size=(n_rows, 2)), rng.choice(universe, size=(n_rows, 2))
    la, lb = rng.integers(0, 3, size=n_rows), rng.integers(0, 3, size=n_rows)
    longs = te_block_long_positions(n_cu)
    la[longs] = lb[longs] = 0
    for r in longs:  # a short row of two tokens on both sides directly behind every long one (row 1 is long itself)
        if r + 1 not in longs:
            la[r + 1] = lb[r + 1] = 2
    want = te_small_want(A, la, B, lb, universe)

    def csr(M, ln, extra):
        cnt = ln.copy()
        for r, row in extra.items():
            cnt[r] = len(row)
        off = np.zeros(n_rows + 1, dtype=np.uint64)
        np.cumsum(cnt, out=off[1:])
        ids = np.zeros(int(off[-1]), dtype=np.uint32)
        row = np.repeat(np.arange(n_rows), ln)
        col = np.arange(row.size) - np.repeat(np.cumsum(ln) - ln, ln)
        ids[off[:-1].astype(np.int64)[row] + col] = M[row, col]
        for r, row in extra.items():
            ids[int(off[r]):int(off[r + 1])] = row
        return ids, off, (np.arange(TE_V) + TE_CANON).astype(np.uint32), 0, False

    xa, xb = {}, {}
    for k, r in enumerate(longs):
        if k == 3:
            a = rng.permutation(TE_V)[:2 * TE_BLOCK_CAP].astype(np.uint32)  # 4,096 distinct keys in two parts: the fuller one splits
            b = np.concatenate([rng.permutation(a)[:4000], rng.integers(0, TE_V, size=600).astype(np.uint32)])
        else:
            n = TE_WAVE_CAP + 1 + 40 * k
            a = rng.integers(0, 900, size=n).astype(np.uint32)
            b = np.concatenate([a[:n // 2], rng.integers(0, 900, size=n // 2 + 30 + k).astype(np.uint32)])
        if k % 2:
            a, b = b, a
        xa[r], xb[r] = a, b
        want[r] = te_brute(a, b)
    return csr(A, la, xa), csr(B, lb, xb), want, longs
