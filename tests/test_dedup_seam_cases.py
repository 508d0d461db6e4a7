"""The conditions that keep tests/test_gpu_dedup_seams.py from being hollow, checked without a GPU: the constants the
constructions are laid out by are the kernels', every construction reaches the seam it is named for in the model of
tests/dedup_seam_cases.py, and the oracle sees in the handmade table what the cases suppose."""
import json
import os
import re
import time

import pytest

from tests import dedup_seam_cases as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "subword-tokenizers_amd", "csrc")
ALL = list(D.FAMILIES) + ["counter"]


@pytest.fixture(scope="module", autouse=True)
def started():
    """when the first test of this file began"""
    return time.monotonic()


def read(name):
    with open(os.path.join(CSRC, name), encoding="utf-8") as f:
        return f.read()


def test_constants_are_the_kernels():
    """the seams sit where these say; if the kernels' constants move, the cases have to move with them"""
    dd, hdr, enc = read("swt_dedup.hip"), read("swt_dedup.h"), read("swt_bpe_encode.hip")

    def num(src, pattern):
        return [int(x) for x in re.findall(pattern, src)]

    assert num(dd, r"#define SWT_DTILE (\d+)") == [D.TILE]
    assert num(dd, r"#define SWT_DCAP (\d+)") == [D.CAP]
    assert "kDTile = SWT_DTILE" in dd and "kDCap = SWT_DCAP" in dd
    assert num(dd, r"kDdMaxProbes = (\d+);") == [D.MAX_PROBES]
    own = num(dd, r"if \(len >= (\d+)u\) \{ is_new = true; return dd_own_slot")
    assert own == [D.OWN_LEN, D.OWN_LEN]  # the one-lane form and the LDS form
    assert "p + 4 <= staged" in dd and "staged - 3u" in dd and D.CUT_ROOM == 4
    assert "const uint64_t abase = cb & ~15ull;" in dd
    assert num(enc, r"constexpr uint64_t kUMaxTiles = (\d+);") == [D.U_MAX_TILES]
    assert "(ut == 64 || ut == 128) ? (uint32_t)ut : 256u" in enc and D.U_TILES == (64, 128, 256)
    assert num(dd, r"new_blk_base\[t >> (\d+)\]") == [10] and num(dd, r"blk_base\[t >> (\d+)\]").count(10) >= 2
    assert num(dd, r"nb_new = \(n_tiles \+ 1023\) / (\d+);") == [D.SCAN_BLOCK] and 1 << 10 == D.SCAN_BLOCK
    assert re.search(r"kDirectBytes = (\d+), kDirectSents = (\d+);", enc).groups() == (str(D.DIRECT_BYTES), str(D.DIRECT_SENTS))
    # what the model takes from the header and the host half
    assert "kDedupMinBytes = 7u << 18" in hdr
    assert "mode == kDedupWp ? 0u : 1u" in dd and "span_base >> 1" in dd


def test_model_classes_are_the_library_classes(native):
    """the model's white space and punctuation, for every character the cases use, against the library's class table"""
    chars = set()
    for family in D.FAMILIES:
        for b in D.batches(family):
            chars.update("".join(b.sents))
    for ch in sorted(chars):
        c = native.lib().swt_class_of(ord(ch))  # SWT_CLS_BERT_WS 1, SWT_CLS_BERT_PUNCT 2
        got = D.WS if c & 1 else (D.PN if c & 2 else D.SYM)
        assert got == D.classify(ord(ch)), "U+%04X" % ord(ch)


def test_handmade_table(oracle):
    assert D.is_proper(D.HANDMADE)
    assert not D.is_proper(D.HANDMADE[::-1]) and not D.is_proper(D.HANDMADE + D.HANDMADE[:1])
    assert set("".join(l + r for l, r in D.HANDMADE)) <= set("abcdxyżółq")
    orc = oracle.OracleBPE(D.HANDMADE)
    assert len(D.CHAIN) == 12 and orc.encode_word(D.CHAIN) == [D.CHAIN]
    assert len(orc.encode_word(D.STUBBORN)) >= 5
    ids, off = orc.tokenize_batch_ids(["ab " + D.CHAIN + " " + D.STUBBORN])
    assert ids.size == 1 + 1 + len(D.STUBBORN)


def test_hash_model_is_the_kernels():
    """the arithmetic of dd_hash, constant by constant (the tag collisions of the compare family rest on it)"""
    dd = read("swt_dedup.hip")
    for c in ("0x9E3779B97F4A7C15ull", "0xff51afd7ed558ccdull", "0xc4ceb9fe1a85ec53ull", "0x94d049bb133111ebull", "h ^= h >> 32;",
              "h ^= h >> 29;", "(unsigned long long)n << 56", "(h >> 40) & 0xFFull"):
        assert c in dd, c
    assert D.dd_hash(b"ab") != D.dd_hash(b"ba") and D.dd_hash(b"a" * 17)[0] != D.dd_hash(b"a" * 16 + b"b")[0]


def test_compare_words_differ_at_one_byte():
    sets = D.compare_sets()
    assert {(L, k) for L, k, _, _ in sets} == {(L, k % L) for L in D.COMPARE_L for k in D.COMPARE_K if k < L}
    # every position but the top byte of the last eight bytes the hash takes in has a pair that only the compare tells apart
    assert {(L, k) for L, k, _, collide in sets if not collide} == {(16, 15), (24, 23), (40, 39)}
    for L, k, trio, collide in sets:
        assert len(set(trio)) == 3
        for w in trio:
            assert len(w.encode()) == L
        for a in trio:
            for b in trio:
                assert a == b or [i for i in range(L) if a[i] != b[i]] == [k], (L, k)
        if not collide:
            continue
        assert D.dd_hash(trio[0].encode())[1] == D.dd_hash(trio[1].encode())[1]
        assert D.dd_hash(trio[0].encode())[0] & 15 == D.dd_hash(trio[1].encode())[0] & 15  # one home slot under table bits 4
        assert D.dd_hash(trio[0].encode())[0] != D.dd_hash(trio[1].encode())[0]


def test_every_construction_reaches_its_seam():
    """the model shows the event each batch is named for, and what the geometry allows holds in all of them"""
    n_batches = n_bytes = 0
    giants = {"ws": 0, "punct": 0, "symbol": 0, "word": 0}
    for family in ALL:
        names = set()
        for b in D.batches(family):
            size = sum(map(D.nbytes, b.sents))
            assert size <= 1_200_000, b.name
            assert b.name not in names, b.name
            names.add(b.name)
            assert all(s == s.lower() for s in b.sents)
            if family in D.CHUNK_END or family in ("giant", "one symbol"):
                assert b.expect or "small call" in b.name or "symbol" in family, b.name
            w = D.holds(b)
            n_batches += 1
            n_bytes += size
            for t in range(w.n_tiles):
                for c in w.chunks(t):
                    if c["giant"]:
                        giants[c["giant"][0]] += 1
                    else:
                        assert c["last"] or c["off0"] < c["cut"] - c["abase"] <= c["staged"] - D.CUT_ROOM
            if size < 100_000:
                for s in range(w.n_sent):
                    assert w.sent_word(s) <= D.TILE < D.CAP, b.name
    print("%d batches, %d bytes; one-lane trips: %r" % (n_batches, n_bytes, giants))
    assert min(giants[k] for k in ("ws", "punct", "word")) >= 4
    # the parts leave nothing out
    for family in D.FAMILIES:
        assert sum(len(D.part(family, k)) for k in range(D.PARTS.get(family, 1))) == len(D.batches(family))


def test_chunk_end_sweep_is_complete():
    both = [b for f in D.CHUNK_END for b in D.batches(f)]
    names = {b.name for b in both}
    assert len(names) == 2 * len(D.OFF0) * len(D.STRADDLERS) * 11
    walked = 0
    for b in both:
        if "sentence" in b.name:
            continue
        m = re.match(r"chunk end (\d): (.*) at end ([-+]\d+), off0 (\d+)", b.name)
        which, d, p = int(m.group(1)) - 1, int(m.group(3)), int(m.group(4))
        w = D.Walk(b.sents)
        c = w.chunks(1)[which]
        s = dict(D.STRADDLERS)[m.group(2)].encode("utf-8")
        at = c["abase"] + D.CAP + d
        assert w.text[at:at + len(s)] == s and c["off0"] == p and not c["last"]
        walked += 1
    assert walked == 2 * len(D.OFF0) * (len(D.STRADDLERS) - 2) * 11


def test_density_tiles_hold_span_over_two_distinct_tabled_words():
    for b in D.batches("density"):
        if "512" not in b.name:
            continue
        w = D.Walk(b.sents)
        for t in (1, 2):
            lo, hi = w.span(t)
            words = w.tabled(t)
            assert (hi - lo) % 2 == 0 and len(words) == len(set(words)) == (hi - lo) // 2 == 512
            assert w.n_words(t) == 512
        assert (w.span(1)[0] % 2 == 1) == ("odd" in b.name)


def test_oracle_work_is_short(oracle):
    """the C oracle over every batch, under both tables"""
    merges = [tuple(m) for m in json.load(open(os.path.join(ROOT, "tests", "golden", "ref", "resources", "pretrained", "FastBPE", "merges.json"), encoding="utf-8"))]
    t0 = time.monotonic()
    for table in (D.HANDMADE, merges):
        orc = oracle.OracleBPE(table)
        made = time.monotonic()
        for family in ALL:
            for b in D.batches(family):
                ids, off = orc.tokenize_batch_ids(b.sents)
                assert off.size == len(b.sents) + 1 and int(off[-1]) == ids.size
        print("oracle over every batch: %.2f s (table of %d merges)" % (time.monotonic() - made, len(table)))
    assert time.monotonic() - t0 < 30


def test_this_file_is_quick(started):
    """runs last: everything above, the generators included, within a minute"""
    assert time.monotonic() - started < 60
