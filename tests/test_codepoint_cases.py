"""The self-check of tests/codepoint_cases.py, on the CPU: the oracle agrees with the fixtures on every code point, the position
family reaches every seam it names, and the edge set holds both sides of every edge.  tests/test_gpu_codepoints.py compares the
device with the oracle on these inputs; this file is why that comparison says something about the fixtures too.

Measured on the CPU (one core): S1 (1,114,111 sentences, 8.8 MB) through OracleBPE 0.4 s and through OracleWP 0.5 s, building and
packing it 1.3 s; S16 (69,632 sentences, 5.6 MB) through OracleBPE 0.1 s, through the trainer's census 0.1 s (BPE) and 0.7 s
(WordPiece); P is 528 batches of 1.1 MB together, built in 0.1 s.  The whole file runs in 3 s."""
import unicodedata

import numpy as np

from tests import codepoint_cases as K

A, B = ord("a"), ord("b")


def test_constants_are_the_kernels():
    """the seams of P sit where these say; if a kernel's constants move, codepoint_cases.py has to move with them"""
    assert K.constants() == K.EXPECTED_CONSTANTS
    assert K.constants()["kClsLds"] == K.constants()["kWpClsLds"] == 0x400  # the LDS cut-off that E names


def test_classes_are_disjoint_where_the_expectations_need_it():
    tab = K.class_table()
    assert not np.any((tab & K.WS != 0) & (tab & K.PUNCT != 0))
    assert not np.any((tab & K.SPACE != 0) & (tab & K.ALNUM != 0))


def test_oracle_bpe_agrees_with_the_fixtures_on_s1(oracle):
    """bert_ws: two words; bert_punct: three, the character on its own; otherwise one word of five symbols with the lowered
    code point in the middle -- continuation flags included.  (No merges: a token is a code point.)"""
    tab, low = K.class_table(), K.lower_table()
    orc = oracle.OracleBPE([])
    ids, off = K.oracle_bpe(oracle, orc, K.s1_lowered())
    lo = low[1:].astype(np.uint32)
    c = tab[lo]
    ws, punct = (c & K.WS) != 0, (c & K.PUNCT) != 0
    n = lo.size
    m = np.empty((n, 5), dtype=np.uint32)
    m[:, 0], m[:, 1], m[:, 4] = A, B | K.CONT, B | K.CONT
    m[:, 2] = np.where(punct, lo, lo | K.CONT)
    m[:, 3] = np.where(ws | punct, A, A | K.CONT)
    keep = np.ones((n, 5), dtype=bool)
    keep[:, 2] = ~ws
    want_off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(keep.sum(axis=1), out=want_off[1:])
    assert np.array_equal(off, want_off)
    assert np.array_equal(ids, m[keep])
    counts = K.fixture("unicode_classes.json")["meta"]["counts"]
    assert int(ws.sum()) == counts["bert_ws"] == 25 and int(punct.sum()) == counts["bert_punct"] == 726
    # the 26 host code points: S1's sentence holds them unlowered above, which checks their class; their lowercase is this
    # interpreter's, and is compared only when it follows the fixture's Unicode version
    checked = 0
    if unicodedata.unidata_version == K.fixture("unicode_lower.json")["meta"]["unidata"]:
        for cp in sorted(K.host_cps()):
            text = ("ab" + chr(cp) + "ab").lower()
            got = orc.tokenize_ids("ab" + chr(cp) + "ab")
            want = [ord(ch) | (K.CONT if k else 0) for w in K.split_words(text) for k, ch in enumerate(w)]
            assert got.tolist() == want, hex(cp)
            checked += 1
        assert checked == 26  # nothing is left out under the fixture's Unicode version; under another one, these 26 and no more


WP_VOCAB = ["a", "b", "##a", "##b", ".", "[UNK]"]


def test_oracle_wp_agrees_with_the_fixtures_on_s1(oracle):
    """FastWP on "ab" + c + "ab" with a vocabulary that knows a, b and '.': a py_space character parts two words; an alphanumeric
    one that the vocabulary lacks makes the whole run ['UNK']; any other character is a word boundary, and behind it the
    reference never returns (status 1) unless the trie has an edge for it at the root ('.', and '[' and '#', which vanish)."""
    tab, low = K.class_table(), K.lower_table()
    orc = oracle.OracleWP(WP_VOCAB)
    v = {t: i for i, t in enumerate(WP_VOCAB)}
    unk = len(WP_VOCAB)
    ids, off, status = K.oracle_wp(oracle, orc, K.s1_lowered())
    lo = low[1:]
    c = tab[lo]
    space, alnum = (c & K.SPACE) != 0, (c & K.ALNUM) != 0
    n = lo.size
    two = [v["a"], v["##b"], v["a"], v["##b"]]
    want_status = np.where(space | alnum, 0, 1).astype(np.uint8)
    counts = np.where(space, 4, np.where(alnum, 1, 0))
    special = {A: [v["a"], v["##b"], v["##a"], v["##a"], v["##b"]], B: [v["a"], v["##b"], v["##b"], v["##a"], v["##b"]],
               ord("."): [v["a"], v["##b"], v["."], v["a"], v["##b"]], ord("["): two, ord("#"): two}
    for cp, toks in special.items():
        for i in np.flatnonzero(lo == cp):
            counts[i], want_status[i] = len(toks), 0
    want_off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(counts, out=want_off[1:])
    assert np.array_equal(status, want_status)
    assert np.array_equal(off, want_off)
    flat = np.full(int(want_off[-1]), unk, dtype=np.uint32)
    for i in np.flatnonzero(space):
        flat[int(want_off[i]):int(want_off[i + 1])] = two
    for cp, toks in special.items():
        for i in np.flatnonzero(lo == cp):
            flat[int(want_off[i]):int(want_off[i + 1])] = toks
    assert np.array_equal(ids, flat)


def test_edge_set_holds_both_sides_of_every_edge():
    e = set(K.edge_set())
    fx = K.fixture("unicode_classes.json")
    n_edges = 0
    for name, _bit in K.CLASS_NAMES:
        for lo, hi in fx[name]:
            for cp in (lo - 1, lo, hi, hi + 1):
                if 1 <= cp < K.N_CP:
                    assert cp in e, (name, hex(cp))
                    n_edges += 1
    lw = K.fixture("unicode_lower.json")
    assert all(s in e and d in e for s, d in lw["pairs"]) and e >= set(lw["host"])
    assert e >= {0x7F, 0x80, 0x7FF, 0x800, 0xFFFF, 0x10000, 0x10FFFF, 0x3FF, 0x400, 0xD7FF, 0xD800, 0xDFFF, 0xE000}
    assert 2000 < len(e) < 8000, len(e)
    print("E: %d code points, %d range edges" % (len(e), n_edges))


def test_every_class_and_length_of_the_fixtures_is_in_p():
    pairs = K.kind_lengths()
    # what the issue names must be there: letters of 2, 3 and 4 bytes, a cased letter of 4, bert_ws / py_space of 2 and 3,
    # bert_punct of 2, 3 and 4
    for key in [("letter", 2), ("letter", 3), ("letter", 4), ("cased", 4), ("bert_ws", 2), ("bert_ws", 3), ("py_space", 2),
                ("py_space", 3), ("bert_punct", 2), ("bert_punct", 3), ("bert_punct", 4)]:
        assert key in pairs, key
    assert ("bert_ws", 4) not in pairs and ("py_space", 4) not in pairs  # the fixtures hold none
    placed = {p.cp for p in K.position_family()}
    for (kind, n), cp in pairs.items():
        assert cp in placed and K.utf8_len(cp) == n and K.kind_member(kind, cp), (kind, n, hex(cp))
    assert int(K.lower_table()[pairs[("cased", 4)]]) >= 0x10000


def test_every_seam_offset_and_surrounding_is_reached():
    """from the generated bytes: the character's lead byte lies at seam + offset, a letter stands on either side of it, and the
    surroundings are what they claim"""
    seams = K.seams()
    max_cap = max(K.EXPECTED_CONSTANTS[k] for k in ("SWT_LANE_CAP", "kDCap", "kWCap", "kWpCap"))
    reached = set()
    tab = K.class_table()
    for p in K.position_family():
        buf, off = K.pack(p.texts)
        raw = buf.tobytes()
        ch = K.utf8(chr(p.cp))
        for lead in p.leads:
            assert raw[lead:lead + len(ch)] == ch, p.name
            before, after = raw[lead - 1:lead], raw[lead + len(ch):lead + len(ch) + 1]
            assert (before.isalpha() or before >= b"\x80" or lead == 0) and (after.isalpha() or after >= b"\x80"), p.name
            for name, at in seams.items():
                if lead == at + p.offset:
                    reached.add((name, p.offset, p.layout, p.cp))
        starts = set(off.tolist())
        if p.layout == "long":
            assert int(off[1]) > max_cap + 64  # every kernel cuts its first chunk inside the first sentence
        elif p.layout == "sentences":
            assert int(np.diff(off.astype(np.int64)).max()) < 128
            for tile in ("SWT_LANE_TILE", "kWTile", "kDTile"):
                t = seams[tile]
                assert any(t - 128 < s < t for s in starts) and any(t <= s < t + 128 for s in starts), p.name
        else:
            words = K.split_words(K.lower(p.texts[0]))
            assert len(words) == {"bert_ws": 2, "bert_punct": 3}.get(p.kind, 1), p.name
            assert K.nbytes(words[-1]) >= K.GIANT_TAIL > max_cap  # the one-lane walk over global memory runs behind it
            if p.leads[0] >= max_cap + 1:
                assert K.nbytes(words[0]) > max_cap
    cps = set(K.representatives().values())
    missing = [(name, d, layout, hex(cp)) for name in seams for d in K.OFFSETS for layout in ("sentences", "long", "giant") for cp in cps
               if (name, d, layout, cp) not in reached]
    assert not missing, missing[:10]
    print("P: %d batches, %d (seam, offset, layout, character) placements" % (len(K.position_family()), len(reached)))


def test_level2_batch_crosses_the_second_scan_level():
    texts, leads = K.level2_batch()
    buf, off = K.pack(texts)
    assert buf.size > K.LEVEL2 + 4096 and len(texts) > 64
    assert leads[0] == K.LEVEL2 - 4 and any(l < K.LEVEL2 < l + 4 for l in leads)  # a character straddles the seam
    assert any(int(o) > K.LEVEL2 for o in off[:-1])                                # sentences start behind it
    # the separator form is longer by one byte per sentence: its seam lies elsewhere in the text, and S1 crosses it seven times
    assert sum(map(K.nbytes, K.s1())) > 7 * K.LEVEL2


def test_sweeps_are_what_they_say():
    s1, s16 = K.s1(), K.s16()
    assert len(s1) == 0x10FFFF and s1[0] == "ab\x01ab" and s1[-1] == "ab\U0010ffffab" and ord(s1[K.edge_set()[5] - 1][2]) == K.edge_set()[5]
    assert len(s16) == 69632 and len(s16[0]) == 31 and len(s16[1]) == 33 and s16[-1][-2] == "\U0010ffff"
    assert not any("\x00" in t for t in s16[:2]) and all("\x00" in t or t == "" for t in K.nul_batch())
    assert K.lower("Aİ\U00010400") == "aİ\U00010428"  # a host code point stays


def test_what_the_four_byte_lowercase_pairs_can_show():
    """every cased code point above U+FFFF lies below U+40000, so bits 12..17 of its lowercase are below 0x40: the mask on the
    second byte of lower_kernel's 4-byte branch changes nothing for them, and a mutant that drops it is output-equivalent
    ("Code-point sweeps").  The low four of those bits do differ from zero, which is what a test can see."""
    four = [(s, d) for s, d in K.fixture("unicode_lower.json")["pairs"] if s >= 0x10000]
    assert len(four) == 225 and all(d >= 0x10000 for _s, d in four)
    assert max(d for _s, d in four) < 0x40000
    assert any((d >> 12) & 0x0F for _s, d in four) and any(((s >> 6) & 0x3F) != ((d >> 6) & 0x3F) for s, d in four)
