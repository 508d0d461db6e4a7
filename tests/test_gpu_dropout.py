"""BPE-dropout on the device (swt_bpe_encode_dropout*, the Dropout form of bpe_lane_kernel: the literal rounds under a DropRule)
against the plain-Python model of tests/dropout_cases.py: ids and sentence offsets equal element by element, at the smallest
shapes that reach each seam of the kernel -- the single workgroup and the tiles, tile boundaries moved by SWT_OPT_LANE_SPAN and
SWT_OPT_LANE_TAPER, a word across a chunk's end, words beyond the 32-slot mask, a word longer than a chunk (one lane, global
memory), multi-byte code points, empty sentences, one word 500 times -- and through the Python surface.  Every case fails
without the feature: the entry points are not there.

Needs a real MI355X: `-m gpu`."""
import ctypes as C
import json
import os
import random

import numpy as np
import pytest

from tests import dropout_cases as D

pytestmark = pytest.mark.gpu

SEED, EPOCH = (1 << 63) + 977, 3
CHUNK = 512  # staged bytes per chunk of the dropout kernel: kLaneCap


@pytest.fixture(scope="module")
def dev(native):
    if native.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests need an MI355X (there is no CPU fallback to test)")
    native.init(0)
    return native


@pytest.fixture(scope="module")
def split(swt):
    return swt.SubwordTokenizer._split


def table_info(dev, tok, which):
    fn = dev.lib().swt_debug_bpe_table_info
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int]
    return fn(tok._table._h, which)


class Case:
    """a FastBPE over `merges` and the model's table of the same merges"""

    def __init__(self, swt, dev, merges, shift=0):
        from subword_tokenizers_amd import tokenizers as T

        self.tok, self.table, self.dev = swt.FastBPE(), D.Table(merges), dev
        self.tok.merges_list = [tuple(m) for m in merges]
        if shift:  # merged symbols numbered from SYM_BASE + shift: beyond what a packed value holds
            syms = T._SymbolTable()
            for k in range(shift):
                syms.intern("\x00pad %d" % k)
            ids = np.array([x for l, r in self.tok.merges_list for x in (syms.intern(l), syms.intern(r), syms.intern(l + r))],
                           dtype=np.uint32).reshape(-1, 3)
            self.tok._bpe_ranks = {pair: i for i, pair in enumerate(self.tok.merges_list)}
            self.tok._set_table(syms, ids[:, 0], ids[:, 1], ids[:, 2])
        else:
            self.tok._build_table()

    def intern(self, s):
        return self.dev.SYM_BASE + self.tok._syms.index[s]

    def want(self, split, texts, below, seed=SEED, epoch=EPOCH, first=0):
        return D.ids_of(D.tokenize(self.table, split, texts, below, seed, epoch, first), self.intern)

    def got(self, texts, below, seed=SEED, epoch=EPOCH):
        text, off = self.dev.pack_and_lower(texts)
        return self.tok._table.encode_dropout(text, off, (below, seed, epoch))


@pytest.fixture(scope="module")
def cases(swt, dev, ref_dir):
    with open(os.path.join(ref_dir, "resources/pretrained/FastBPE", "merges.json"), encoding="utf-8") as f:
        pretrained = json.load(f)
    out = {"proper": Case(swt, dev, D.PROPER), "improper": Case(swt, dev, D.IMPROPER), "unpacked": Case(swt, dev, D.PROPER, 0x10000),
           "pretrained": Case(swt, dev, pretrained)}
    # a packed and an unpacked table, a proper and an improper one
    assert [table_info(dev, out[k].tok, 1) for k in ("proper", "improper", "unpacked", "pretrained")] == [1, 1, 0, 1]
    assert [table_info(dev, out[k].tok, 2) for k in ("proper", "improper", "unpacked", "pretrained")] == [1, 0, 1, 1]
    return out


def same(got, want, tag):
    assert np.array_equal(np.asarray(got[1], dtype=np.uint64), want[1]), "sentence offsets differ: " + tag
    assert np.array_equal(got[0], want[0]), "ids differ: " + tag


# ---- the single workgroup: at most 64 sentences and 1,024 bytes
DIRECT = D.short_sentences(12, 800, seed=11)


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("name", ["proper", "improper", "unpacked"])
def test_direct_route(cases, split, name, p):
    c = cases[name]
    assert len(DIRECT) <= 64 and sum(len(t.encode()) for t in DIRECT) <= 1024
    same(c.got(DIRECT, D.drop_below(p)), c.want(split, DIRECT, D.drop_below(p)), "%s table, p = %g" % (name, p))


def test_direct_route_pretrained(cases, split, corpora):
    c, texts = cases["pretrained"], corpora["pan"][100:112]
    assert sum(len(t.lower().encode()) for t in texts) <= 1024
    same(c.got(texts, D.drop_below(0.2)), c.want(split, texts, D.drop_below(0.2)), "pretrained merges")


# ---- the tiles: about 200 short sentences, 20 KB; the model is computed once
TILED = D.short_sentences(200, 20000, seed=12)
TILED_P = 0.25


@pytest.fixture(scope="module")
def tiled_want(cases, split):
    return {name: cases[name].want(split, TILED, D.drop_below(TILED_P)) for name in ("proper", "improper", "unpacked")}


@pytest.mark.parametrize("name", ["proper", "improper", "unpacked"])
def test_tile_route(cases, tiled_want, name):
    assert 15000 < sum(len(t.encode()) for t in TILED) < 25000
    same(cases[name].got(TILED, D.drop_below(TILED_P)), tiled_want[name], "%s table" % name)


GEOMETRY = [("span 1", {"OPT_LANE_SPAN": 1}), ("span 2", {"OPT_LANE_SPAN": 2}), ("taper c = 1, 8 slots", {"OPT_LANE_TAPER": 8, "OPT_LANE_SLOTS": 8}),
            ("taper c = 2/8 to 192 bytes, 16 slots", {"OPT_LANE_TAPER": 256 + 2, "OPT_LANE_SLOTS": 16})]


def test_tile_boundaries_do_not_matter(dev, cases, tiled_want):
    c = cases["proper"]
    h, maps = c.tok._table, set()
    for tag, options in GEOMETRY:
        try:
            for k, v in options.items():
                h.set_option(getattr(dev, k), v)
            same(c.got(TILED, D.drop_below(TILED_P)), tiled_want["proper"], tag)
            out = np.zeros(16, dtype=np.uint64)
            fn = dev.lib().swt_debug_bpe_tile_map
            fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p]
            dev.check(fn(h._h, sum(len(t.encode()) for t in TILED), out.ctypes.data))
            maps.add(tuple(out.tolist()))
        finally:
            for k in options:
                h.set_option(getattr(dev, k), 0)
    assert len(maps) >= 3, "the geometries of this test give the same tiles"


def test_dedup_is_never_taken(dev, cases, tiled_want):
    c = cases["proper"]
    h, got = c.tok._table, {}
    for mode in (dev.DEDUP_NEVER, dev.DEDUP_ALWAYS):
        h.set_option(dev.OPT_DEDUP, mode)
        dev.profile_enable(3)  # level 3 brackets the first launch of the dedup pipeline and nothing else
        try:
            dev.profile_read()
            got[mode] = c.got(TILED, D.drop_below(TILED_P))
            _, n = dev.profile_read()
        finally:
            dev.profile_enable(0)
            h.set_option(dev.OPT_DEDUP, dev.DEDUP_AUTO)
        assert n == 0, "%d dedup pipelines ran under SWT_OPT_DEDUP %d" % (n, mode)
        same(got[mode], tiled_want["proper"], "SWT_OPT_DEDUP %d" % mode)
    # (the plain encode of the same handle does take it when told to: the knob is live)
    h.set_option(dev.OPT_DEDUP, dev.DEDUP_ALWAYS)
    dev.profile_enable(3)
    try:
        dev.profile_read()
        c.tok._table.encode(*dev.pack_and_lower(TILED))
        _, n = dev.profile_read()
    finally:
        dev.profile_enable(0)
        h.set_option(dev.OPT_DEDUP, dev.DEDUP_AUTO)
    assert n == 1


# ---- words at the seams
def straddlers():
    """sentences longer than a chunk, so that the chunk is cut at a word boundary and the word across its end is staged again;
    the prefix moves which word that is, byte by byte"""
    rng = random.Random(13)
    return ["q" * k + " " + D.fill(1300, rng) for k in (0, 1, 2, 3, 5, 8, 13, 15)]


LONG33, LONG100 = "ab" * 16 + "a", "abcd" * 25
GIANT_ASCII, GIANT_WIDE = "abcd" * 150, "żół" * 120 + "\U0001F600\U0001F600"  # 600 and 728 bytes: longer than a chunk
SEAMS = {
    "a word across a chunk's end": straddlers(),
    "words of 33 and 100 symbols": ["xy " + LONG33 + " ab", LONG100, "", LONG33 + " " + LONG100 + " " + LONG33 + "," + LONG100 + " cd"] + D.short_sentences(30, 2000, 14),
    "a word longer than a chunk, among others": D.short_sentences(20, 1500, 15) + ["ab " + GIANT_ASCII + " cd xy", "", GIANT_WIDE, GIANT_ASCII + GIANT_ASCII]
    + D.short_sentences(10, 600, 16),
    "a word longer than a chunk, single workgroup": ["cd ab", "xy " + GIANT_ASCII + " abcd"],
    "a wide word longer than a chunk, single workgroup": ["", GIANT_WIDE + " żół", "ab"],
    "multi-byte and 4-byte code points": ["żółżół \U0001F600\U0001F600\U0001F600\U0001F600 €a€a zażółć — ¿co? łłł óż", "\U0001F600\U0001F600€a", "ż"] * 30,
    "empty sentences": ["", "", "abcd abab", "", "xyxy", "", ""] * 40 + [""],
    "a sentence that starts mid-tile": ["ab" * 50 + " " + "xy" * 45, "abcdabcd " * 30, "qqqq " * 37, "cd"] * 8,
}


@pytest.mark.parametrize("name", ["proper", "improper", "unpacked"])
@pytest.mark.parametrize("seam", list(SEAMS))
def test_seams(cases, split, seam, name):
    c, texts = cases[name], SEAMS[seam]
    n_bytes = sum(len(t.encode()) for t in texts)
    if "single workgroup" in seam:
        assert len(texts) <= 64 and n_bytes <= 1024 and max(len(w.encode()) for t in texts for w in t.split()) > CHUNK
    elif "longer than a chunk" in seam:
        assert n_bytes > 1024 and max(len(w.encode()) for t in texts for w in t.split()) > CHUNK
    elif "across" in seam:
        assert min(len(t.encode()) for t in texts) > 2 * CHUNK
    below = D.drop_below(0.3)
    same(c.got(texts, below), c.want(split, texts, below), "%s, %s table, %d bytes" % (seam, name, n_bytes))


def test_the_same_word_500_times(cases, split):
    c, text = cases["proper"], " ".join(["abcdabcdabcd"] * 500)
    got = c.got([text], D.drop_below(0.5))
    same(got, c.want(split, [text], D.drop_below(0.5)), "p = 0.5")
    per_word = lambda ids: {tuple(w.tolist()) for w in np.split(ids, np.flatnonzero((ids & D.CONT) == 0)[1:])}  # noqa: E731
    assert len(per_word(got[0])) > 20, "the occurrences of one word come out alike at p = 0.5"
    none = c.got([text], 0)
    assert len(none[0]) == 500 and len(per_word(none[0])) == 1
    same(none, c.want(split, [text], 0), "p = 0")


# ---- end points and tables
@pytest.mark.parametrize("name", ["proper", "improper", "unpacked", "pretrained"])
def test_end_points(dev, cases, split, corpora, name):
    c = cases[name]
    for texts in (DIRECT, TILED if name != "pretrained" else corpora["pan"][:150]):
        text, off = dev.pack_and_lower(texts)
        same(c.got(texts, 0), c.tok._table.encode(text, off, flags=dev.BPE_NO_DEDUP), "drop_below 0 against swt_bpe_encode, %s table" % name)
        same(c.got(texts, D.ONE), D.ids_of(D.characters(split, texts), c.intern), "drop_below 2^32, %s table" % name)


def test_a_threshold_above_one_is_refused(dev, cases):
    with pytest.raises(dev.SwtError) as err:
        cases["proper"].got(DIRECT, D.ONE + 1)
    assert err.value.code == dev.ERR_INVALID


# ---- a text's ids depend on (seed, epoch, its index) and its own bytes
def test_batch_independence(cases):
    c, below, rng = cases["proper"], D.drop_below(0.4), random.Random(17)
    base = c.got(TILED, below)
    for i in (0, 1, 57, 120, 199):
        others = [D.fill(rng.randrange(1, 400), rng) for _ in TILED]
        others[i] = TILED[i]
        got = c.got(others, below)
        a, b = (int(x) for x in base[1][i:i + 2])
        a2, b2 = (int(x) for x in got[1][i:i + 2])
        assert b - a > 0 and np.array_equal(base[0][a:b], got[0][a2:b2]), "text %d" % i
    got = c.got([TILED[57]] * 8, below)  # the same text at eight places
    rows = [tuple(got[0][int(got[1][k]):int(got[1][k + 1])].tolist()) for k in range(8)]
    assert len(set(rows)) > 1, "the sentence index does not reach the draws"


# ---- the host form against the `_dev` form
@pytest.mark.parametrize("texts", [DIRECT, TILED], ids=["single workgroup", "tiles"])
def test_host_form_against_dev_form(dev, cases, texts):
    import torch

    c, below = cases["proper"], D.drop_below(0.35)
    text, off = dev.pack_and_lower(texts)
    host = c.tok._table.encode_dropout(text, off, (below, SEED, EPOCH))
    n = int(text.size)
    d_text = torch.from_numpy(np.concatenate([text, np.zeros(64, dtype=np.uint8)])).cuda()
    d_off = torch.from_numpy(off.view(np.int64)).cuda()
    d_ids = torch.zeros(n + 64, dtype=torch.int32, device="cuda")
    d_out_off = torch.zeros(len(texts) + 1, dtype=torch.int64, device="cuda")
    d_ntok = torch.zeros(1, dtype=torch.int64, device="cuda")
    c.tok._table.encode_dropout_dev(d_text.data_ptr(), n, d_off.data_ptr(), len(texts), d_ids.data_ptr(), d_out_off.data_ptr(), d_ntok.data_ptr(),
                                    (below, SEED, EPOCH), 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    nt = int(d_ntok.item())
    assert nt == host[0].size
    same((d_ids[:nt].cpu().numpy().view(np.uint32), d_out_off.cpu().numpy().view(np.uint64)), host, "the _dev form")


# ---- the Python surface
DROP = {"probability": 0.15, "seed": 41, "epoch": 2}


@pytest.fixture(scope="module")
def pan_model(cases, split, corpora):
    return D.tokenize(cases["pretrained"].table, split, corpora["pan"][:100], D.drop_below(0.15), 41, 2)


def test_tokenize_batch(cases, corpora, pan_model):
    tok, pan = cases["pretrained"].tok, corpora["pan"][:100]
    assert tok.tokenize_batch(pan, dropout=DROP) == pan_model
    assert tok.tokenize_batch(pan, dropout=DROP) != tok.tokenize_batch(pan)
    assert tok.tokenize(pan[0], dropout=DROP) == pan_model[0]
    assert tok.tokenize_batch(pan, dropout={"probability": 0.0}) == corpora["pan_tokens"]["FastBPE"][:100]
    assert tok.tokenize_batch(pan, dropout=dict(DROP, epoch=3)) != pan_model


def test_encode_batch_round_trip_and_offsets(cases, corpora, pan_model):
    tok, pan = cases["pretrained"].tok, corpora["pan"][:100]
    plain = tok.decode_batch(tok.encode_batch(pan)["input_ids"])
    batch = tok.encode_batch(pan, dropout=DROP, return_offsets=True)
    assert tok.decode_batch(batch["input_ids"], batch["attention_mask"]) == plain
    voc, unk = tok.vocab_list(), tok.special_ids()["unk"]
    for r, text in enumerate(pan):
        low, row = text.lower(), []
        for col in range(int(batch["length"][r])):
            word = int(batch["word_ids"][r, col])
            if word < 0:
                continue
            s, e = (int(x) for x in batch["offset_mapping"][r, col])
            cont = "##" if word == int(batch["word_ids"][r, col - 1]) else ""
            dense = int(batch["input_ids"][r, col])
            assert dense == unk or voc[dense] == cont + low[s:e]  # (a character the merges never saw has no dense id)
            row.append(cont + low[s:e])
        assert row == pan_model[r]


def test_encode_batch_composes(cases, split, corpora):
    import torch

    c, pan = cases["pretrained"], corpora["pan"]
    tok, a, b = c.tok, pan[:40], pan[40:80]
    dense = lambda tokens: [tok.token_to_id(t) for t in tokens]  # noqa: E731  ([UNK] for a character the merges never saw)
    # pairs: the sentence index of pair j is len(texts) + j, the order of the one encode call that serves both sides
    model = D.tokenize(c.table, split, a + b, D.drop_below(0.15), 41, 2)
    batch = tok.encode_batch(a, text_pairs=b, dropout=DROP)
    for r in range(40):
        seq, ids = batch["sequence_ids"][r], batch["input_ids"][r]
        assert ids[seq == 0].tolist() == dense(model[r]) and ids[seq == 1].tolist() == dense(model[40 + r])
    # the device path gives the host path's rows
    for kw in ({}, {"text_pairs": b}, {"return_offsets": True}, {"packing": "whole", "max_length": 64}):
        host, on_dev = tok.encode_batch(a, dropout=DROP, **kw), tok.encode_batch(a, dropout=DROP, device=True, **kw)
        for k in ("input_ids", "attention_mask") + (("offset_mapping", "word_ids") if "return_offsets" in kw else ()):
            assert np.array_equal(host[k], on_dev[k].cpu().numpy()), (kw, k)
    # packing and masking work on the dropout ids
    packed = tok.encode_batch(a, dropout=DROP, packing="split", max_length=48, add_special_tokens=False)
    flat = packed["input_ids"][packed["attention_mask"] != 0]
    assert flat.tolist() == [i for row in model[:40] for i in dense(row)]
    masked = tok.encode_batch(a, dropout=DROP, mlm={"probability": 0.2, "seed": 9}, return_offsets=True)
    plain = tok.encode_batch(a, dropout=DROP, return_offsets=True)
    sel = masked["labels"] != -100
    assert sel.any() and np.array_equal(masked["labels"][sel], plain["input_ids"][sel])
    assert np.array_equal(masked["input_ids"][~sel], plain["input_ids"][~sel])
    assert np.array_equal(masked["offset_mapping"], plain["offset_mapping"])
    assert torch.cuda.is_available()


@pytest.mark.parametrize("cls", ["NaiveBPE", "NaiveWP", "FastWP"])
def test_the_other_classes_raise(swt, dev, cls):
    tok = getattr(swt, cls)()
    if cls.endswith("BPE"):
        tok.merges_list = [("a", "b")]
    else:
        tok.vocab = {"a", "b", "##b"}
        if cls == "FastWP":
            tok._build_trie()
    for call in (lambda: tok.encode_ids_batch(["ab"], dropout=DROP), lambda: tok.tokenize_batch(["ab"], dropout=DROP),
                 lambda: tok.encode_batch(["ab"], dropout=DROP)):
        with pytest.raises(ValueError, match="FastBPE"):
            call()
