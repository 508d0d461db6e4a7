"""MaxMatch-Dropout on the device (swt_wp_encode_naive_dropout*, the dropout form of wp_naive_kernel: naive_word with a WpDraw)
against the plain-Python model of tests/maxmatch_cases.py: ids, sentence offsets and statuses equal element by element, at the
smallest shapes that reach each seam of the 512-byte tile, 1,024-byte chunk skeleton -- the single workgroup and the tiles, a
sentence start on a tile seam, runs of empty sentences (where the sentence index of a word can go wrong), a sentence longer than
a chunk and one longer than the single workgroup's 2,048 bytes (one lane, global memory: its key must be the tiled one's), code
points of two to four bytes, a candidate of 70 code points (the cached group of draws refilled many times), one word 500 times
-- and through the Python surface.  Every case fails without the feature: the entry points are not there.

Needs a real MI355X: `-m gpu`."""
import random

import numpy as np
import pytest

from tests import maxmatch_cases as M
from tests.test_gpu_wp_seams import CAP, DIRECT_BYTES, DIRECT_SENTS, PIECE, TILE, handmade_vocab
from tests.test_naive_wp_encode import naivewp_cases

pytestmark = pytest.mark.gpu

SEED, EPOCH = (1 << 63) + 977, 3
LONG = "x" * 70
# the handmade vocabulary with code points of three and four bytes, pieces that mix the widths, and one piece of 70 code points
WIDE = handmade_vocab() + ["€", "##€", "\U0001F600", "##\U0001F600", "中", "##中", "€a", "##€ż", "a€", "\U0001F600\U0001F600", "##\U0001F600a",
                           "ż中€", "##中ż", LONG, "##" + LONG]
WIDE_WORDS = M.WORDS + ["€", "€a", "a€ż", "\U0001F600\U0001F600\U0001F600a", "ż中€中ż", "中中", "x€ż\U0001F600", "żół€", LONG, LONG + "xxxxx", "q" * 85]


@pytest.fixture(scope="module")
def dev(native):
    if native.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests need an MI355X (there is no CPU fallback to test)")
    native.init(0)
    return native


@pytest.fixture(scope="module")
def split(swt):
    return swt.SubwordTokenizer._split


class Case:
    """a NaiveWP over `vocab` and the model of the same vocabulary"""

    def __init__(self, swt, dev, vocab):
        self.tok, self.model, self.dev = swt.NaiveWP(), M.Model(vocab), dev
        self.tok.vocab = set(vocab)

    def want(self, split, texts, below, seed=SEED, epoch=EPOCH, first=0):
        return self.model.batch(split, texts, below, seed, epoch, first)

    def got(self, texts, below, seed=SEED, epoch=EPOCH):
        text, off = self.dev.pack_and_lower(texts)
        return self.tok._ensure_naive_trie().encode_naive_dropout(text, off, (below, seed, epoch))


@pytest.fixture(scope="module")
def pan_case():
    (vocab, texts), = [(v, t) for name, v, t, _ in naivewp_cases() if name == "pan_tadeusz_pretrained"]
    return vocab, texts


@pytest.fixture(scope="module")
def cases(swt, dev, pan_case):
    (unk_vocab,) = [v for name, v, _, _ in naivewp_cases() if name == "unk_after_first_piece"]
    return {"handmade": Case(swt, dev, handmade_vocab()), "wide": Case(swt, dev, WIDE), "pretrained": Case(swt, dev, pan_case[0]),
            "loop": Case(swt, dev, M.MICRO_LOOP), "unk": Case(swt, dev, M.MICRO_UNK), "unk_late": Case(swt, dev, unk_vocab)}


def same(got, want, tag):
    assert np.array_equal(got[2], want[2]), "statuses differ: " + tag
    assert np.array_equal(np.asarray(got[1], dtype=np.uint64), want[1]), "sentence offsets differ: " + tag
    assert np.array_equal(got[0], want[0]), "ids differ: " + tag


def nbytes(texts):
    return sum(len(t.lower().encode()) for t in texts)


# ---- the single workgroup: at most 64 sentences and 2,048 bytes
DIRECT = M.short_sentences(14, 1700, seed=11, words=WIDE_WORDS, empty=6)


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("name", ["handmade", "wide"])
def test_direct_route(cases, split, name, p):
    c = cases[name]
    assert len(DIRECT) <= DIRECT_SENTS and 1024 < nbytes(DIRECT) <= DIRECT_BYTES
    want = c.want(split, DIRECT, M.drop_below(p))
    if name == "handmade":
        assert want[2].any() and not want[2].all()  # a euro sign under the handmade vocabulary never returns
    same(c.got(DIRECT, M.drop_below(p)), want, "%s vocabulary, p = %g" % (name, p))


def test_direct_route_pretrained(cases, split, pan_case):
    c, texts = cases["pretrained"], pan_case[1][100:112]
    assert nbytes(texts) <= DIRECT_BYTES
    same(c.got(texts, M.drop_below(0.2)), c.want(split, texts, M.drop_below(0.2)), "pretrained vocabulary")


# ---- the tiles: about 200 short sentences, 20 KB; the model is computed once per vocabulary and p
TILED = M.short_sentences(200, 20000, seed=12, words=WIDE_WORDS)


def tiled_texts(name, pan):
    if name != "pretrained":
        return TILED
    return [("" if k % 31 == 7 else t) for k, t in enumerate(pan[200:650])]  # (a line of the poem has some 44 bytes)


@pytest.fixture(scope="module")
def tiled_want(cases, split, pan_case):
    return {(name, p): cases[name].want(split, tiled_texts(name, pan_case[1]), M.drop_below(p))
            for name in ("handmade", "wide", "pretrained") for p in (0.1, 0.5)}


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("name", ["handmade", "wide", "pretrained"])
def test_tile_route(cases, tiled_want, pan_case, name, p):
    texts = tiled_texts(name, pan_case[1])
    assert 15000 < nbytes(texts) < 30000 and len(texts) > 150
    same(cases[name].got(texts, M.drop_below(p)), tiled_want[(name, p)], "%s vocabulary, p = %g" % (name, p))


# ---- the seams
def exact(n, seed, tail=""):
    """a sentence of n bytes exactly, ending with `tail`"""
    rng = random.Random(seed)
    t = M.fill(n - len(tail.encode()), rng, WIDE_WORDS) + tail
    assert len(t.encode()) == n
    return t


GIANT = exact(CAP + 300, 21, "żółżół abżół ż中€中ż xyab")           # longer than a chunk
HUGE = exact(DIRECT_BYTES + 500, 22, "żółab \U0001F600\U0001F600\U0001F600a " + LONG + "xxxxx żół€")  # and than the single workgroup
SEAMS = {
    "a sentence start on a tile seam": [exact(TILE, 23), exact(TILE, 24), exact(3, 25), exact(TILE - 3, 26), exact(2 * TILE, 27), "abcd żół"]
    + M.short_sentences(20, 1500, 28, WIDE_WORDS),
    "empty sentences, single workgroup": ["", "", "", "abcd abab", "", "xyxy żółżół", "", "", "aaaaab", ""] * 6 + ["", "", "", ""],
    "empty sentences, tiles": ["", "", "abcd abab żółżół", "", "xyxy abcdabcdabcd", "", ""] * 60 + [""] * 70 + ["abab"] + [""] * 3,
    "empty sentences around a tile seam": [exact(TILE - 2, 29), "", "", "", "ab", "", "", exact(TILE, 30), "", "abcd"] * 4 + ["", ""],
    "a sentence longer than a chunk, among others": M.short_sentences(20, 1500, 31, WIDE_WORDS) + ["", "", GIANT, "", "abcd"]
    + M.short_sentences(10, 600, 32, WIDE_WORDS) + [HUGE, "", ""],
    "a sentence longer than a chunk, single workgroup": ["cd ab", "", "", GIANT, "", "żół abcd", ""],
    "a sentence longer than the single workgroup, alone": [HUGE],
    "multi-byte code points and punctuation": ["żółżół \U0001F600\U0001F600\U0001F600a €a a€ż żażółó — ¿ab? łłł óż x,y ab-cd a.b d. ,- .", "ż中€中ż中中€", "ż", ",",
                                               "x€ż\U0001F600 żół€"] * 30,
    "candidates of 70 code points": [LONG + " " + LONG + "xxxxx x" + LONG, "q" * 85 + " " + PIECE + " " + "q" * 41, "xy" + LONG] * 12,
}


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("seam", list(SEAMS))
def test_seams(cases, split, seam, p):
    c, texts = cases["wide"], SEAMS[seam]
    n = nbytes(texts)
    if seam.endswith("single workgroup"):
        assert len(texts) <= DIRECT_SENTS and n <= DIRECT_BYTES
    else:
        assert len(texts) > DIRECT_SENTS or n > DIRECT_BYTES
    if "longer than a chunk" in seam:
        assert max(len(t.encode()) for t in texts) > CAP
    below = M.drop_below(p)
    want = c.want(split, texts, below)
    assert not want[2].any()
    same(c.got(texts, below), want, "%s, %d bytes, p = %g" % (seam, n, p))


def test_the_draws_reach_beyond_the_first_groups(cases, split):
    """at p = 0.5 the 70-code-point piece is dropped somewhere and kept somewhere: c >> 2 = 17 is drawn for"""
    c, texts = cases["wide"], SEAMS["candidates of 70 code points"]
    long_id = c.model.ids[LONG]
    full = int((c.got(texts, 0)[0] == long_id).sum())
    assert full == int((c.want(split, texts, 0)[0] == long_id).sum()) >= 24
    assert 0 < int((c.got(texts, M.drop_below(0.5))[0] == long_id).sum()) < full


def words_of_ids(c, ids):
    """the id rows of the words: a word's first token is the one that does not begin with '##'"""
    names = sorted(c.model.vocab)
    first = np.array([not (int(i) < len(names) and names[int(i)].startswith("##")) for i in ids])
    return {tuple(w.tolist()) for w in np.split(ids, np.flatnonzero(first)[1:])}


def test_the_same_word_500_times(cases, split):
    c, word = cases["wide"], "abcdabcdabcd"
    for texts in ([" ".join([word] * 500)], [word] * 500):
        got = c.got(texts, M.drop_below(0.5))
        same(got, c.want(split, texts, M.drop_below(0.5)), "p = 0.5, %d sentences" % len(texts))
        assert len(words_of_ids(c, got[0])) > 20, "the occurrences of one word come out alike at p = 0.5"
        none = c.got(texts, 0)
        assert len(words_of_ids(c, none[0])) == 1
        same(none, c.want(split, texts, 0), "p = 0, %d sentences" % len(texts))


# ---- end points
@pytest.mark.parametrize("name", ["handmade", "wide", "pretrained"])
def test_end_points(dev, cases, split, pan_case, name):
    c = cases[name]
    for texts in (DIRECT if name != "pretrained" else pan_case[1][100:112], tiled_texts(name, pan_case[1])):
        text, off = dev.pack_and_lower(texts)
        plain = c.tok._ensure_naive_trie().encode_naive(text, off)
        same(c.got(texts, 0), plain, "drop_below 0 against swt_wp_encode_naive, %s vocabulary" % name)
        same(plain, c.want(split, texts, 0), "the model at 0, %s vocabulary" % name)
        same(c.got(texts, M.ONE), c.want(split, texts, M.ONE), "drop_below 2^32, %s vocabulary" % name)
        if name == "pretrained":
            chars = [c.model.ids_of(row) for row in M.characters(split, texts)]
            assert c.got(texts, M.ONE)[0].tolist() == [i for row in chars for i in row]


def test_a_threshold_above_one_is_refused(dev, cases):
    with pytest.raises(dev.SwtError) as err:
        cases["wide"].got(DIRECT, M.ONE + 1)
    assert err.value.code == dev.ERR_INVALID


def test_a_triple_sharp_vocabulary_is_refused(swt, dev):
    c = Case(swt, dev, ["a", "###b", "##"])
    with pytest.raises(dev.SwtError) as err:
        c.got(["ab"], M.drop_below(0.5))
    assert err.value.code == dev.ERR_UNSUPPORTED


# ---- where the outcome depends on the draw
@pytest.mark.parametrize("rows", [40, 200], ids=["single workgroup", "tiles"])
def test_the_status_depends_on_the_draw(cases, split, rows):
    texts, below = ["abc"] * rows, M.drop_below(0.5)
    loop, unk = cases["loop"].got(texts, below, 0, 0), cases["unk"].got(texts, below, 0, 0)
    same(loop, cases["loop"].want(split, texts, below, 0, 0), "{a, ##, ##bc}")
    same(unk, cases["unk"].want(split, texts, below, 0, 0), "{a, ##bc}")
    assert 0 < int(loop[2].sum()) < rows and not unk[2].any()
    assert np.array_equal(np.diff(unk[1].astype(np.int64)) == 1, loop[2] != 0)  # one "[UNK]" where the other never returns


def test_unk_discards_stored_pieces(cases, split):
    c, texts, below = cases["unk_late"], ["unaffable x unaffab xy"] * 60, M.drop_below(0.5)
    got = c.got(texts, below, 11, 0)
    same(got, c.want(split, texts, below, 11, 0), "un ##aff ##able")
    late = [i for i in range(60) if not M.dropped(2, 0, i, 0, 11, below) and not M.dropped(3, 2, i, 0, 11, below)
            and M.dropped(4, 5, i, 0, 11, below)]
    assert late and all(int(got[0][int(got[1][i])]) == c.model.unk for i in late)


# ---- a text's ids depend on (seed, epoch, its index) and its own bytes
def test_batch_independence(cases):
    c, below, rng = cases["wide"], M.drop_below(0.4), random.Random(17)
    base = c.got(TILED, below)
    for i in (0, 1, 57, 120, 199):
        others = [M.fill(rng.randrange(1, 400), rng, M.WORDS) for _ in TILED]
        others[i] = TILED[i]
        got = c.got(others, below)
        a, b = (int(x) for x in base[1][i:i + 2])
        a2, b2 = (int(x) for x in got[1][i:i + 2])
        assert b - a > 0 and np.array_equal(base[0][a:b], got[0][a2:b2]), "text %d" % i
    got = c.got([TILED[57]] * 8, below)  # the same text at eight places
    rows = [tuple(got[0][int(got[1][k]):int(got[1][k + 1])].tolist()) for k in range(8)]
    assert len(set(rows)) > 1, "the sentence index does not reach the draws"
    assert c.got(TILED, below, SEED + 1)[0].tolist() != base[0].tolist() and c.got(TILED, below, SEED, EPOCH + 1)[0].tolist() != base[0].tolist()


# ---- the host form against the `_dev` form
@pytest.mark.parametrize("texts", [DIRECT, TILED], ids=["single workgroup", "tiles"])
def test_host_form_against_dev_form(dev, cases, texts):
    import torch

    c, below = cases["handmade"], M.drop_below(0.35)
    text, off = dev.pack_and_lower(texts)
    host = c.got(texts, below)
    assert host[2].any()
    n = int(text.size)
    d_text = torch.from_numpy(np.concatenate([text, np.zeros(64, dtype=np.uint8)])).cuda()
    d_off = torch.from_numpy(off.view(np.int64)).cuda()
    d_ids = torch.zeros(n + 64, dtype=torch.int32, device="cuda")
    d_out_off = torch.zeros(len(texts) + 1, dtype=torch.int64, device="cuda")
    d_status = torch.zeros(len(texts) + 8, dtype=torch.uint8, device="cuda")
    d_ntok = torch.zeros(1, dtype=torch.int64, device="cuda")
    c.tok._ensure_naive_trie().encode_naive_dropout_dev(d_text.data_ptr(), n, d_off.data_ptr(), len(texts), d_ids.data_ptr(), d_out_off.data_ptr(),
                                                        d_status.data_ptr(), d_ntok.data_ptr(), (below, SEED, EPOCH),
                                                        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    nt = int(d_ntok.item())
    assert nt == host[0].size
    same((d_ids[:nt].cpu().numpy().view(np.uint32), d_out_off.cpu().numpy().view(np.uint64), d_status[:len(texts)].cpu().numpy()), host,
         "the _dev form")


# ---- the Python surface
DROP = {"probability": 0.15, "seed": 41, "epoch": 2}


@pytest.fixture(scope="module")
def pan_model(cases, split, pan_case):
    return cases["pretrained"].model.tokenize(split, pan_case[1][:100], M.drop_below(0.15), 41, 2)


def test_tokenize_batch(cases, pan_case, pan_model):
    tok, pan = cases["pretrained"].tok, pan_case[1][:100]
    assert tok.tokenize_batch(pan, maxmatch_dropout=DROP) == pan_model
    assert tok.tokenize_batch(pan, maxmatch_dropout=DROP) != tok.tokenize_batch(pan)
    assert tok.tokenize(pan[0], maxmatch_dropout=DROP) == pan_model[0]
    assert tok.tokenize_batch(pan, maxmatch_dropout={"probability": 0.0}) == tok.tokenize_batch(pan) == [tok.tokenize(t) for t in pan]
    assert tok.tokenize_batch(pan, maxmatch_dropout=dict(DROP, epoch=3)) != pan_model
    ids, off, status = tok.encode_ids_batch(pan, maxmatch_dropout=DROP)
    assert not status.any() and ids.tolist() == [i for row in pan_model for i in cases["pretrained"].model.ids_of(row)]


def test_a_text_that_never_returns_raises(cases):
    tok = cases["loop"].tok
    with pytest.raises(RuntimeError):
        tok.tokenize_batch(["abc"] * 40, maxmatch_dropout={"probability": 0.5})
    assert tok.tokenize_batch(["abc"] * 40, maxmatch_dropout={"probability": 0.0}) == [["a", "##bc"]] * 40


def test_encode_batch_round_trip_and_offsets(cases, pan_case, pan_model):
    tok, pan = cases["pretrained"].tok, pan_case[1][:100]
    assert not any("[UNK]" in row for row in pan_model)
    plain = tok.decode_batch(tok.encode_batch(pan)["input_ids"])
    batch = tok.encode_batch(pan, maxmatch_dropout=DROP, return_offsets=True)
    assert tok.decode_batch(batch["input_ids"], batch["attention_mask"]) == plain
    voc = tok.vocab_list()
    for r, text in enumerate(pan):
        low, row, covered = text.lower(), [], []
        for col in range(int(batch["length"][r])):
            word = int(batch["word_ids"][r, col])
            if word < 0:
                continue
            s, e = (int(x) for x in batch["offset_mapping"][r, col])
            cont = "##" if word == int(batch["word_ids"][r, col - 1]) else ""
            assert voc[int(batch["input_ids"][r, col])] == cont + low[s:e]
            if cont:
                assert s == covered[-1][1]  # the tokens of a word tile it
                covered[-1][1] = e
            else:
                covered.append([s, e])
            row.append(cont + low[s:e])
        assert row == pan_model[r]
        assert [low[s:e] for s, e in covered] == [w for w, _ in tok._split(low)]


def test_encode_batch_composes(cases, split, pan_case):
    import torch

    c, pan = cases["pretrained"], pan_case[1]
    tok, a, b = c.tok, pan[:40], pan[40:80]
    dense = lambda tokens: [tok.token_to_id(t) for t in tokens]  # noqa: E731
    # pairs: the sentence index of pair j is len(texts) + j, the order of the one encode call that serves both sides
    model = c.model.tokenize(split, a + b, M.drop_below(0.15), 41, 2)
    batch = tok.encode_batch(a, text_pairs=b, maxmatch_dropout=DROP)
    for r in range(40):
        seq, ids = batch["sequence_ids"][r], batch["input_ids"][r]
        assert ids[seq == 0].tolist() == dense(model[r]) and ids[seq == 1].tolist() == dense(model[40 + r])
    # the device path gives the host path's rows
    for kw in ({}, {"text_pairs": b}, {"return_offsets": True}, {"packing": "whole", "max_length": 128}):
        host, on_dev = tok.encode_batch(a, maxmatch_dropout=DROP, **kw), tok.encode_batch(a, maxmatch_dropout=DROP, device=True, **kw)
        for k in ("input_ids", "attention_mask") + (("offset_mapping", "word_ids") if "return_offsets" in kw else ()):
            assert np.array_equal(host[k], on_dev[k].cpu().numpy()), (kw, k)
    # packing and masking work on the dropout ids
    whole = tok.encode_batch(a, maxmatch_dropout=DROP, packing="whole", max_length=128, add_special_tokens=False)
    flat = sorted(whole["input_ids"][whole["attention_mask"] != 0].tolist())
    assert flat == sorted(i for row in model[:40] for i in dense(row))  # (whole rows move, none is cut: the same ids, reordered)
    packed = tok.encode_batch(a, maxmatch_dropout=DROP, packing="split", max_length=48, add_special_tokens=False)
    assert packed["input_ids"][packed["attention_mask"] != 0].tolist() == [i for row in model[:40] for i in dense(row)]
    masked = tok.encode_batch(a, maxmatch_dropout=DROP, mlm={"probability": 0.2, "seed": 9}, return_offsets=True)
    plain = tok.encode_batch(a, maxmatch_dropout=DROP, return_offsets=True)
    sel = masked["labels"] != -100
    assert sel.any() and np.array_equal(masked["labels"][sel], plain["input_ids"][sel])
    assert np.array_equal(masked["input_ids"][~sel], plain["input_ids"][~sel])
    assert np.array_equal(masked["offset_mapping"], plain["offset_mapping"])
    assert torch.cuda.is_available()


@pytest.mark.parametrize("cls", ["NaiveBPE", "FastBPE", "FastWP"])
def test_the_other_classes_raise(swt, dev, cls):
    tok = getattr(swt, cls)()
    if cls.endswith("BPE"):
        tok.merges_list = [("a", "b")]
    else:
        tok.vocab = {"a", "b", "##b"}
        tok._build_trie()
    for call in (lambda: tok.encode_ids_batch(["ab"], maxmatch_dropout=DROP), lambda: tok.tokenize_batch(["ab"], maxmatch_dropout=DROP),
                 lambda: tok.encode_batch(["ab"], maxmatch_dropout=DROP)):
        with pytest.raises(ValueError, match="NaiveWP"):
            call()
