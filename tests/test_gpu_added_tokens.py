"""Added and special tokens written in the text, on the device (csrc/swt_added.hip): swt_added_find / swt_added_splice in their
host and `_dev` forms through encode_batch of the four classes, against the plain-Python model of tests/added_cases.py -- matches,
blanking and splice by the model, the tokens in between by the class's own span call over the model-blanked text, the rows by the
models of tests/batch_cases.py, pair_cases.py and pack_cases.py -- and, for the two WordPiece classes, against the `tokenizers`
wheel's recorded output (tests/golden/added_tokens.json)."""
import os

import numpy as np
import pytest

from tests import added_cases as A
from tests import batch_cases as B
from tests import pack_cases as K
from tests import pair_cases as P

pytestmark = pytest.mark.gpu

CLASSES = ["FastBPE", "FastWP", "NaiveBPE", "NaiveWP"]
KEYS = ("input_ids", "attention_mask", "length", "offset_mapping", "word_ids")


@pytest.fixture(scope="module")
def dev(native):
    if native.device_count() < 1:
        pytest.fail("no HIP device")
    native.init(0)
    return native


_tokenizers = {}


def _tokenizer(swt, ref_dir, cls):
    """one tokenizer per class for the module -- the small WordPiece vocabulary the filler words are made of, the pretrained
    merges -- handed out with no added token"""
    if cls not in _tokenizers:
        tok = getattr(swt, cls)()
        tok.load_resources(os.path.join(ref_dir, "resources", "pretrained/FastBPE" if "BPE" in cls else "tests/FastWordPiece"))
        _tokenizers[cls] = tok
    _tokenizers[cls].clear_added_tokens()
    return _tokenizers[cls]


def _to_numpy(res):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in res.items()}


def _blanked(added, texts):
    patterns = A.patterns_of(added)
    low = [t.lower() for t in texts]
    matches = [A.find_matches(t, patterns) for t in low]
    return matches, [A.blank(t, m) for t, m in zip(low, matches)]


def _kept(tok, added, texts):
    """the texts whose blanked form the class's encoder returns from: a text the reference's WordPiece loops never end on has no
    spans, and the span calls raise on it -- behaviour that was there before added tokens"""
    if not hasattr(tok, "_raise_naive_status"):
        return list(texts)
    status = tok.encode_ids_batch(_blanked(added, texts)[1])[2]
    return [t for t, st in zip(texts, status) if not st]


# the texts of the cases that leave, after blanking, a punctuation mark the small WordPiece vocabulary does not hold: only these may
# be dropped by _kept, and none of them lies on a seam of the find kernel
NEVER_RETURNS = {"[mask", "mask]", "MASK]", "exam <use", "r> exam", "a été€été€ b été € été€", "a Été€été€ b été € Été€ t"}


def _model(tok, added, texts, dropout=None):
    """-> (rows of raw ids, (spans, words)): the class's span call over the model-blanked texts, the matches spliced in by the
    model; the tokenizer holds `added`"""
    matches, blanked = _blanked(added, texts)
    got = tok._batch_encode_spans(blanked) if dropout is None else tok._batch_encode_spans(blanked, dropout)
    raw, off, spans, word = got[0], got[1], got[-2], got[-1]
    base = tok._batch_vocabulary().added_base
    rows, sp, wd = [], [], []
    for i in range(len(texts)):
        lo, hi = int(off[i]), int(off[i + 1])
        toks = [(int(raw[t]), (int(spans[t][0]), int(spans[t][1])), int(word[t])) for t in range(lo, hi)]
        out = A.splice(toks, matches[i], base)
        assert len(out) == len(toks) + len(matches[i])
        rows.append([i for i, _, _ in out]); sp.append([list(s) for _, s, _ in out]); wd.append([w for _, _, w in out])
    return rows, (sp, wd)


def _check(tok, added, texts, what, **kw):
    """encode_batch(texts, return_offsets=True) on both paths against the model; -> the host result"""
    assert tok.added_tokens() == list(added)
    rows, pay = _model(tok, added, texts)
    voc, sp = tok._batch_vocabulary(), tok.special_ids()
    s = B.spec(max(max((len(r) for r in rows), default=0), 1) + 2, pad_id=sp["pad"], unk_id=sp["unk"], cls_id=sp["cls"], sep_id=sp["sep"])
    want = B.expected_batch(rows, s, (voc.cmap, voc.n_map, voc.flagged), pay)
    first = None
    for device in (False, True):
        got = _to_numpy(tok.encode_batch(texts, return_offsets=True, device=device, **kw))
        for k in KEYS:
            assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (what, k, device)
        assert got["n_unknown"] == want["n_unknown"]
        first = first or got
    return first, rows


# ---- model parity and the seams

@pytest.mark.parametrize("cls", CLASSES)
def test_seams_against_the_model(swt, dev, ref_dir, cls):
    """a match starting at every byte from step - 64 to step + 1 of a text; at a text's start and end; a text that is one match;
    adjacent matches; a would-be match across two texts; empty texts between matches; more than 64 matches in a text and more
    than 64 candidates in a step; two- and three-byte patterns with tokens behind them; several steps with matches in the last"""
    step, halo = dev.added_capacity()[:2]
    assert halo == 63
    tok = _tokenizer(swt, ref_dir, cls)
    added, texts = A.seam_texts(step)
    assert tok.add_special_tokens([c for c, s in added if s]) == 2 and tok.add_tokens([c for c, s in added if not s]) == 1
    added = tok.added_tokens()
    kept = _kept(tok, added, texts)
    assert set(texts) - set(kept) <= NEVER_RETURNS and ("WP" in cls or kept == texts)  # every text at a seam stays, for every class
    assert sum(len(t.encode()) > step for t in kept) == sum(len(t.encode()) > step for t in texts) >= 8
    got, rows = _check(tok, added, kept, "seams")
    mask = tok.mask_id()
    n_mask = sum(t.lower().count("[mask]") for t in kept)
    assert n_mask > 200 and int((got["input_ids"] == mask).sum()) == n_mask


@pytest.mark.parametrize("cls", CLASSES)
def test_overlaps_prefixes_and_long_patterns(swt, dev, ref_dir, cls):
    for added, texts in A.overlap_cases():
        tok = _tokenizer(swt, ref_dir, cls)
        assert tok.add_tokens([c for c, _ in added]) == len(added)
        _check(tok, added, _kept(tok, added, texts), added[0][0])


@pytest.mark.parametrize("cls", ["FastBPE", "NaiveWP"])
def test_4096_patterns_sharing_a_first_byte(swt, dev, ref_dir, cls):
    tok = _tokenizer(swt, ref_dir, cls)
    added, texts = A.many_patterns()
    assert tok.add_tokens([c for c, _ in added]) == 4096
    got, _ = _check(tok, added, texts, "4096")
    voc = tok._batch_vocabulary()
    assert got["input_ids"][0].tolist().count(int(voc.added_dense[0])) == 1 and int(voc.added_dense[4095]) in got["input_ids"][0].tolist()


@pytest.mark.parametrize("cls", CLASSES)
def test_an_all_empty_batch_and_no_occurrence(swt, dev, ref_dir, cls):
    tok = _tokenizer(swt, ref_dir, cls)
    tok.add_special_tokens(["[MASK]"])
    added = tok.added_tokens()
    _check(tok, added, ["", "", ""], "empty")
    _check(tok, added, ["exam is a test.", "", "examples"], "no occurrence")


@pytest.mark.parametrize("cls", ["FastWP", "NaiveWP"])
def test_wordpiece_equals_the_wheel(swt, dev, ref_dir, golden, cls):
    """ids, offsets and word ids of the wheel's recorded cases, element by element; host and device"""
    recorded = golden("added_tokens.json")
    n_texts = 0
    for case in recorded["cases"]:
        tok = _tokenizer(swt, ref_dir, cls)
        assert sorted(tok.vocab) == recorded["vocab"]
        added = [(c, s) for c, s in case["added"]]
        for c, s in added:
            assert tok.add_tokens([c], special=s) == 1
        voc, unk = tok._batch_vocabulary(), tok.special_ids()["unk"]
        dense = {(c if s else c.lower()): int(d) for (c, s), d in zip(added, voc.added_dense)}
        kept = set(_kept(tok, added, case["texts"]))
        assert set(case["texts"]) - kept <= (NEVER_RETURNS if cls == "FastWP" else set()), case["name"]
        pick = [i for i, t in enumerate(case["texts"]) if t in kept]
        texts = [case["texts"][i] for i in pick]
        n_texts += len(texts)
        for device in (False, True):
            got = _to_numpy(tok.encode_batch(texts, return_offsets=True, add_special_tokens=False, device=device))
            for r, i in enumerate(pick):
                n = len(case["tokens"][i])
                ids = [dense[t] if x < 0 else unk if x >= len(recorded["vocab"]) else x for t, x in zip(case["tokens"][i], case["ids"][i])]
                assert int(got["length"][r]) == n, (case["name"], texts[r])
                assert got["input_ids"][r, :n].tolist() == ids, (case["name"], texts[r])
                assert got["offset_mapping"][r, :n].tolist() == case["offsets"][i], (case["name"], texts[r])
                assert got["word_ids"][r, :n].tolist() == case["word_ids"][i], (case["name"], texts[r])
    assert n_texts >= (44 if cls == "FastWP" else 49)


# ---- reach through the existing forms

TEXTS = ["exam [MASK] is a <user> test.", "ex<user>am", "[MASK]", "", "a test is a test is [mask] a test is a test", "examples is <USER>",
         "is a test of exam [MASK] [MASK] example", "test"]
ADDED = [("[MASK]", True), ("<user>", False)]


def _with_added(swt, ref_dir, cls):
    tok = _tokenizer(swt, ref_dir, cls)
    assert tok.add_special_tokens(["[MASK]"]) == 1 and tok.add_tokens(["<user>"]) == 1
    return tok


@pytest.mark.parametrize("cls", CLASSES)
def test_pairs_with_a_match_in_each_side(swt, dev, ref_dir, cls):
    tok = _with_added(swt, ref_dir, cls)
    n = 4
    a, b = TEXTS[:n], TEXTS[n:2 * n]
    rows, (spans, word) = _model(tok, ADDED, a + b)
    voc, sp = tok._batch_vocabulary(), tok.special_ids()
    pay = ((spans[:n], word[:n]), (spans[n:], word[n:]))
    for truncation, strategy, windows, stride, width in (("longest_first", P.LONGEST_FIRST, False, 0, 16), ("only_second", P.ONLY_SECOND, True, 1, 40),
                                                         ("longest_first", P.LONGEST_FIRST, False, 0, 72)):
        s = P.spec(width, stride, windows, pad_id=sp["pad"], unk_id=sp["unk"], cls_id=sp["cls"], sep_id=sp["sep"])
        want = P.expected_pair_batch(rows[:n], rows[n:], s, strategy, (voc.cmap, voc.n_map, voc.flagged), pay)
        assert not want["refused"]
        for device in (False, True):
            got = _to_numpy(tok.encode_batch(a, text_pairs=b, max_length=width, stride=stride, padding="max_length", truncation=truncation,
                                             return_overflowing=windows, return_offsets=True, device=device))
            for k in KEYS + ("token_type_ids", "sequence_ids"):
                assert np.array_equal(got[k], want[k]), (k, truncation, device)
    assert (want["input_ids"] == tok.mask_id()).sum() == 5  # (the last width truncates nothing)


@pytest.mark.parametrize("cls", CLASSES)
def test_windows_with_an_edge_on_an_added_token(swt, dev, ref_dir, cls):
    tok = _with_added(swt, ref_dir, cls)
    rows, pay = _model(tok, ADDED, TEXTS)
    voc, sp = tok._batch_vocabulary(), tok.special_ids()
    base, edges = voc.added_base, 0
    for cap, stride in ((1, 0), (2, 1), (3, 0), (4, 2), (5, 0)):
        s = B.spec(cap + 2, stride, True, pad_id=sp["pad"], unk_id=sp["unk"], cls_id=sp["cls"], sep_id=sp["sep"])
        want = B.expected_batch(rows, s, (voc.cmap, voc.n_map, voc.flagged), pay)
        edges += sum(1 for r in rows for lo in range(0, len(r), cap - stride) if r[lo] >= base or r[min(lo + cap, len(r)) - 1] >= base)
        for device in (False, True):
            got = _to_numpy(tok.encode_batch(TEXTS, max_length=cap + 2, stride=stride, padding="max_length", return_overflowing=True,
                                             return_offsets=True, device=device))
            for k in KEYS:
                assert np.array_equal(got[k], want[k]), (k, cap, device)
            assert np.array_equal(got["overflow_to_sample_mapping"], want["sample"])
    assert edges > 10


@pytest.mark.parametrize("cls", CLASSES)
def test_packing(swt, dev, ref_dir, cls):
    tok = _with_added(swt, ref_dir, cls)
    rows, _ = _model(tok, ADDED, TEXTS)
    voc, sp = tok._batch_vocabulary(), tok.special_ids()
    width = 16
    s = B.spec(width, pad_id=sp["pad"], unk_id=sp["unk"], cls_id=sp["cls"], sep_id=sp["sep"])
    for packing, mode in (("whole", K.WHOLE), ("split", K.SPLIT)):
        want = K.expected_pack(rows, s, mode, (voc.cmap, voc.n_map, voc.flagged))
        for device in (False, True):
            got = _to_numpy(tok.encode_batch(TEXTS, max_length=width, packing=packing, device=device))
            for k in ("input_ids", "attention_mask", "position_ids", "length"):
                assert np.array_equal(got[k], want[k]), (k, packing, device)
            for k in ("sequence_ids", "sample_ids"):
                assert np.array_equal(got[k], want[k].view(np.int32)), (k, packing, device)
            assert np.array_equal(got["segment_length"], want["seg"])
    assert (want["input_ids"] == tok.mask_id()).sum() == 5  # ("split" cuts no text short)


@pytest.mark.parametrize("cls", CLASSES)
def test_mlm_never_selects_a_special_added_token(swt, dev, ref_dir, cls):
    tok = _with_added(swt, ref_dir, cls)
    voc = tok._batch_vocabulary()
    user = int(voc.added_dense[1])
    for device in (False, True):
        plain = _to_numpy(tok.encode_batch(TEXTS, device=device))
        got = _to_numpy(tok.encode_batch(TEXTS, device=device, mlm={"probability": 1.0, "mask_share": 0.0, "random_share": 0.0}))
        assert np.array_equal(got["input_ids"], plain["input_ids"])  # every selected token is kept
        at_mask, at_user = plain["input_ids"] == tok.mask_id(), plain["input_ids"] == user
        assert at_mask.sum() == 5 and at_user.sum() == 3
        assert (got["labels"][at_mask] == -100).all()  # a special added token is never selected
        assert (got["labels"][at_user] == user).all()  # an ordinary one may be
        rand = _to_numpy(tok.encode_batch(TEXTS * 8, device=device, mlm={"probability": 1.0, "mask_share": 0.0, "random_share": 1.0}))
        assert not (rand["input_ids"][rand["labels"] != -100] == tok.mask_id()).any()  # nor is it a random replacement


def test_bpe_dropout_over_the_blanked_text(swt, dev, ref_dir):
    tok = _with_added(swt, ref_dir, "FastBPE")
    drop = {"probability": 0.3, "seed": 7, "epoch": 2}
    rows, pay = _model(tok, ADDED, TEXTS, drop)
    plain, _ = _model(tok, ADDED, TEXTS)
    assert rows != plain
    voc, sp = tok._batch_vocabulary(), tok.special_ids()
    s = B.spec(max(len(r) for r in rows) + 2, pad_id=sp["pad"], unk_id=sp["unk"], cls_id=sp["cls"], sep_id=sp["sep"])
    want = B.expected_batch(rows, s, (voc.cmap, voc.n_map, voc.flagged), pay)
    for device in (False, True):
        got = _to_numpy(tok.encode_batch(TEXTS, return_offsets=True, device=device, dropout=drop))
        for k in KEYS:
            assert np.array_equal(got[k], want[k]), (k, device)


def test_maxmatch_dropout_over_the_blanked_text(swt, dev, ref_dir):
    from subword_tokenizers_amd import batching
    tok = _with_added(swt, ref_dir, "NaiveWP")
    drop = {"probability": 0.5, "seed": 3, "epoch": 1}
    rows, pay = _model(tok, ADDED, TEXTS, batching.MaxMatch(drop))
    plain, _ = _model(tok, ADDED, TEXTS)
    assert rows != plain
    voc, sp = tok._batch_vocabulary(), tok.special_ids()
    s = B.spec(max(len(r) for r in rows) + 2, pad_id=sp["pad"], unk_id=sp["unk"], cls_id=sp["cls"], sep_id=sp["sep"])
    want = B.expected_batch(rows, s, (voc.cmap, voc.n_map, voc.flagged), pay)
    for device in (False, True):
        got = _to_numpy(tok.encode_batch(TEXTS, return_offsets=True, device=device, maxmatch_dropout=drop))
        for k in KEYS:
            assert np.array_equal(got[k], want[k]), (k, device)


# ---- end to end

@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("cls", CLASSES)
def test_fill_mask_from_a_typed_mask(swt, dev, ref_dir, cls, device):
    tok = _tokenizer(swt, ref_dir, cls)
    text = "paris is the [MASK] of france."
    before = _to_numpy(tok.encode_batch([text], device=device))
    assert not (before["input_ids"] == tok.mask_id()).any()  # "[", "mask", "]"
    assert tok.add_special_tokens(["[MASK]"]) == 1 and tok.add_tokens(["<Capital>"]) == 1
    batch = tok.encode_batch([text, "is [mask] a <capital> test"], device=device, return_offsets=True)
    ids = _to_numpy(batch)["input_ids"]
    words = _to_numpy(batch)["word_ids"][0].tolist()
    cols = [c for c in range(ids.shape[1]) if ids[0, c] == tok.mask_id()]
    assert len(cols) == 1 and words[cols[0]] == 3  # paris, is, the, [MASK]
    assert _to_numpy(batch)["offset_mapping"][0, cols[0]].tolist() == [13, 19]
    # fill_mask over synthetic logits finds that column
    V = max(len(tok.vocab_list()), tok.mask_id() + 1)
    rng = np.random.default_rng(1)
    logits = rng.standard_normal((ids.shape[0], ids.shape[1], V)).astype(np.float32)
    best = tok.token_to_id("<capital>")
    logits[0, cols[0], best] = 50.0
    if device:
        import torch
        logits = torch.from_numpy(logits).cuda()
    out = tok.fill_mask(batch["input_ids"], logits, top_k=2, tokens=True)
    assert out["n_positions"] == 2
    assert _to_numpy(out)["row"].tolist() == [0, 1] and int(_to_numpy(out)["col"][0]) == cols[0]
    assert out["tokens"][0][0] == "<capital>" and int(_to_numpy(out)["token_ids"][0, 0]) == best
    # decode: the special token is skipped or spelled, the ordinary one is spelled with the join rule
    spelled = tok.decode_batch(batch["input_ids"], batch["attention_mask"], skip_special_tokens=False)
    skipped = tok.decode_batch(batch["input_ids"], batch["attention_mask"])
    assert "[MASK]" in spelled[0] and "[MASK]" in spelled[1] and "[MASK]" not in skipped[0] + skipped[1]
    assert " a <capital> " in skipped[1] and " a <capital> " in spelled[1]


@pytest.mark.parametrize("cls", CLASSES)
def test_the_list_survives_train(swt, dev, ref_dir, corpora, cls):
    """train builds a new vocabulary: the added tokens stay, their dense ids follow it, and encode_batch finds them"""
    tok = getattr(swt, cls)()
    assert tok.add_special_tokens(["[MASK]"]) == 1 and tok.add_tokens(["<user>"]) == 1
    tok.train(list(corpora["pan"])[:40], 200)
    assert tok.added_tokens() == [("[MASK]", True), ("<user>", False)]
    base = len(tok.vocab_list()) - 2
    assert tok.vocab_list()[base:] == ["[MASK]", "<user>"] and tok.mask_id() == base and tok.token_to_id("<user>") == base + 1
    text = "a [mask] a<USER>"
    for device in (False, True):
        got = _to_numpy(tok.encode_batch([text], return_offsets=True, device=device))
        n = int(got["length"][0])
        ids = got["input_ids"][0, :n].tolist()
        assert ids[2] == base and ids[-2] == base + 1 and n == 6  # [CLS] a [MASK] a <user> [SEP]
        assert got["offset_mapping"][0, [2, 4]].tolist() == [[2, 8], [10, 16]] and got["word_ids"][0, :n].tolist() == [-1, 0, 1, 2, 3, -1]
    tok.reset()
    assert tok.added_tokens() == [("[MASK]", True), ("<user>", False)]


# ---- unchanged when unused

@pytest.mark.parametrize("cls", CLASSES)
def test_unchanged_when_unused(swt, dev, ref_dir, cls):
    tok = _tokenizer(swt, ref_dir, cls)
    texts = _kept(tok, [], ["exam [MASK] is a <user> test.", "examples", "", "a [mask] test", "exam mask user"])
    assert len(texts) >= 3
    base_list = tok.vocab_list()
    before = [_to_numpy(tok.encode_batch(texts, return_offsets=True, device=device)) for device in (False, True)]
    tok.add_special_tokens(["[MASK]", "<user>"])
    assert tok.encode_batch(["[MASK] <user>"])["input_ids"].shape == (1, 4)  # [CLS] [MASK] <user> [SEP]
    tok.clear_added_tokens()
    assert tok.vocab_list() == base_list and tok.added_tokens() == []
    for device in (False, True):
        after = _to_numpy(tok.encode_batch(texts, return_offsets=True, device=device))
        assert set(after) == set(before[device])
        for k, v in after.items():
            assert np.array_equal(v, before[device][k]), (k, device)
