"""Sampled UnigramWP on the device against the model of tests/sample_cases.py, element by element, at every seam (MI355X)."""
import numpy as np
import pytest

from tests import batch_cases as B
from tests import sample_cases as S
from tests.test_gpu_viterbi import SCORES, TEXTS, dev  # noqa: F401  (dev: the fixture)

pytestmark = pytest.mark.gpu
LOG, SEED, EPOCH = SCORES["log"], 0x123456789ABCDEF0, 3
WEIGHTS = {"log at 0.1": S.weights(LOG, 0.1), "log at 1": S.weights(LOG, 1.0), "alpha 0": S.weights(LOG, 0.0),
           "2^-64": {t: 2.0 ** -64 for t in S.HANDMADE}}  # (the last: the exponent path, "x" * 100 stands in the first text)


def make(swt, dev, kind, max_word_chars=100):  # -> (the tokenizer, encode(texts, seed, epoch) by the weights as given, the model)
    tok = swt.UnigramWP(max_word_chars=max_word_chars)
    tok.vocab = set(S.HANDMADE)
    tok.set_scores(LOG)
    trie = tok._ensure_scored_trie()
    trie.set_weights([WEIGHTS[kind][t] for t in sorted(S.HANDMADE)])
    return tok, lambda texts, seed=SEED, epoch=EPOCH: trie.encode_sample(*dev.pack_and_lower(texts), (None, seed, epoch)), \
        S.Model(S.HANDMADE, WEIGHTS[kind], max_word_chars)


def same(got, want, what):
    assert all(np.array_equal(np.asarray(g, dtype=w.dtype), w) for g, w in zip(got[::-1], want[::-1])), what


CASES = [(name, kind, chars) for name in TEXTS for kind in WEIGHTS for chars in (100, 4)
         if not name.startswith("host") or (kind, chars) == ("log at 0.1", 100)]


@pytest.mark.parametrize("name,kind,max_word_chars", CASES)
def test_the_device_equals_the_model(swt, dev, name, kind, max_word_chars):
    _, encode, model = make(swt, dev, kind, max_word_chars)
    same(encode(TEXTS[name]), model.batch(swt.SubwordTokenizer._split, TEXTS[name], SEED, EPOCH), name)


def test_a_draw_goes_by_seed_epoch_and_index(swt, dev):
    _, encode, model = make(swt, dev, "log at 0.1")
    texts, split = TEXTS["tiles"], swt.SubwordTokenizer._split
    first, other = encode(texts), encode(texts, epoch=EPOCH + 1)
    same(encode(texts), first, "the same (seed, epoch) twice")
    same(other, model.batch(split, texts, SEED, EPOCH + 1), "another epoch")
    assert not np.array_equal(other[0], first[0])
    for s in (7, 45):  # alone at index s (behind empty sentences, in one workgroup) as inside the tiled batch at index s
        alone = encode([""] * s + [texts[s]])
        assert np.array_equal(alone[0], first[0][int(first[1][s]):int(first[1][s + 1])]) and alone[0].size


def test_encode_batch_on_the_device(swt, dev):
    tok, _, _ = make(swt, dev, "log at 1")
    model = S.Model(S.HANDMADE, S.weights(LOG, 0.5))  # (the weights that the Python layer makes of the scores at this alpha)
    texts, split = TEXTS["single workgroup"], swt.SubwordTokenizer._split
    rows, spans, word = [], [], []
    for s, text in enumerate(texts):
        rows.append([]), spans.append([]), word.append([])
        for w, ((piece_word, (start, end)), (_, a0)) in enumerate(zip(split(text.lower()), S.words_of(split, text.lower()))):
            at = start
            for t in model.encode_word(piece_word, SEED, EPOCH, s, a0):
                width = end - start if t == "[UNK]" else len(t) - 2 * (at > start)
                rows[-1].append(model.ids.get(t, model.unk)), spans[-1].append((at, at + width)), word[-1].append(w)
                at += width
    voc, sp = tok._batch_vocabulary(), tok.special_ids()
    s = B.spec(12, pad_id=sp["pad"], unk_id=sp["unk"], cls_id=sp["cls"], sep_id=sp["sep"])
    want = B.expected_batch(rows, s, (voc.cmap, voc.n_map, voc.flagged), (spans, word))
    sample = {"alpha": 0.5, "seed": SEED, "epoch": EPOCH}
    got = tok.encode_batch(texts, max_length=12, padding="max_length", return_offsets=True, device=True, sample=sample)
    for k in ("input_ids", "attention_mask", "offset_mapping", "word_ids"):
        assert np.array_equal(got[k].cpu().numpy(), want[k]), k
    assert tok.tokenize_batch(texts, sample=sample) == model.tokenize(split, texts, SEED, EPOCH)
    assert tok.tokenize(texts[2], sample=sample) == model.tokenize(split, texts[2:3], SEED, EPOCH)[0]


def test_what_is_refused(swt, dev):
    for call in [getattr(getattr(swt, cls)(), name) for cls in ("NaiveWP", "FastBPE") for name in ("encode_ids_batch", "tokenize_batch", "encode_batch")]:
        with pytest.raises(ValueError):
            call(["ab"], sample={"alpha": 0.1})
    tok = make(swt, dev, "alpha 0")[0]
    for bad in ({"alpha": -1.0}, {"alpha": float("nan")}, {"alpha": float("inf")}, {"seed": 1 << 64}, {"epoch": 1 << 32}, {"beta": 1}):
        pytest.raises(ValueError, tok.encode_ids_batch, ["ab"], sample=bad)
