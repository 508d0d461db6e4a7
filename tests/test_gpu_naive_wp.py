"""NaiveWP.encode_ids_batch / tokenize_batch on the device (swt_wp_encode_naive*, wp_naive_kernel) against the reference's
output (tests/golden/naivewp.json) and the bounded MaxMatch model of tests/test_naive_wp_encode.py.  Needs an MI355X."""
import json
import os

import numpy as np
import pytest

from tests.test_naive_wp_encode import MaxMatch, naivewp_cases, splitter

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(native):
    if native.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests need an MI355X (there is no CPU fallback to test)")
    native.init(0)
    return native


@pytest.fixture(scope="module")
def pre_vocab(ref_dir):
    with open(os.path.join(ref_dir, "resources/pretrained/FastWordPiece/vocab.json"), encoding="utf-8") as f:
        return json.load(f)


def naive(swt, vocab):
    tok = swt.NaiveWP()
    tok.vocab = set(vocab)
    return tok


def model_batch(m, texts):
    """(ids, offsets, status) as the device must give them"""
    split = splitter()
    ids, off, st = [], [0], []
    for t in texts:
        toks = m.tokenize(t, split)
        st.append(0 if toks is not None else 1)
        if toks is not None:
            ids += m.ids_of(toks)
        off.append(len(ids))
    return np.array(ids, dtype=np.uint32), np.array(off, dtype=np.uint64), np.array(st, dtype=np.uint8)


def same(tok, m, texts):
    ids, off, st = tok.encode_ids_batch(texts)
    wids, woff, wst = model_batch(m, texts)
    assert np.array_equal(st, wst)
    assert np.array_equal(off, woff)
    assert np.array_equal(ids, wids)
    return ids, off, st


def test_reference_fixture_every_case(swt, dev):
    for name, vocab, texts, tokens in naivewp_cases():
        tok, m = naive(swt, vocab), MaxMatch(vocab)
        ids, off, st = same(tok, m, texts)  # one batch (the joined path when > 64 texts)
        for i, want in enumerate(tokens):
            assert (st[i] != 0) == (want == "TIMEOUT"), (name, texts[i][:60])
        ok = [i for i, w in enumerate(tokens) if w != "TIMEOUT"]
        assert tok.tokenize_batch([texts[i] for i in ok]) == [tokens[i] for i in ok], name
        for i, want in enumerate(tokens[:80]):  # one sentence per call: the single-launch form
            if want == "TIMEOUT":
                with pytest.raises(RuntimeError):
                    tok.tokenize_batch([texts[i]])
            else:
                assert tok.tokenize_batch([texts[i]]) == [want], (name, texts[i][:60])


def test_pan_tadeusz_is_the_authors_list(swt, dev, pre_vocab, corpora):
    tok = naive(swt, pre_vocab)
    out = tok.tokenize_batch(corpora["pan"])
    assert out == corpora["pan_tokens"]["FastWordPiece"]  # the author's NaiveWordPiece list (identical to FastWordPiece's)
    assert tok.tokenize_batch([corpora["pan"][3]]) == [out[3]]


def test_s85k_and_train5k_sentence_by_sentence(swt, dev, pre_vocab, corpora):
    """>= 20,000 sentences against the model: S85k with the pretrained vocabulary, train-5K with it and with a vocabulary
    NaiveWP.train made on the device"""
    from subword_tokenizers_amd import synth

    tok, m = naive(swt, pre_vocab), MaxMatch(pre_vocab)
    s85k = synth.s85k()[:20000]
    _, _, st = same(tok, m, s85k)
    same(tok, m, corpora["t5k"])
    trained = swt.NaiveWP()
    trained.train(corpora["t5k"], 3000)
    _, _, st2 = same(trained, MaxMatch(trained.vocab), corpora["t5k"])
    assert not st2.any()  # a vocabulary trained on the text covers it
    # tokenize_batch == [tokenize(t) ...] wherever the reference returns
    texts = [t for t, s in zip(s85k[:300], st[:300]) if not s]
    assert tok.tokenize_batch(texts) == [tok.tokenize(t) for t in texts]


def test_paths_and_shapes(swt, dev, pre_vocab):
    tok, m = naive(swt, pre_vocab), MaxMatch(pre_vocab)
    cases = [
        [], [""], ["", "", ""], ["", "a", "", "b", ""],
        ["słowo " * 3000],                                   # one sentence longer than the LDS chunk (one lane, global memory)
        ["x" * 20000], ["nie wiem " * 700, "a", "tak " * 1200, ""],
        ["a" * 4095, "b" * 4096, "c" * 4097, "d" * 2047, "e" * 2048, "f" * 2049],
        ["wyraz"] * 3000, ["w " * 2500],
        ["dom"] * 64, ["dom"] * 65, ["d" * 2048], ["d" * 2049],  # the single-launch form's edges
        ["hello!", "a ## b", "(a", "ok", "abc€def", "dobrze"],
        ["5×2km", "˝zgoda˝", "áb", "zażółć gęślą jaźń", "a b", "a b c　d"],
    ]
    for texts in cases:
        same(tok, m, texts)
    # the joined path (> 64 texts) and its fallback for a sentence only the host lowercases (need_host)
    many = ["Zażółć Gęślą Jaźń %d" % i for i in range(100)]
    same(tok, m, many)
    same(tok, m, many[:50] + ["İstanbul ǅungla ΣΑΣ"] + many[50:])
    trie = tok._ensure_naive_trie()
    joined, _ = dev.join_texts(many[:50] + ["İstanbul"] + many[50:])
    assert trie.encode_naive_joined(joined, 101) is None  # the device flags it; the class goes the host-lowercase way
    joined, _ = dev.join_texts(many)
    got = trie.encode_naive_joined(joined, 100)
    assert all(np.array_equal(a, b) for a, b in zip(got, model_batch(m, many)))


def test_vocabulary_changes_rebuild_the_handle(swt, dev):
    tok = naive(swt, ["a", "##b"])
    assert tok.tokenize_batch(["ab", "abc"]) == [["a", "##b"], ["[UNK]"]]
    tok.vocab.add("##c")  # changed in place
    assert tok.tokenize_batch(["abc"]) == [["a", "##b", "##c"]]
    tok.reset()
    assert tok.tokenize_batch(["abc"]) == [["[UNK]"]]


def test_vocabulary_with_excess_tokens_is_refused(swt, dev):
    tok = naive(swt, ["a", "#", "###b"])  # "ab" -> a, #, ###b: more tokens than bytes
    with pytest.raises(dev.SwtError) as e:
        tok.encode_ids_batch(["ab"])
    assert e.value.code == dev.ERR_UNSUPPORTED


def test_quality_metrics_equal_the_per_call_python_metrics(swt, dev, pre_vocab, corpora):
    from subword_tokenizers_amd import metrics as M

    tok = naive(swt, pre_vocab)
    corpus = corpora["pan"][:400]
    got = M.quality_metrics(tok, corpus)
    inputs = [tok.tokenize(s) for s in corpus]  # the reference's own per-call path (benchmarks.py:333-337)
    words = {w for sent in tok.preprocessing(corpus) for w, _ in sent}
    by_word = {w: tok.tokenize(w) for w in words}
    chars = sum(len(s.replace(" ", "")) for s in corpus)
    total = sum(len(t) for t in inputs)
    want = {"avg_tokens_per_sentence": M.avg_tokens_per_sentence(inputs), "avg_tokens_per_word": M.avg_tokens_per_word(by_word),
            "compression_rate": M.compression_rate(chars, inputs), "normalized_sequence_length": M.normalized_sequence_length(total, chars),
            "subword_fragmentation_rate": M.subword_fragmentation_rate(by_word),
            "vocabulary_coverage_rate": M.vocabulary_coverage_rate(by_word)}
    for k, v in want.items():
        assert got[k] == pytest.approx(v, rel=1e-12), k
    z = M.zipf_distribution(inputs)
    for k in ("slope", "intercept", "correlation"):
        assert got["zipf"][k] == pytest.approx(z[k], rel=1e-9, abs=1e-12), k


def test_cli_tokenize_naive_wordpiece(swt, dev, ref_dir, corpora, tmp_path, monkeypatch, capsys):
    import shutil

    from subword_tokenizers_amd import cli

    os.makedirs(tmp_path / "resources" / "pretrained")
    shutil.copytree(os.path.join(ref_dir, "resources", "pretrained", "FastWordPiece"), tmp_path / "resources" / "pretrained" / "NaiveWordPiece")
    os.makedirs(tmp_path / "data")
    shutil.copy(os.path.join(ref_dir, "data", "pan_tadeusz.json"), tmp_path / "data" / "pan_tadeusz.json")
    monkeypatch.chdir(tmp_path)
    assert cli.main(["-m", "NaiveWordPiece", "--pretrained", "pretrained", "--tokenize", "data/pan_tadeusz.json"]) == 0
    capsys.readouterr()
    got = json.loads((tmp_path / "data" / "pan_tadeusz.tokens.json").read_text(encoding="utf-8"))
    assert got == {"NaiveWordPiece": corpora["pan_tokens"]["FastWordPiece"]}
