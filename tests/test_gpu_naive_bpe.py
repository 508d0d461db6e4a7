"""NaiveBPE.encode_ids_batch / tokenize_batch on the device (swt_bpe_encode_naive*, the ordered form of bpe_lane_kernel) against the
reference's output (tests/golden/naivebpe.json) and the rising-floor model of tests/test_naive_bpe_encode.py.  Needs an MI355X."""
import json
import os
import random

import numpy as np
import pytest

from tests.test_naive_bpe_encode import NOT_ORDER_EQUIVALENT, RisingFloor, naivebpe_cases, splitter

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(native):
    if native.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests need an MI355X (there is no CPU fallback to test)")
    native.init(0)
    return native


@pytest.fixture(scope="module")
def pre_merges(ref_dir):
    with open(os.path.join(ref_dir, "resources/pretrained/FastBPE/merges.json"), encoding="utf-8") as f:
        return [tuple(p) for p in json.load(f)]


def naive(swt, merges):
    tok = swt.NaiveBPE()
    tok.merges_list = [tuple(p) for p in merges]
    return tok


def improper(merges, at):
    """the list with two DEPENDENT merges swapped (the second's left symbol is what the first produces): not proper any more"""
    merges = list(merges)
    for i in range(at, len(merges)):
        made = merges[i][0] + merges[i][1]
        for j in range(i + 1, len(merges)):
            if merges[j][0] == made:
                merges[i], merges[j] = merges[j], merges[i]
                return merges
    raise AssertionError("no dependent pair of merges")


def tokens_of(tok, ids, off):
    toks = tok.decode_ids(ids)
    return [toks[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]


def test_reference_fixture_every_case_three_ways(swt, dev):
    for name, merges, texts, tokens, _ in naivebpe_cases():
        tok = naive(swt, merges)
        ids, off = tok.encode_ids_batch(texts)  # one batch (the joined path where the case has more than 64 texts ...)
        assert tokens_of(tok, ids, off) == tokens, name
        ids, off = tok.encode_ids_batch(texts[:50])  # ... and the host-lowercase path
        assert tokens_of(tok, ids, off) == tokens[:50], name
        assert tok.tokenize_batch(texts) == tokens, name
        assert tok._ensure_naive_table().order_equivalent() == (name not in NOT_ORDER_EQUIVALENT), name
        for i, want in enumerate(tokens[:90]):  # one sentence per call: the single-workgroup form
            assert tok.tokenize_batch([texts[i]]) == [want], (name, texts[i][:60])


def test_pan_tadeusz_is_the_authors_list_and_fastbpes_ids(swt, dev, pre_merges, corpora):
    tok = naive(swt, pre_merges)
    assert tok.tokenize_batch(corpora["pan"]) == corpora["pan_tokens"]["FastBPE"]  # the author's NaiveBPE list (identical to FastBPE's)
    fast = swt.FastBPE()
    fast.merges_list = list(pre_merges)
    fast._build_table()
    for texts in (corpora["pan"], corpora["pan"][:40], [corpora["pan"][3]]):
        a, b = tok.encode_ids_batch(texts), fast.encode_ids_batch(texts)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])  # order-equivalent table: bit for bit


def test_train5k_with_a_table_trained_on_the_device(swt, dev, corpora):
    tok = swt.NaiveBPE()
    tok.train(corpora["t5k"], 1000)
    fast = swt.FastBPE()
    fast.train(corpora["t5k"], 1000)
    assert fast.merges_list == tok.merges_list
    table = tok._ensure_naive_table()
    assert table.order_equivalent() and tok._naive_syms.strings == tok._train_syms.strings  # the ids the trainer named, reused
    a, b = tok.encode_ids_batch(corpora["t5k"]), fast.encode_ids_batch(corpora["t5k"])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    m, split = RisingFloor(tok.merges_list), splitter()
    out = tok.tokenize_batch(corpora["t5k"])
    for i in range(0, len(out), 9):
        assert out[i] == m.tokenize(corpora["t5k"][i], split), i
    assert tok.tokenize_batch(corpora["t5k"][:30]) == [tok.tokenize(t) for t in corpora["t5k"][:30]]  # == the Python loop
    # the same merges made improper: the ordered form of the kernel
    bad = naive(swt, improper(tok.merges_list, 100))
    assert not bad._ensure_naive_table().order_equivalent()
    m, out = RisingFloor(bad.merges_list), bad.tokenize_batch(corpora["t5k"])
    for i in range(0, len(out), 9):
        assert out[i] == m.tokenize(corpora["t5k"][i], split), i
    tok.merges_list.pop()  # changed in place: the handle follows
    assert tok._ensure_naive_table() is not table and tok._ensure_naive_table().n_merges == len(tok.merges_list)
    assert tok.tokenize_batch(corpora["t5k"][:30]) == [tok.tokenize(t) for t in corpora["t5k"][:30]]


def test_s85k_under_every_dedup_mode(swt, dev, corpora):
    """>= 20,000 sentences, SWT_OPT_DEDUP 0/1/2 identical, for an order-equivalent table and for the ordered path; a sample
    against the model (word-memoised)"""
    from subword_tokenizers_amd import synth

    s85k = synth.s85k()[:24000]
    trained = swt.NaiveBPE()
    trained.train(corpora["t5k"], 1500)
    split = splitter()
    for merges, equivalent in ((trained.merges_list, True), (improper(improper(trained.merges_list, 50), 400), False)):
        tok = naive(swt, merges)
        table = tok._ensure_naive_table()
        assert table.order_equivalent() == equivalent
        got = []
        for mode in (dev.DEDUP_AUTO, dev.DEDUP_NEVER, dev.DEDUP_ALWAYS):
            table.set_option(dev.OPT_DEDUP, mode)
            got.append(tok.encode_ids_batch(s85k))
        for ids, off in got[1:]:
            assert np.array_equal(ids, got[0][0]) and np.array_equal(off, got[0][1])
        m = RisingFloor(merges)
        out = tokens_of(tok, *got[0])
        for i in range(0, len(s85k), 16):
            assert out[i] == m.tokenize(s85k[i], split), (equivalent, i)


def test_random_improper_tables_fuzz(swt, dev):
    """lists with repeated and misordered pairs over a small alphabet against the Python NaiveBPE.encode_word loop"""
    rng = random.Random(20260114)
    n_ordered = 0
    for trial in range(60):
        alpha = rng.choice(["ab", "abc", "abcd", "aąb€"])
        pool = list(alpha)
        merges = []
        for _ in range(rng.randint(1, 14)):
            kind = rng.random()
            if merges and kind < 0.2:
                pair = rng.choice(merges)  # a repeat
            else:
                pair = (rng.choice(pool), rng.choice(pool))
                if kind > 0.5:
                    pool.append(pair[0] + pair[1])  # later merges may use it, and earlier ones after the shuffle below
            merges.append(pair)
        if rng.random() < 0.6:
            rng.shuffle(merges)
        tok = naive(swt, merges)
        n_ordered += not tok._ensure_naive_table().order_equivalent()
        words = ["".join(rng.choice(alpha) for _ in range(rng.choice([1, 2, 3, 5, 8, 13, 21, 34, 40, 70]))) for _ in range(40)]
        want = [tok.encode_word(w) for w in words]
        assert tok.tokenize_batch([" ".join(words)]) == [sum(want, [])], (trial, merges)
        assert tok.tokenize_batch(words) == want, (trial, merges)
        # SWT_BPE_RAW_WORDS = encode_word batched: nothing splits, not even at punctuation or white space
        raw = words + ["a.b", "a b", "ab!!ab"]
        text, off = dev.pack_utf8(raw)
        ids, ooff = tok._ensure_naive_table().encode_naive(text, off, flags=dev.BPE_RAW_WORDS)
        assert tokens_of(tok, ids, ooff) == [tok.encode_word(w) for w in raw], (trial, merges)
    assert n_ordered > 30


def test_unpacked_table_long_and_giant_words(swt, dev):
    """a merged-symbol index >= 0xFFFF (unpacked table values), words beyond 32 symbols and beyond a 512-byte chunk"""
    lib = dev.lib()
    import ctypes
    lib.swt_debug_bpe_table_info.restype = ctypes.c_int
    lib.swt_debug_bpe_table_info.argtypes = [ctypes.c_void_p, ctypes.c_int]
    # 66,000 merges of distinct two-letter pairs over a large alphabet push the merged indices past 16 bits; in front of them a
    # few that matter, out of order and repeated
    head = [("ab", "ab"), ("a", "b"), ("ab", "ab"), ("x", "xx"), ("x", "x"), ("xx", "xx"), ("x", "x"), ("abab", "c"), ("c", "abab")]
    filler = [(chr(0x4E00 + i // 300), chr(0x5E00 + i % 300)) for i in range(66000)]
    tail = [("abab", "abab"), ("xx", "x"), ("y", "y"), ("yy", "yy"), ("y", "y")]
    merges = head + filler + tail
    tok = naive(swt, merges)
    table = tok._ensure_naive_table()
    assert lib.swt_debug_bpe_table_info(table._h, 1) == 0 and not table.order_equivalent()
    small = naive(swt, head + tail)  # the same merges that can apply, in a packed table
    assert lib.swt_debug_bpe_table_info(small._ensure_naive_table()._h, 1) == 1
    texts = ["abab", "ab" * 20, "x" * 45, "abc" * 30, "ab" * 400 + "c", "x" * 700, "y" * 1500 + " ab" * 10, "x" * 5000,
             "cabab ababc " * 30, chr(0x4E00) + chr(0x5E00) + "ab", "xyxxy" * 9, "a" * 33 + "b"]
    m = RisingFloor(head + tail)
    want = [m.tokenize(t, splitter()) for t in texts[:9] + texts[10:]]
    for t in (tok, small):
        assert t.tokenize_batch(texts[:9] + texts[10:]) == want
        for text, w in zip(texts[:9] + texts[10:], want):
            assert t.tokenize_batch([text]) == [w], text[:40]
    assert tok.tokenize_batch([texts[9]]) == [[chr(0x4E00) + chr(0x5E00), "##ab"]]
    # many sentences around it: tiles of running text (Mode 0), and the unique-word pass of the dedup path (Mode 1)
    many = (texts[:9] + texts[10:]) * 40
    for t in (tok, small):
        for mode in (dev.DEDUP_NEVER, dev.DEDUP_ALWAYS):
            t._ensure_naive_table().set_option(dev.OPT_DEDUP, mode)
            assert t.tokenize_batch(many) == want * 40, mode


def test_joined_path_and_host_lowercase(swt, dev):
    merges = [("ab", "c"), ("a", "b"), ("ż", "ó"), ("a", "b"), ("i", "s"), ("σ", "α"), ("α", "σ")]
    tok, m, split = naive(swt, merges), RisingFloor(merges), splitter()
    many = ["Zażółć ABC abcab Jaźń %d" % i for i in range(100)]
    assert tok.tokenize_batch(many) == [m.tokenize(t, split) for t in many]
    mixed = many[:50] + ["İstanbul ǅungla ΣΑΣ abc"] + many[50:]
    assert tok.tokenize_batch(mixed) == [m.tokenize(t, split) for t in mixed]
    table = tok._ensure_naive_table()
    joined, _ = dev.join_texts(mixed)
    assert table.encode_naive_joined(joined, 101) is None  # the device flags it; the class goes the host-lowercase way
    joined, _ = dev.join_texts(many)
    ids, off = table.encode_naive_joined(joined, 100)
    assert tokens_of(tok, ids, off) == [m.tokenize(t, split) for t in many]
    for texts in ([], [""], ["", "", ""], ["", "abc", "", "b", ""]):
        assert tok.tokenize_batch(texts) == [m.tokenize(t, split) for t in texts]


def test_encode_naive_dev_on_torch_tensors_and_a_side_stream(swt, dev):
    import torch

    merges = [("ab", "c"), ("a", "b"), ("b", "c"), ("a", "b"), ("abc", "abc")]
    tok, m, split = naive(swt, merges), RisingFloor(merges), splitter()
    texts = ["abc abcabc cab", "bcab ab", "", "abcabcabc " * 300] * 50
    text, off = dev.pack_and_lower(texts)
    want_ids, want_off = tok._ensure_naive_table().encode_naive(text, off)
    assert tokens_of(tok, want_ids, want_off)[:4] == [m.tokenize(t, split) for t in texts[:4]]
    d_text = torch.from_numpy(np.concatenate([text, np.zeros(64, np.uint8)])).cuda()
    d_off = torch.from_numpy(off.astype(np.int64)).cuda()
    d_out = torch.zeros(int(text.size) + 64, dtype=torch.int32, device="cuda")
    d_out_off = torch.zeros(len(texts) + 1, dtype=torch.int64, device="cuda")
    d_n = torch.zeros(1, dtype=torch.int64, device="cuda")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        tok._ensure_naive_table().encode_naive_dev(d_text.data_ptr(), int(text.size), d_off.data_ptr(), len(texts), d_out.data_ptr(),
                                                   d_out_off.data_ptr(), d_n.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    n = int(d_n.item())
    assert n == want_ids.size
    assert np.array_equal(d_out[:n].cpu().numpy().view(np.uint32), want_ids)
    assert np.array_equal(d_out_off.cpu().numpy().astype(np.uint64), want_off)
