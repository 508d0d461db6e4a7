"""Decoding without a GPU: the Python model (tests/decode_cases.py) against the reference's recorded strings
(tests/golden/recover_sentence.json), the Vocabulary's tables against the model's flags, and what the host forms of
swt_decode_plan / swt_decode_rows refuse from their arguments alone."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

from tests import decode_cases as D


@pytest.fixture(scope="module")
def recorded(golden):
    return golden("recover_sentence.json")


def test_fixture_shape(recorded):
    assert recorded["alphabet"] == D.ALPHABET and recorded["fuzz_alphabet"] == D.FUZZ_ALPHABET
    assert len(recorded["exhaustive"]) == 1 + 14 + 14 ** 2 + 14 ** 3 == 2955
    assert len(recorded["fuzz"]) == 2000
    assert {k: len(v) for k, v in recorded["pan_tadeusz"].items()} == {"FastBPE": 989, "FastWordPiece": 989}


def test_model_equals_the_reference_on_every_short_row(recorded):
    rows = [list(r) for n in range(4) for r in itertools.product(D.ALPHABET, repeat=n)]
    assert [D.join(r) for r in rows] == recorded["exhaustive"]


def test_model_equals_the_reference_on_the_fuzz(recorded):
    for row, want in recorded["fuzz"]:
        assert D.join([D.FUZZ_ALPHABET[i] for i in row]) == want, row


@pytest.mark.parametrize("name", ["FastBPE", "FastWordPiece"])
def test_model_equals_the_reference_on_the_recorded_rows(recorded, corpora, name):
    assert [D.join(r) for r in corpora["pan_tokens"][name]] == recorded["pan_tadeusz"][name]


def test_id_model_equals_the_string_model(recorded):
    """decode() over ids and tables spells what join() spells over strings, skipped columns and specials aside"""
    tabs = D.tables(D.FUZZ_ALPHABET)
    rows = [r for r, _ in recorded["fuzz"]]
    width = max(len(r) for r in rows)
    ids = np.full((len(rows), width), -5, dtype=np.int64)
    mask = np.zeros(ids.shape, dtype=np.uint8)
    for i, r in enumerate(rows):
        ids[i, :len(r)], mask[i, :len(r)] = r, 1
    text, off, status, info = D.decode(ids, mask, tabs, flags=0)
    assert D.strings(text, off) == [s for _, s in recorded["fuzz"]]
    assert not status.any() and info.tolist() == [text.size, 0, sum(map(len, rows))]
    text, off, status, info = D.decode(ids, mask, tabs, flags=D.SKIP_SPECIAL)
    assert D.strings(text, off) == [D.join([D.FUZZ_ALPHABET[i] for i in r if D.FUZZ_ALPHABET[i] not in D.SKIPPED]) for r in rows]


def test_whitespace_list_is_pythons():
    assert {c for c in range(0x110000) if re.match(r"\s", chr(c))} == set(D.WS)


def test_model_reports_and_skips():
    ix, mask_id = D.toy_ids()
    tabs = D.tables(D.TOY, mask_id)
    assert tabs[3] == len(D.TOY) + 1 and tabs[2][mask_id] == D.SPECIAL
    ids = np.array([[ix["ab"], -1, ix["##cd"], mask_id], [ix["ab"], D.TOY_BAD, ix["##cd"], mask_id + 1], [ix["[PAD]"], ix["##cd"], ix["[UNK]"], ix["."]]],
                   dtype=np.int32)
    text, off, status, info = D.decode(ids, None, tabs)
    assert D.strings(text, off) == ["abcd", "abcd", "##cd [UNK]."] and status.tolist() == [1, 3, 0] and info.tolist() == [19, 2, 10]
    mask = np.array([[1, 0, 1, 1], [1, 0, 1, 0], [1, 1, 1, 1]], dtype=np.uint8)
    text, off, status, info = D.decode(ids, mask, tabs, flags=0)
    assert D.strings(text, off) == ["abcd [MASK]", "abcd", "[PAD]cd [UNK]."] and not status.any() and info.tolist() == [29, 0, 9]


# ---- the Vocabulary's tables

def _check_tables(voc):
    tok_bytes, tok_off, tok_flags, n_tok = voc.decode_tables
    tokens = list(voc.tokens) + ([D.MASK] if voc.mask_id == len(voc.tokens) else [])
    want = D.tables(voc.tokens, voc.mask_id)
    assert n_tok == want[3] == len(tokens)
    assert np.array_equal(tok_off, want[1]) and tok_off.dtype == np.uint32
    assert np.array_equal(tok_flags, want[2]) and tok_flags.dtype == np.uint8
    assert tok_bytes[:int(tok_off[-1])].tobytes() == "".join(tokens).encode("utf-8")
    return tok_flags


@pytest.mark.parametrize("cls", ["FastBPE", "NaiveBPE", "FastWP", "NaiveWP"])
def test_vocabulary_tables_of_the_pretrained_models(swt, ref_dir, cls):
    tok = getattr(swt, cls)()
    tok.load_resources(os.path.join(ref_dir, "resources/pretrained", "FastBPE" if "BPE" in cls else "FastWordPiece"))
    voc = tok._batch_vocabulary()
    flags = _check_tables(voc)
    assert not (flags & D.BAD).any()  # neither pretrained vocabulary holds a token the rule does not spell
    special = {voc.special[k] for k in ("pad", "cls", "sep")} | {voc.mask_id}
    assert set(np.flatnonzero(flags & D.SPECIAL).tolist()) == special


def test_vocabulary_tables_of_a_toy_vocabulary(swt):
    from subword_tokenizers_amd import batching
    voc = batching.wp_vocabulary(sorted(["ab", "##cd", "", "a\u001db", "x　", "’", "##", "###", "(", ".", "x’", "##(", "[MASK]"]))
    flags = _check_tables(voc)
    by = dict(zip(voc.tokens, flags.tolist()))
    assert by[""] == by["a\u001db"] == by["x　"] == D.BAD
    assert by["’"] == D.NO_SPACE_BEFORE | D.NO_SPACE_AFTER and by["##"] == 0 and by["###"] == D.GLUE and by["##("] == D.GLUE | D.NO_SPACE_AFTER
    assert by["[MASK]"] == by["[PAD]"] == D.SPECIAL and by["[UNK]"] == 0
    no_mask = batching.wp_vocabulary(sorted(["ab", "##cd"]))
    assert no_mask.mask_id == len(no_mask.tokens)
    flags = _check_tables(no_mask)
    assert flags.size == len(no_mask.tokens) + 1 and flags[-1] == D.SPECIAL


# ---- the built library, without a device

NAMES_PLAN = ("ids", "mask", "tok_off", "tok_flags", "text_off", "status", "info")
NAMES_ROWS = ("ids", "mask", "tok_bytes", "tok_off", "tok_flags", "text_off", "out_text")


def _bufs():
    tabs = D.tables(D.TOY, len(D.TOY))
    ids = np.full((3, 4), 4, dtype=np.int32)
    text, off, _, _ = D.decode(ids, None, tabs)
    return {"ids": ids, "mask": None, "tok_bytes": tabs[0], "tok_off": tabs[1], "tok_flags": tabs[2], "n_tok": tabs[3], "text_off": off,
            "status": np.zeros(3, dtype=np.uint8), "info": np.full(3, 9, dtype=np.uint64), "out_text": np.zeros(text.size, dtype=np.uint8)}


def _call(native, form, rows=None, width=None, n_tok=None, flags=1, text_cap=None, **given):
    b = _bufs()
    b.update({k: v for k, v in given.items() if isinstance(v, np.ndarray)})
    p = {k: None if given.get(k, True) is False or b[k] is None else b[k].ctypes.data for k in set(NAMES_PLAN + NAMES_ROWS)}
    lib = native.lib()
    head = (p["ids"], p["mask"], 3 if rows is None else rows, 4 if width is None else width)
    n_tok = b["n_tok"] if n_tok is None else n_tok
    if form == "plan":
        rc = lib.swt_decode_plan(*head, p["tok_off"], p["tok_flags"], n_tok, flags, p["text_off"], p["status"], p["info"])
    else:
        rc = lib.swt_decode_rows(*head, p["tok_bytes"], p["tok_off"], p["tok_flags"], n_tok, flags, p["text_off"], p["out_text"],
                                 b["out_text"].size if text_cap is None else text_cap)
    return rc, lib.swt_last_error().decode(), b


@pytest.mark.parametrize("form", ["plan", "rows"])
def test_host_forms_refuse_bad_arguments_without_a_device(native, form):
    INV = native.ERR_INVALID
    for name in NAMES_PLAN if form == "plan" else NAMES_ROWS:
        if name == "mask":
            continue
        rc, msg, _ = _call(native, form, **{name: False})
        assert rc == INV and name in msg, name
    for kw, word in (({"width": 0}, "width"), ({"rows": 1 << 32}, "rows"), ({"width": 1 << 31}, "width"), ({"flags": 2}, "flag"),
                     ({"flags": 8}, "flag"), ({"n_tok": 0}, "n_tok")):
        rc, msg, _ = _call(native, form, **kw)
        assert rc == INV and word in msg, (kw, msg)
    down = _bufs()["tok_off"].copy()
    down[3] = down[4] + 1
    rc, msg, _ = _call(native, form, tok_off=down)
    assert rc == INV and "tok_off" in msg
    large = _bufs()["tok_off"].copy()
    large[-1] = 1 << 23  # a step's bytes are summed in 32 bits: 256 columns of such a vocabulary may not fit
    rc, msg, _ = _call(native, form, tok_off=large)
    assert rc == INV and "tok_off" in msg
    large[-1] = (1 << 23) - 1
    rc, msg, _ = _call(native, form, tok_off=large, rows=0)
    assert rc == 0, msg


def test_plan_of_no_row_succeeds_without_a_device(native):
    off, info = np.full(1, 7, dtype=np.uint64), np.full(3, 9, dtype=np.uint64)
    rc, _, _ = _call(native, "plan", rows=0, text_off=off, info=info)
    assert rc == 0 and off.tolist() == [0] and info.tolist() == [0, 0, 0]
    rc, _, _ = _call(native, "plan", rows=0, width=0)
    assert rc == 0
    rc, _, _ = _call(native, "rows", rows=0, text_off=np.zeros(1, dtype=np.uint64))
    assert rc == 0
    assert native.decode_plan(np.zeros((0, 5), dtype=np.int64), None, *_bufs_tables())[0].tolist() == [0]


def _bufs_tables():
    b = _bufs()
    return b["tok_off"], b["tok_flags"], b["n_tok"]


def test_rows_refuse_a_foreign_plan_and_a_short_capacity_without_a_device(native):
    INV = native.ERR_INVALID
    good = _bufs()["text_off"]
    for k, delta in ((0, 1), (1, 1), (3, -1), (2, 5)):
        off = good.copy()
        off[k] = np.uint64(int(off[k]) + delta)
        rc, msg, _ = _call(native, "rows", text_off=off)
        assert rc == INV and "text_off" in msg, (k, delta)
    rc, msg, _ = _call(native, "rows", text_off=good[::-1].copy())
    assert rc == INV and "text_off" in msg
    # the plan of other flags is not the plan of these
    ids = np.array([[0, 4, 5, 3]] * 3, dtype=np.int32)  # [PAD] ab ##cd [SEP]
    tabs = D.tables(D.TOY, len(D.TOY))
    off_skip, off_all = D.decode(ids, None, tabs, flags=1)[1], D.decode(ids, None, tabs, flags=0)[1]
    rc, msg, _ = _call(native, "rows", ids=ids, text_off=off_all, flags=1, text_cap=1 << 20)
    assert rc == INV and "text_off" in msg
    rc, msg, _ = _call(native, "rows", ids=ids, text_off=off_skip, flags=1, text_cap=int(off_skip[-1]) - 1)
    assert rc == native.ERR_CAPACITY and "text_cap" in msg
    rc, msg, _ = _call(native, "rows", text_cap=int(good[-1]) - 1)
    assert rc == native.ERR_CAPACITY
    if native.device_count() == 0:  # everything in order: only now is a device looked for
        assert _call(native, "rows")[0] == native.ERR_NO_DEVICE
        assert _call(native, "plan")[0] == native.ERR_NO_DEVICE


def test_symbols_and_constants(native):
    lib = C.CDLL(native._build.LIB_PATH)
    for name in ("swt_decode_plan", "swt_decode_plan_dev", "swt_decode_rows", "swt_decode_rows_dev", "swt_decode_capacity"):
        assert hasattr(lib, name) and name in native.SIGNATURES
    assert native.decode_capacity() == (256, 1024)
    assert (native.DECODE_SKIP_SPECIAL, native.DECODE_IDS64) == (D.SKIP_SPECIAL, D.IDS64) == (1, 4)
    assert (native.TOK_GLUE, native.TOK_NO_SPACE_BEFORE, native.TOK_NO_SPACE_AFTER, native.TOK_SPECIAL, native.TOK_BAD) == \
        (D.GLUE, D.NO_SPACE_BEFORE, D.NO_SPACE_AFTER, D.SPECIAL, D.BAD) == (1, 2, 4, 8, 16)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "swt.h"), encoding="utf-8").read()
    for name, value in (("SWT_DECODE_SKIP_SPECIAL", 1), ("SWT_DECODE_IDS64", 4), ("SWT_TOK_GLUE", 1), ("SWT_TOK_NO_SPACE_BEFORE", 2),
                        ("SWT_TOK_NO_SPACE_AFTER", 4), ("SWT_TOK_SPECIAL", 8), ("SWT_TOK_BAD", 16)):
        assert re.search(r"#define %s %du\b" % (name, value), header), name


def test_decode_methods_refuse_bad_arguments(swt):
    """decided from the arguments alone, before a vocabulary or a device is looked for"""
    tok = swt.FastWP()
    for bad in (np.zeros((2, 3), dtype=np.int16), np.zeros(3, dtype=np.int32), np.zeros((2, 4), dtype=np.int64)[:, ::2], [[1, 2]], "ab"):
        with pytest.raises(TypeError):
            tok.decode_batch_bytes(bad)
    with pytest.raises(TypeError):
        tok.decode(np.zeros((2, 2), dtype=np.int32))
    with pytest.raises(TypeError):
        tok.decode([0.5])
    assert tok.decode([]) == ""
