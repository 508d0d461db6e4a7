"""The Python model of packed batches (tests/pack_cases.py) held, without a GPU, to tests/batch_cases.expected_batch -- which
tests/test_batch_cases.py pins to the `tokenizers` wheel -- and to the properties that make a packing one."""
import json
import os

import numpy as np
import pytest

from tests import batch_cases as B
from tests import pack_cases as K

HERE = os.path.dirname(os.path.abspath(__file__))
SPECIALS = [(None, None), (2, None), (None, 3), (2, 3)]
WIDTHS = (3, 4, 5, 8, 64, 129, 130)


def cases():
    rng = np.random.RandomState(11)
    n_map = 40
    table = (500 + rng.permutation(n_map)).astype(np.uint32)
    table[5] = B.NONE
    for width in WIDTHS:
        for k, (cls_id, sep_id) in enumerate(SPECIALS):
            if width - (cls_id is not None) - (sep_id is not None) < 1:
                continue
            for n, kind in ((0, 0), (1, 0), (37, 0), (60, 1), (25, 2)):
                lengths = K.random_lengths(n, width, width * 10 + k) if kind == 0 else \
                    [int(x) for x in rng.choice([0, 0, 0, 1, width], size=n)] if kind == 1 else [0] * n
                rows = B.stream(lengths, seed=width + k, id_lo=0, id_hi=n_map + 5)[0]
                s = B.spec(width, ids64=bool(k & 1), pad_id=90, unk_id=91, cls_id=cls_id, sep_id=sep_id)
                yield rows, s, (table, n_map, False)


def live(out, key):
    return out[key][out["attention_mask"] == 1]


@pytest.mark.parametrize("mode", [K.WHOLE, K.SPLIT, K.SPLIT | K.DROP_LAST])
def test_columns_are_those_of_the_padded_batch(mode):
    """the non-padding columns of all packed rows, read in order, are the non-padding columns of expected_batch read in order:
    WHOLE at the same width (the same truncation), SPLIT at a width no row reaches (none)"""
    for rows, s, cmap in cases():
        got = K.expected_pack(rows, s, mode, cmap)
        n_special = (s["cls_id"] is not None) + (s["sep_id"] is not None)
        wide = dict(s, width=max([len(r) for r in rows] + [1]) + n_special) if mode & K.SPLIT else s
        want = B.expected_batch(rows, wide, cmap)
        flat = live(want, "input_ids")
        if mode & K.DROP_LAST:
            assert got["rows"] == flat.size // s["width"]
            flat = flat[:got["rows"] * s["width"]]
        else:
            assert got["n_unknown"] == want["n_unknown"] and got["lost"] == want["lost"]
        assert live(got, "input_ids").tolist() == flat.tolist()
        assert got["input_ids"].dtype == want["input_ids"].dtype
        assert (got["input_ids"][got["attention_mask"] == 0] == s["pad_id"]).all()
        assert got["length"].tolist() == got["attention_mask"].sum(axis=1).tolist()
        assert got["longest"] == max([len(r) for r in rows] + [0])


def test_whole_is_next_fit():
    for rows, s, cmap in cases():
        width = s["width"]
        got = K.expected_pack(rows, s, K.WHOLE, cmap)
        seg, n = got["seg"], len(rows)
        assert K.next_fit_search(seg, width) == K.next_fit_loop(seg, width) == got["row_first"][:got["rows"]].tolist()
        assert got["rows"] == (0 if n == 0 else max(1, got["rows"])) and (n == 0 or got["rows"] >= 1)
        assert got["total"] == sum(seg) and max(seg + [0]) <= width
        first = got["row_first"].tolist()
        assert first[got["rows"]:] == [n] * (n + 1 - got["rows"])
        for b in range(got["rows"]):
            held = sum(seg[first[b]:first[b + 1]])
            assert first[b] < first[b + 1] and held <= width and held == int(got["length"][b])
            if b + 1 < got["rows"]:
                assert held + seg[first[b + 1]] > width, "the next row's first segment would have fitted"
        for r in range(n):  # no segment crosses a row
            at = int(got["slot"][r])
            assert seg[r] == 0 or at // width == (at + seg[r] - 1) // width
        assert int(got["slot"][n]) == (int(got["slot"][n - 1]) + seg[-1] if n else 0)


def test_split_is_concatenate_and_cut():
    for rows, s, cmap in cases():
        width, n = s["width"], len(rows)
        for mode in (K.SPLIT, K.SPLIT | K.DROP_LAST):
            got = K.expected_pack(rows, s, mode, cmap)
            total = sum(len(r) for r in rows) + n * ((s["cls_id"] is not None) + (s["sep_id"] is not None))
            assert got["total"] == total and got["lost"] == 0
            assert got["rows"] == (total // width if mode & K.DROP_LAST else -(-total // width))
            fill = got["length"].tolist()
            assert fill[:-1] == [width] * (len(fill) - 1)
            if fill:
                assert fill[-1] == (width if mode & K.DROP_LAST or total % width == 0 else total % width)
            assert got["slot"].tolist() == np.concatenate([[0], np.cumsum(got["seg"])]).tolist()


@pytest.mark.parametrize("mode", [K.WHOLE, K.SPLIT, K.SPLIT | K.DROP_LAST])
def test_plan_and_columns_are_consistent(mode):
    """slot, row_first, position_ids, sequence_ids and sample_ids say the same thing"""
    for rows, s, cmap in cases():
        width, n = s["width"], len(rows)
        got = K.expected_pack(rows, s, mode, cmap)
        mask = got["attention_mask"].reshape(-1)
        pos, seq, doc = (got[k].reshape(-1) for k in ("position_ids", "sequence_ids", "sample_ids"))
        assert (pos[mask == 0] == 0).all() and (seq[mask == 0] == K.NONE).all() and (doc[mask == 0] == K.NONE).all()
        x = np.flatnonzero(mask)
        r = doc[x].astype(np.int64)
        assert (np.diff(r) >= 0).all()
        # a column's flat position is its segment's slot and its position in the segment
        assert (got["slot"][r].astype(np.int64) + pos[x] == x).all()
        assert (pos[x] < np.array(got["seg"], dtype=np.int64)[r]).all()
        owners = got["row_first"].astype(np.int64)
        known = x // width <= n
        assert (seq[x][known] == r[known] - owners[x[known] // width]).all()
        for b in range(min(got["rows"], n + 1)):
            row_docs = doc[b * width:(b + 1) * width][mask[b * width:(b + 1) * width] == 1]
            if row_docs.size:  # column 0 belongs to the owner, or to the first row behind it that has a column at all
                assert int(row_docs[0]) >= int(owners[b]) and not any(got["seg"][int(owners[b]):int(row_docs[0])])
        # every column of every segment is there once, unless a last row was dropped
        if not mode & K.DROP_LAST:
            assert x.size == got["total"]
            assert np.bincount(r, minlength=n).tolist() == list(got["seg"]) if n else x.size == 0


def test_the_table_of_the_issue():
    """the row counts of pan_tadeusz's recorded token lists with [CLS] and [SEP]: next-fit and concatenate-and-cut"""
    with open(os.path.join(HERE, "golden", "ref", "data", "pan_tadeusz.tokens.json")) as f:
        tokens = json.load(f)
    want = {("FastBPE", 64): (227, 205), ("FastBPE", 512): (26, 26), ("FastWordPiece", 64): (664, 487),
            ("FastWordPiece", 128): (278, 244), ("FastWordPiece", 512): (63, 61)}
    for (name, width), (whole, split) in want.items():
        lengths = [len(t) for t in tokens[name]]
        assert len(lengths) == 989
        s = B.spec(width, cls_id=2, sep_id=3)
        assert K.expected_plan(lengths, s, K.WHOLE)["rows"] == whole
        assert K.expected_plan(lengths, s, K.SPLIT)["rows"] == split
