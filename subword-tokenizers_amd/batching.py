"""Model-ready batches: what stands between the tokenizer classes and swt_batch_plan / swt_batch_rows.

A tokenizer class gives its `Vocabulary` (`_batch_vocabulary`: specials and token strings in dense-id order, and the map from the
encoder's ids to dense ids) and its encode calls (`encode_ids_batch`, `_batch_encode_spans`, `_batch_encode_dev`); `encode_batch`
pads, truncates or windows the rows on the device -- through the host forms of the C ABI into NumPy arrays, or with
`device=True` on torch tensors without the ids ever leaving the device.  `mask_tokens` masks such rows for the masked-LM
objective (swt_mlm_mask), from `encode_batch(..., mlm={...})` or on rows that stay resident.  `decode_batch`
spells rows of dense ids back as text (swt_decode_plan / swt_decode_rows).  `align_word_labels`,
`answer_positions` and `best_answers` make the labels of token classification and extractive QA, and a QA model's best spans,
from the rows of a batch (swt_label_words, swt_answer_positions, swt_answer_best)."""
import collections
import ctypes as C
import re

import numpy as np

from . import _native as N

SPECIALS = ("[PAD]", "[UNK]", "[CLS]", "[SEP]")
MASK = "[MASK]"
# Code points every BPE vocabulary holds besides those of its merges: merges.json is all a BPE model saves (bpe.py:167-177), and a
# code point that never merged -- every punctuation mark: the pre-tokenizer isolates them -- is in no merge.  Basic Latin, Latin-1
# Supplement and Latin Extended-A without controls and spaces.
BPE_BASE_ALPHABET = [chr(c) for c in range(0x21, 0x180) if not 0x7F <= c <= 0xA0]


class Vocabulary:
    """tokens: strings in dense-id order; index: string -> dense id; cmap, n_map, flagged: the encoder's ids -> dense ids in the
    convention of swt_batch_rows; special: name -> dense id"""

    def __init__(self, tokens, index, cmap, n_map, flagged):
        self.tokens, self.index, self.cmap, self.n_map, self.flagged = tokens, index, cmap, n_map, flagged
        self.special = {name: index[s] for name, s in zip(("pad", "unk", "cls", "sep"), SPECIALS)}
        self.d_cmap = None  # the map as a torch tensor, made by the first device call
        self.mask_id = index.get(MASK, len(tokens))  # one past the end where the vocabulary has no "[MASK]": no dense id moves
        self._cls_tab = self._rand_ids = None
        self.d_mlm = None  # (device, cls_tab, rand_ids) as torch tensors, made by the first device call of mask_tokens
        self._decode = None
        self.d_decode = None  # (device, tok_bytes, tok_off, tok_flags) as torch tensors, made by the first device call of decode_batch
        # added tokens (with_added): the encoder-side id of the first, the dense id of each, the strings of the special and of
        # the ordinary ones
        self.added_base, self.added_dense, self.added_special, self.added_ordinary = None, (), frozenset(), frozenset()

    @property
    def cls_tab(self):
        """uint8 per dense id: 0 starts a word, 1 continues one ('##' and more), 2 is never masked (the specials, [MASK] and
        the special added tokens); an ordinary added token that was appended starts a word, one the vocabulary held keeps its class"""
        if self._cls_tab is None:
            never, word = set(SPECIALS) | {MASK} | self.added_special, self.added_ordinary
            self._cls_tab = np.fromiter((2 if t in never else 0 if t in word else 1 if len(t) > 2 and t.startswith("##") else 0
                                         for t in self.tokens), dtype=np.uint8, count=len(self.tokens))
        return self._cls_tab

    @property
    def rand_ids(self):
        """uint32, ascending: every dense id a random replacement may be (class 0 or 1)"""
        if self._rand_ids is None:
            self._rand_ids = np.flatnonzero(self.cls_tab < 2).astype(np.uint32)
        return self._rand_ids

    @property
    def decode_tables(self):
        """(tok_bytes uint8, tok_off uint32[n + 1], tok_flags uint8[n], n): the vocabulary of swt_decode_* (include/swt.h), with
        "[MASK]" appended where mask_id is one past the end"""
        if self._decode is None:
            tokens = list(self.tokens) + ([MASK] if self.mask_id == len(self.tokens) else [])
            raw = [t.encode("utf-8") for t in tokens]
            off = np.zeros(len(raw) + 1, dtype=np.uint32)
            total = sum(map(len, raw))
            if total >= 1 << 23:
                raise ValueError("decode: the vocabulary's tokens take %d bytes, swt_decode_* takes fewer than 2^23" % total)
            off[1:] = np.cumsum([len(b) for b in raw], dtype=np.uint64)
            special = self.added_special
            flags = np.fromiter((_decode_flags(t) | (N.TOK_SPECIAL if t in special else 0) for t in tokens), dtype=np.uint8,
                                count=len(tokens))
            self._decode = (np.frombuffer(b"".join(raw) + b"\0", dtype=np.uint8), off, flags, len(tokens))
        return self._decode


_NO_SPACE_BEFORE, _NO_SPACE_AFTER = frozenset(".,)]\\’-'/"), frozenset("([\\’-'/")  # utils.py:150, 152
_DECODE_SKIPPED = frozenset(("[PAD]", "[CLS]", "[SEP]", MASK))  # [UNK] stands for a word of the text: it is spelled
_PY_SPACE = re.compile(r"\s")


def _decode_flags(tok):
    """the tok_flags byte of a token string (include/swt.h)"""
    f = N.TOK_SPECIAL if tok in _DECODE_SKIPPED else 0
    if not tok or _PY_SPACE.search(tok):
        return f | N.TOK_BAD  # the reference's regular expressions would act inside it: not spelled by the join rule
    if len(tok) >= 3 and tok.startswith("##"):
        f |= N.TOK_GLUE
    if tok[0] in _NO_SPACE_BEFORE:
        f |= N.TOK_NO_SPACE_BEFORE
    if tok[-1] in _NO_SPACE_AFTER:
        f |= N.TOK_NO_SPACE_AFTER
    return f


def bpe_vocabulary(merges, syms):
    """The four specials, the symbol strings sorted, the same strings with '##'.  The strings are those of merges.json -- both
    sides and the result of every merge, and their code points -- and BPE_BASE_ALPHABET: nothing that save_resources does not
    keep.  Any other code point has no dense id and becomes [UNK]."""
    strings = set(BPE_BASE_ALPHABET)
    for left, right in merges:
        strings.update((left, right, left + right))
    strings.update(c for s in list(strings) for c in s)
    strings.discard("")
    strings = sorted(strings)
    n = len(strings)
    tokens = list(SPECIALS) + strings + ["##" + s for s in strings]
    index = {}
    for i, tok in enumerate(tokens):
        index.setdefault(tok, i)
    n_map = N.SYM_BASE + len(syms.strings)
    cmap = np.full(2 * n_map, N.BATCH_NONE, dtype=np.uint32)
    for i, s in enumerate(strings):
        sid = ord(s) if len(s) == 1 else syms.index.get(s)
        if sid is None:
            continue  # a string no id of this table spells
        if len(s) > 1:
            sid += N.SYM_BASE
        cmap[sid] = len(SPECIALS) + i
        cmap[n_map + sid] = len(SPECIALS) + n + i
    return Vocabulary(tokens, index, cmap, n_map, True)


def wp_vocabulary(sorted_tokens):
    """The vocabulary in the encoder's own order (ids index sorted(vocab): vocab.json is a set's order, wordpiece.py:196), so the
    map is the identity on it; a special takes its index where the vocabulary has the string and is appended where not.  Both
    unknown ids (n_vocab "['UNK']", n_vocab + 1 "[UNK]") go to [UNK]; the marker of a multi-token '##' corner has no dense id."""
    tokens = list(sorted_tokens)
    index = {tok: i for i, tok in enumerate(tokens)}
    for s in SPECIALS:
        if s not in index:
            index[s] = len(tokens)
            tokens.append(s)
    index.setdefault("['UNK']", index["[UNK]"])
    n = len(sorted_tokens)
    cmap = np.concatenate([np.arange(n, dtype=np.uint32), np.array([index["[UNK]"], index["[UNK]"], N.BATCH_NONE], dtype=np.uint32)])
    return Vocabulary(tokens, index, cmap, n + 3, False)


def with_added(voc, added):
    """`voc` (of bpe_vocabulary / wp_vocabulary) with the added tokens `added`, a list of (content, special), behind it: a new
    Vocabulary in which no dense id of `voc` has moved.  The string of an added token -- content for a special one,
    content.lower() for an ordinary one -- takes its index where `voc` holds the string, mask_id where it is "[MASK]", and else
    the next free id from max(len(voc.tokens), voc.mask_id + 1) on, in the order of addition; once an id is handed out, the
    token list runs to the highest id, with "[MASK]" at its reserved slot.  The encoder-side id of added token k is added_base
    + k, past every id of the encoder, and the map grows by those entries in the convention it has (flagged or plain)."""
    if not added:
        return voc
    tokens, index = list(voc.tokens), dict(voc.index)
    dense, special, ordinary = [], set(), set()
    for content, is_special in added:
        s = content if is_special else content.lower()
        if is_special:
            special.add(s)
        elif s not in voc.index:  # an ordinary token the vocabulary holds keeps the class it has there ('##x' goes on continuing)
            ordinary.add(s)
        if s in index:
            d = index[s]
        elif s == MASK:
            d = voc.mask_id
        else:
            if len(tokens) == voc.mask_id:  # the reserved slot is spelled before anything goes behind it
                index[MASK] = len(tokens)
                tokens.append(MASK)
            d = index[s] = len(tokens)
            tokens.append(s)
        dense.append(d)
    dense = np.array(dense, dtype=np.uint32)
    if voc.flagged:  # [plain | flagged], each n_map long; n_map itself is the encoder's id of a symbol it cannot spell
        base = voc.n_map + 1
        n_map = base + len(dense)
        cmap = np.full(2 * n_map, N.BATCH_NONE, dtype=np.uint32)
        cmap[:voc.n_map], cmap[n_map:n_map + voc.n_map] = voc.cmap[:voc.n_map], voc.cmap[voc.n_map:]
        cmap[base:n_map] = dense
    else:
        base, n_map = voc.n_map, voc.n_map + len(dense)
        cmap = np.concatenate([voc.cmap, dense])
    out = Vocabulary(tokens, index, cmap, n_map, voc.flagged)
    assert out.mask_id == voc.mask_id and out.special == voc.special
    out.added_base, out.added_dense, out.added_special, out.added_ordinary = base, dense, frozenset(special), frozenset(ordinary - special)
    return out


def check_added_token(token, n_so_far):
    """the ValueError of add_tokens for a token that cannot be added (include/swt.h states the limits), naming it"""
    if not isinstance(token, str):
        raise TypeError("an added token is a string")
    if token == "":
        raise ValueError("added token %r: the empty string" % token)
    if any(N.class_of(ord(ch)) & N.CLS_BERT_WS or ch.isspace() for ch in token + token.lower()):
        raise ValueError("added token %r: whitespace inside" % token)
    if any(ord(ch) > 0xFFFF or ord(ch) == 0 or 0xD800 <= ord(ch) < 0xE000 for ch in token + token.lower()):
        raise ValueError("added token %r: a code point past U+FFFF, a surrogate or U+0000" % token)
    if len(token.lower().encode("utf-8")) > 64:
        raise ValueError("added token %r: its pattern takes more than 64 bytes" % token)
    if n_so_far >= 4096:
        raise ValueError("added token %r: more than 4096 added tokens" % token)


def _width(longest, n_special, max_length, padding, multiple):
    if padding not in ("longest", "max_length"):
        raise ValueError("padding is 'longest' or 'max_length'")
    if padding == "max_length":
        if max_length is None:
            raise ValueError("padding='max_length' needs a max_length")
        width = int(max_length)
    else:
        width = max(longest, 1) + n_special
        if max_length is not None:
            width = min(width, int(max_length))
    if multiple:
        width = -(-width // int(multiple)) * int(multiple)
    return width


def _spec(tok, voc, width, stride, windows, add_special_tokens, padding_side, int64):
    if padding_side not in ("right", "left"):
        raise ValueError("padding_side is 'right' or 'left'")
    sp = voc.special
    return N.batch_spec(width, stride, windows, padding_side == "left", int64, sp["pad"], sp["unk"],
                        sp["cls"] if add_special_tokens else None, sp["sep"] if add_special_tokens else None)


def _check(texts, max_length, stride, return_overflowing):
    if not isinstance(texts, list) or not all(isinstance(t, str) for t in texts):
        raise TypeError("Text to tokenize must be a string.")
    if return_overflowing and max_length is None:
        raise ValueError("return_overflowing needs a max_length")
    if stride < 0:
        raise ValueError("stride must not be negative")


STRATEGIES = {"longest_first": N.PAIR_LONGEST_FIRST, "only_first": N.PAIR_ONLY_FIRST, "only_second": N.PAIR_ONLY_SECOND}


def _check_pairs(texts, text_pairs, truncation, return_overflowing, return_token_type_ids, return_special_tokens_mask):
    if truncation not in STRATEGIES:
        raise ValueError("truncation is 'longest_first', 'only_first' or 'only_second'")
    if text_pairs is None:
        if truncation != "longest_first" or return_token_type_ids or return_special_tokens_mask:
            raise ValueError("truncation strategies, token types and the special-tokens mask need text_pairs")
        return
    if not isinstance(text_pairs, list) or not all(isinstance(t, str) for t in text_pairs):
        raise TypeError("Text to tokenize must be a string.")
    if len(text_pairs) != len(texts):
        raise ValueError("text_pairs holds one text for every text")
    if return_overflowing and truncation == "longest_first":
        raise ValueError("return_overflowing with pairs needs truncation='only_first' or 'only_second'")


def _raise_refused(status, off_a, off_b, cap, stride, windows, truncation):
    """the ValueError for the first refused pair; off_a, off_b: the offsets of both sides as NumPy arrays"""
    r = int(np.flatnonzero(status)[0])
    na, nb = int(off_a[r + 1] - off_a[r]), int(off_b[r + 1] - off_b[r])
    budget = cap - (nb if truncation == "only_first" else na)
    why = "no token" if budget < 1 else "%d tokens, not more than the stride %d" % (budget, stride) if windows else "%d tokens" % budget
    raise ValueError("pair %d (%d and %d tokens) cannot be truncated with %r: %d tokens fit a row and the other side leaves %s"
                     % (r, na, nb, truncation, cap, why))


def _pair_result(out, overflowing, offsets, token_types, special_mask):
    res = _result(out, overflowing, offsets, int(out["info"][2]))
    res["sequence_ids"] = out["sequence_ids"]
    if token_types:
        res["token_type_ids"] = out["token_type_ids"]
    if special_mask:
        res["special_tokens_mask"] = out["special_tokens_mask"]
    return res


def _encode_host(tok, texts, offsets, dropout=None):
    """one encode through the host forms -> (ids, tok_off, spans, word); spans and word are None without offsets"""
    if tok._added:
        return _encode_host_added(tok, texts, offsets, dropout)
    if offsets:
        got = tok._batch_encode_spans(texts) if dropout is None else tok._batch_encode_spans(texts, dropout)
        return got[0], got[1], got[-2], got[-1]
    got = tok._batch_encode_ids(texts, dropout)
    return got[0], got[1], None, None


def _encode_host_added(tok, texts, offsets, dropout=None):
    """_encode_host of a tokenizer with added tokens: the texts are packed and lowercased once, the added tokens found and
    blanked (swt_added_find), the blanked text encoded by the class's span call -- the spans are needed whether or not the caller
    wants offsets -- and the matches spliced into its streams (swt_added_splice)"""
    patterns, voc = tok._added_patterns(), tok._batch_vocabulary()
    text, off = N.pack_and_lower(texts)
    blank, m_off, m_pat, m_span, _ = patterns.find(text, off)
    got = tok._batch_encode_spans_packed(blank, off, texts, dropout)
    ids, tok_off, spans, word = N.added_splice(got[0], got[1], got[-2], got[-1], m_off, m_pat, m_span, voc.added_base)
    return (ids, tok_off, spans, word) if offsets else (ids, tok_off, None, None)


def _encode_pairs(tok, voc, texts, text_pairs, max_length, stride, padding, multiple, add_special_tokens, padding_side, overflowing, offsets,
                  int64, truncation, token_types, special_mask, dropout=None):
    """pairs through the host forms: ONE encode of texts + text_pairs, whose offsets from len(texts) on are those of the B sides"""
    n, strategy, n_special = len(texts), STRATEGIES[truncation], 3 if add_special_tokens else 0
    ids, tok_off, spans, word = _encode_host(tok, texts + text_pairs, offsets, dropout)
    tok_off = np.ascontiguousarray(tok_off, dtype=np.uint64)
    off_a, off_b = tok_off[:n + 1], tok_off[n:]
    longest = int(N.batch_pair_plan(off_a, off_b, N.batch_spec(0), strategy)[2][1])
    width = _width(longest, n_special, max_length, padding, multiple)
    spec = _spec(tok, voc, width, stride, overflowing, add_special_tokens, padding_side, int64)
    row_base, status, info = N.batch_pair_plan(off_a, off_b, spec, strategy)
    if info[3]:
        _raise_refused(status, off_a, off_b, width - n_special, stride, overflowing, truncation)
    out = N.batch_pair_rows(ids, off_a, off_b, spec, strategy, voc.cmap, voc.n_map, voc.flagged, spans, word, row_base, status)
    return _pair_result(out, overflowing, offsets, token_types, special_mask)


def encode_batch(tok, texts, max_length=None, stride=0, padding="longest", pad_to_multiple_of=None, add_special_tokens=True,
                 padding_side="right", return_overflowing=False, return_offsets=False, int64=False, device=False, text_pairs=None,
                 truncation="longest_first", return_token_type_ids=None, return_special_tokens_mask=False, packing=None, drop_last=False,
                 mlm=None, dropout=None):
    if dropout is not None:
        tok._enc.draw(dropout)  # refused before anything is encoded: a class without that dropout, arguments that give no draw
    if mlm is None:
        return _encode_batch(tok, texts, max_length, stride, padding, pad_to_multiple_of, add_special_tokens, padding_side,
                             return_overflowing, return_offsets, int64, device, text_pairs, truncation, return_token_type_ids,
                             return_special_tokens_mask, packing, drop_last, dropout)
    if not isinstance(mlm, dict):
        raise TypeError("mlm is None or a dict of mask_tokens keywords")
    _mlm_thresholds(**{k: v for k, v in mlm.items() if k != "return_selected"})  # refused before anything is encoded
    res = _encode_batch(tok, texts, max_length, stride, padding, pad_to_multiple_of, add_special_tokens, padding_side, return_overflowing,
                        return_offsets, int64, device, text_pairs, truncation, return_token_type_ids, return_special_tokens_mask, packing,
                        drop_last, dropout)
    res.update(mask_tokens(tok, res["input_ids"], **mlm))
    return res


def _encode_batch(tok, texts, max_length, stride, padding, pad_to_multiple_of, add_special_tokens, padding_side, return_overflowing,
                  return_offsets, int64, device, text_pairs, truncation, return_token_type_ids, return_special_tokens_mask, packing, drop_last,
                  dropout=None):
    _check(texts, max_length, stride, return_overflowing)
    _check_pairs(texts, text_pairs, truncation, return_overflowing, return_token_type_ids, return_special_tokens_mask)
    voc = tok._batch_vocabulary()
    if packing is not None or drop_last:
        mode = _pack_mode(packing, drop_last, max_length, stride, padding_side, return_overflowing, return_offsets, text_pairs)
        width = _width(0, 0, max_length, "max_length", pad_to_multiple_of)
        spec = _spec(tok, voc, width, 0, False, add_special_tokens, "right", int64)
        return (_pack_device if device else _pack_host)(tok, voc, texts, spec, mode, dropout)
    geometry = (max_length, stride, padding, pad_to_multiple_of, add_special_tokens, padding_side, return_overflowing, return_offsets, int64)
    if text_pairs is not None:
        token_types, special_mask = return_token_type_ids is None or bool(return_token_type_ids), bool(return_special_tokens_mask)
        if not device:
            return _encode_pairs(tok, voc, texts, text_pairs, *geometry, truncation, token_types, special_mask, dropout)
        out = _encode_device(tok, voc, texts + text_pairs, len(texts), *geometry, (truncation, token_types, special_mask), dropout)
        return _pair_result(out, return_overflowing, return_offsets, token_types, special_mask)
    if device:
        out = _encode_device(tok, voc, texts, len(texts), *geometry, None, dropout)
        return _result(out, return_overflowing, return_offsets, int(out["info"][2]))
    ids, tok_off, spans, word = _encode_host(tok, texts, return_offsets, dropout)
    _, longest = N.batch_plan(tok_off, N.batch_spec(0))
    width = _width(longest, 2 if add_special_tokens else 0, max_length, padding, pad_to_multiple_of)
    spec = _spec(tok, voc, width, stride, return_overflowing, add_special_tokens, padding_side, int64)
    row_base = N.batch_plan(tok_off, spec)[0] if return_overflowing else None
    out = N.batch_rows(ids, tok_off, spec, voc.cmap, voc.n_map, voc.flagged, spans, word, row_base)
    return _result(out, return_overflowing, return_offsets, int(out["info"][2]))


PACKINGS = {"whole": N.PACK_WHOLE, "split": N.PACK_SPLIT}


def _pack_mode(packing, drop_last, max_length, stride, padding_side, overflowing, offsets, text_pairs):
    """the PACK_* mode of a call, or the ValueError for what does not go with packing"""
    if drop_last and packing != "split":
        raise ValueError("drop_last needs packing='split'")
    if packing not in PACKINGS:
        raise ValueError("packing is None, 'whole' or 'split'")
    if max_length is None:
        raise ValueError("packing needs a max_length: the width of a packed row")
    if padding_side != "right":
        raise ValueError("padding_side is 'right' or 'left'" if padding_side != "left" else "packed rows are padded on the right")
    for given, name in ((text_pairs is not None, "text_pairs"), (overflowing, "return_overflowing"), (stride, "stride"),
                        (offsets, "return_offsets")):
        if given:
            raise ValueError("%s does not go with packing" % name)
    return PACKINGS[packing] | (N.PACK_DROP_LAST if drop_last else 0)


def _pack_result(out, slot, tok_off, spec, mode, info, plan_info, xp):
    """the arrays of a pack call and its plan as encode_batch returns them.  xp: numpy or torch, whichever holds the arrays"""
    n_rows, width = int(slot.shape[0]) - 1, int(spec.width)
    rows = int(out["input_ids"].shape[0])
    n_special = (spec.cls_id != N.BATCH_NONE) + (spec.sep_id != N.BATCH_NONE)
    tokens = tok_off[1:] - tok_off[:-1]
    if mode & N.PACK_WHOLE:
        tokens = xp.clip(tokens, 0, width - n_special) if xp is np else tokens.clamp(max=width - n_special)
    return {"input_ids": out["input_ids"], "attention_mask": out["attention_mask"], "position_ids": out["position_ids"],
            "sequence_ids": out["sequence_ids"], "sample_ids": out["sample_ids"], "length": out["length"],
            "n_unknown": int(info[2]), "n_truncated": int(info[1]),
            "segment_row": slot[:n_rows] // width, "segment_col": slot[:n_rows] % width, "segment_length": tokens + n_special,
            "density": float(min(int(plan_info[3]), rows * width)) / (rows * width) if rows else 0.0}


def _pack_host(tok, voc, texts, spec, mode, dropout=None):
    ids, tok_off = _encode_host(tok, texts, False, dropout)[:2]
    tok_off = np.ascontiguousarray(tok_off, dtype=np.uint64)
    slot, row_first, plan_info = N.pack_plan(tok_off, spec, mode)
    out = N.pack_rows(ids, tok_off, spec, mode, slot, row_first, voc.cmap, voc.n_map, voc.flagged, rows_cap=int(plan_info[0]))
    return _pack_result(out, slot.astype(np.int64), tok_off.astype(np.int64), spec, mode, out["info"], plan_info, np)


Encoded = collections.namedtuple("Encoded", "stream empty ids tok_off spans word checks")


def _encode_on_device(tok, voc, texts, offsets=False, dropout=None):
    """The front half of the device paths, on the current device and stream: ONE upload of the lowercased texts and one `_dev`
    encode (with offsets its span form) into torch-owned buffers, and voc.d_cmap on that device.  -> Encoded: empty(shape, dtype,
    wanted=True) allocates on the device; spans and word are None without offsets; checks: the (statuses, complain) pairs of the
    span form, for the caller to read"""
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = torch.cuda.current_stream().cuda_stream

    def empty(shape, dtype, wanted=True):
        return torch.empty(shape, dtype=dtype, device=dev) if wanted else None

    text, off = N.pack_utf8([t.lower() for t in texts])
    n_bytes, n_sent = int(text.size), len(texts)
    added = tok._added_patterns() if tok._added else None  # with added tokens the span form runs whether or not offsets are wanted
    spans = offsets or added is not None
    d_ids, d_tok_off = empty(n_bytes + 64, torch.int32), empty(n_sent + 1, torch.int64)
    d_spans, d_word = empty(2 * (n_bytes + 64), torch.int32, spans), empty(n_bytes + 64, torch.int32, spans)
    checks = []
    if n_bytes == 0:
        d_tok_off.zero_()  # nothing but empty texts: every row is specials and padding
    else:
        d_text = torch.from_numpy(np.concatenate([text, np.zeros(64, dtype=np.uint8)])).to(dev)
        d_off = torch.from_numpy(off.view(np.int64)).to(dev)
        d_ntok = torch.zeros(1, dtype=torch.int64, device=dev)
        if added is not None:  # the added tokens found and blanked in a copy of the text, which the encoder then reads
            d_seen = empty(n_bytes + 64, torch.uint8)
            d_seen[n_bytes:].zero_()
            d_m_off, d_m_pat, d_m_span = empty(n_sent + 1, torch.int64), empty(n_bytes, torch.int32), empty(2 * n_bytes, torch.int32)
            d_m_info = empty(4, torch.int64)
            added.find_dev(d_text.data_ptr(), n_bytes, d_off.data_ptr(), n_sent, d_seen.data_ptr(), d_m_off.data_ptr(), d_m_pat.data_ptr(),
                           d_m_span.data_ptr(), d_m_info.data_ptr(), stream)
            d_text = d_seen
        checks = tok._batch_encode_dev(d_text.data_ptr(), n_bytes, d_off.data_ptr(), n_sent, d_ids.data_ptr(), d_tok_off.data_ptr(),
                                       d_ntok.data_ptr(), d_spans.data_ptr() if spans else None, d_word.data_ptr() if spans else None,
                                       stream, empty, **({} if dropout is None else {"dropout": dropout}))
        if added is not None:  # and spliced into the encoder's streams: a text has no more tokens and matches than bytes
            before = d_ids, d_tok_off, d_spans, d_word
            d_ids, d_tok_off = empty(n_bytes + 64, torch.int32), empty(n_sent + 1, torch.int64)
            d_spans, d_word = empty(2 * (n_bytes + 64), torch.int32), empty(n_bytes + 64, torch.int32)
            N.check(N.lib().swt_added_splice_dev(*(a.data_ptr() for a in before), n_sent, d_m_off.data_ptr(), d_m_pat.data_ptr(),
                                                 d_m_span.data_ptr(), voc.added_base, d_ids.data_ptr(), d_tok_off.data_ptr(),
                                                 d_spans.data_ptr(), d_word.data_ptr(), stream))
    if voc.d_cmap is None or voc.d_cmap.device != dev:
        voc.d_cmap = torch.from_numpy(voc.cmap.view(np.int32)).to(dev)
    return Encoded(stream, empty, d_ids, d_tok_off, d_spans if offsets else None, d_word if offsets else None, checks)


def _pack_device(tok, voc, texts, spec, mode, dropout=None):
    """as _encode_device: one upload of the texts, one `_dev` encode, the packing plan and rows on torch-owned buffers on the
    current stream; the plan's info (for the rows to allocate) and the rows' info are all that comes back"""
    import torch
    n_rows, width = len(texts), int(spec.width)
    lib, check = N.lib(), N.check
    idt = torch.int64 if spec.flags & N.BATCH_IDS64 else torch.int32
    enc = _encode_on_device(tok, voc, texts, False, dropout)
    stream, empty, d_ids, d_tok_off = enc.stream, enc.empty, enc.ids, enc.tok_off
    d_slot, d_first, d_info = empty(n_rows + 1, torch.int64), empty(n_rows + 1, torch.int64), empty(8, torch.int64)
    check(lib.swt_pack_plan_dev(d_tok_off.data_ptr(), n_rows, C.byref(spec), mode, d_slot.data_ptr(), d_first.data_ptr(), d_info.data_ptr(),
                                stream))
    plan_info = d_info[:4].cpu().numpy()
    rows = int(plan_info[0])
    out = {"input_ids": empty((rows, width), idt), "attention_mask": empty((rows, width), torch.uint8),
           "position_ids": empty((rows, width), torch.int32), "sequence_ids": empty((rows, width), torch.int32),
           "sample_ids": empty((rows, width), torch.int32), "length": empty(rows, torch.int32)}
    info = np.zeros(3, dtype=np.int64)
    if rows:
        check(lib.swt_pack_rows_dev(d_ids.data_ptr(), d_tok_off.data_ptr(), n_rows, voc.d_cmap.data_ptr(), voc.n_map, int(voc.flagged),
                                    C.byref(spec), mode, d_slot.data_ptr(), d_first.data_ptr(), rows, out["input_ids"].data_ptr(),
                                    out["attention_mask"].data_ptr(), out["position_ids"].data_ptr(), out["sequence_ids"].data_ptr(),
                                    out["sample_ids"].data_ptr(), out["length"].data_ptr(), d_info.data_ptr(), stream))
        info = d_info[:3].cpu().numpy()
    return _pack_result(out, d_slot, d_tok_off, spec, mode, info, plan_info, torch)


def _result(out, overflowing, offsets, n_unknown):
    res = {"input_ids": out["input_ids"], "attention_mask": out["attention_mask"], "length": out["length"], "n_unknown": n_unknown}
    if overflowing:
        res["overflow_to_sample_mapping"] = out["sample"]
    if offsets:
        res["offset_mapping"], res["word_ids"] = out["offset_mapping"], out["word_ids"]
    return res


def _encode_device(tok, voc, texts, n_rows, max_length, stride, padding, multiple, add_special_tokens, padding_side, overflowing, offsets,
                   int64, pair=None, dropout=None):
    """The same on torch tensors, on the current device and stream: ONE upload of the lowercased texts, one `_dev` encode (or its
    span form), the plan and the rows call on torch-owned buffers; `info`, the token count and, of a batch that holds a refused
    pair, the statuses are all that comes back.  texts: every text of the call -- of pairs the A sides and then the B sides,
    n_rows of each, so that the B sides' offsets start where the A sides' end.  pair: None for single rows (swt_batch_plan_dev,
    swt_batch_rows_dev), else (truncation, token_types, special_mask) (swt_batch_pair_plan_dev, swt_batch_pair_rows_dev).
    -> the arrays of _native.batch_rows / batch_pair_rows as tensors, an output nobody asked for None, and "info"."""
    import torch
    truncation, token_types, special_mask = pair or (None, False, False)
    n_special, n_info = ((3 if pair else 2) if add_special_tokens else 0), (5 if pair else 3)
    lib, check = N.lib(), N.check
    idt = torch.int64 if int64 else torch.int32
    stream, empty, d_ids, d_tok_off, d_spans, d_word, checks = _encode_on_device(tok, voc, texts, offsets, dropout)
    p_spans, p_word = (d_spans.data_ptr(), d_word.data_ptr()) if offsets else (None, None)

    def outputs(rows, width):
        out = {"input_ids": empty((rows, width), idt), "attention_mask": empty((rows, width), torch.uint8),
               "length": empty(rows, torch.int32), "sample": empty(rows, torch.int32),
               "offset_mapping": empty((rows, width, 2), torch.int32, offsets), "word_ids": empty((rows, width), torch.int32, offsets)}
        if pair:
            out.update({"token_type_ids": empty((rows, width), idt, token_types),
                        "special_tokens_mask": empty((rows, width), torch.uint8, special_mask),
                        "sequence_ids": empty((rows, width), torch.int8)})
        return out

    if n_rows == 0:
        return dict(outputs(0, 0), info=[0] * n_info)
    if offsets:  # as the host span calls, which raise; the ids alone come back with an empty row for such a text
        for d_flags, complain in checks:
            status = d_flags[:len(texts)].cpu().numpy()
            bad = np.flatnonzero(status)
            if bad.size:
                complain(int(status[int(bad[0])]), int(bad[0]), texts[int(bad[0])])
    d_row_base, d_info = empty(n_rows + 1, torch.int64), empty(8, torch.int64)
    p_off = (d_tok_off.data_ptr(),)
    if pair:
        p_off += (d_tok_off.data_ptr() + 8 * n_rows,)
        strategy, d_status = STRATEGIES[truncation], empty(n_rows + 8, torch.uint8)

    def plan(spec):
        if pair:
            check(lib.swt_batch_pair_plan_dev(*p_off, n_rows, C.byref(spec), strategy, d_row_base.data_ptr(), d_status.data_ptr(),
                                              d_info.data_ptr(), stream))
        else:
            check(lib.swt_batch_plan_dev(*p_off, n_rows, C.byref(spec), d_row_base.data_ptr(), d_info.data_ptr(), stream))
        return d_info[:n_info].cpu().numpy()

    width = _width(int(plan(N.batch_spec(0))[1]), n_special, max_length, padding, multiple)
    spec = _spec(tok, voc, width, stride, overflowing, add_special_tokens, padding_side, int64)
    rows = n_rows
    if pair or overflowing:  # a pair's plan also says whether one is refused
        info = plan(spec)
        if pair and info[3]:
            h_off = d_tok_off.cpu().numpy()
            _raise_refused(d_status[:n_rows].cpu().numpy(), h_off[:n_rows + 1], h_off[n_rows:], width - n_special, stride, overflowing, truncation)
        rows = int(info[0])
    out = outputs(rows, width)
    p = {k: (v.data_ptr() if v is not None else None) for k, v in out.items()}
    head = (d_ids.data_ptr(), *p_off, n_rows, voc.d_cmap.data_ptr(), voc.n_map, int(voc.flagged), p_spans, p_word, C.byref(spec))
    tail = (p["offset_mapping"], p["word_ids"], p["sample"], p["length"], d_info.data_ptr(), stream)
    if pair:
        check(lib.swt_batch_pair_rows_dev(*head, strategy, d_row_base.data_ptr(), d_status.data_ptr(), rows, p["input_ids"], p["attention_mask"],
                                          p["token_type_ids"], p["special_tokens_mask"], p["sequence_ids"], *tail))
    else:
        check(lib.swt_batch_rows_dev(*head, d_row_base.data_ptr() if overflowing else None, rows, p["input_ids"], p["attention_mask"], *tail))
    out["info"] = d_info[:n_info].cpu().numpy()
    return out


class MaxMatch:
    """A `maxmatch_dropout` argument on its way through the calls below: they carry one `dropout` value from the public call to the
    encoder record (tokenizers._Encoder.draw), a dict for BPE-dropout as it was given, or this around the dict of MaxMatch-Dropout."""
    __slots__ = ("spec",)

    def __init__(self, spec):
        self.spec = spec


def dropout_draw(dropout, name="dropout"):
    """A `dropout` (or, by `name`, `maxmatch_dropout`) argument of the encode calls -> None, or (drop_below, seed, epoch) of
    swt_bpe_encode_dropout / swt_wp_encode_naive_dropout: drop_below = round(probability * 2^32), seed and epoch 0 unless given.
    TypeError for what is neither None nor a dict, ValueError for a probability that is missing, a NaN or outside [0, 1], an
    unknown key, a seed outside [0, 2^64) or an epoch outside [0, 2^32)."""
    if dropout is None:
        return None
    if not isinstance(dropout, dict):
        raise TypeError(name + " is None or a dict of 'probability', 'seed' and 'epoch'")
    unknown = set(dropout) - {"probability", "seed", "epoch"}
    if unknown or "probability" not in dropout:
        raise ValueError(name + " takes 'probability' and, if wanted, 'seed' and 'epoch'")
    p, seed, epoch = float(dropout["probability"]), int(dropout.get("seed", 0)), int(dropout.get("epoch", 0))
    if not 0.0 <= p <= 1.0:  # (false for a NaN)
        raise ValueError(name + ": probability lies in [0, 1]")
    if not 0 <= seed < 1 << 64:
        raise ValueError(name + ": seed lies in [0, 2^64)")
    if not 0 <= epoch < 1 << 32:
        raise ValueError(name + ": epoch lies in [0, 2^32)")
    return int(round(p * 4294967296.0)), seed, epoch


MLM_COUNTS = ("n_eligible", "n_selected", "n_masked", "n_random", "n_kept")


def _mlm_thresholds(probability=0.15, whole_word=True, seed=0, epoch=0, mask_share=0.8, random_share=0.1):
    """-> (select_below, mask_below, random_below): the integer thresholds of swt_mlm_spec, or the ValueError for arguments that
    give none.  The device compares 32-bit draws with them and knows no floating point."""
    for name, x in (("probability", probability), ("mask_share", mask_share), ("random_share", random_share)):
        if not 0.0 <= float(x) <= 1.0:
            raise ValueError("%s lies in [0, 1]" % name)
    if float(mask_share) + float(random_share) > 1.0 + 1e-12:  # the floors of the two thresholds still add up to 2^32 at most
        raise ValueError("mask_share + random_share must not exceed 1")
    if not 0 <= int(seed) < 1 << 64:
        raise ValueError("seed lies in [0, 2^64)")
    if not 0 <= int(epoch) < 1 << 32:
        raise ValueError("epoch lies in [0, 2^32)")
    mask_below = int(float(mask_share) * 4294967296.0)
    return int(float(probability) * 4294967296.0), mask_below, mask_below + int(float(random_share) * 4294967296.0)


def mask_tokens(tok, input_ids, probability=0.15, whole_word=True, seed=0, epoch=0, mask_share=0.8, random_share=0.1, return_selected=False):
    """SubwordTokenizer.mask_tokens: a NumPy array through swt_mlm_mask, a torch tensor on the GPU through swt_mlm_mask_dev on the
    current device and stream, with `info` the only read-back."""
    select_below, mask_below, random_below = _mlm_thresholds(probability, whole_word, seed, epoch, mask_share, random_share)
    voc = tok._batch_vocabulary()
    if isinstance(input_ids, np.ndarray):
        if input_ids.dtype not in (np.int32, np.int64) or input_ids.ndim != 2 or not input_ids.flags.c_contiguous:
            raise TypeError("input_ids: a 2-D C-contiguous array of int32 or int64")
        spec = N.mlm_spec(voc.cls_tab.size, voc.mask_id, select_below, mask_below, random_below, seed, epoch, whole_word,
                          input_ids.dtype == np.int64)
        out = N.mlm_mask(input_ids, voc.cls_tab, voc.rand_ids, spec, selected=return_selected)
        info = out["info"]
    else:
        import torch
        if not isinstance(input_ids, torch.Tensor) or not input_ids.is_cuda or input_ids.dtype not in (torch.int32, torch.int64) \
                or input_ids.dim() != 2 or not input_ids.is_contiguous():
            raise TypeError("input_ids: a 2-D C-contiguous NumPy array, or torch tensor on the GPU, of int32 or int64")
        dev = input_ids.device
        spec = N.mlm_spec(voc.cls_tab.size, voc.mask_id, select_below, mask_below, random_below, seed, epoch, whole_word,
                          input_ids.dtype == torch.int64)
        with torch.cuda.device(dev):
            if voc.d_mlm is None or voc.d_mlm[0] != dev:
                voc.d_mlm = (dev, torch.from_numpy(voc.cls_tab).to(dev), torch.from_numpy(voc.rand_ids.view(np.int32)).to(dev))
            _, d_cls, d_rand = voc.d_mlm
            out = {"input_ids": torch.empty_like(input_ids), "labels": torch.empty_like(input_ids),
                   "selected": torch.empty(input_ids.shape, dtype=torch.uint8, device=dev) if return_selected else None}
            d_info = torch.empty(len(MLM_COUNTS), dtype=torch.int64, device=dev)
            rows, width = input_ids.shape
            N.check(N.lib().swt_mlm_mask_dev(input_ids.data_ptr() or d_info.data_ptr(), rows, width, d_cls.data_ptr(), d_rand.data_ptr(),
                                             int(d_rand.numel()), C.byref(spec), out["input_ids"].data_ptr() or d_info.data_ptr(),
                                             out["labels"].data_ptr() or d_info.data_ptr(),
                                             out["selected"].data_ptr() or d_info.data_ptr() if return_selected else None,
                                             d_info.data_ptr(), torch.cuda.current_stream().cuda_stream))
            info = d_info.cpu().numpy()
    res = {"input_ids": out["input_ids"], "labels": out["labels"]}
    if return_selected:
        res["selected"] = out["selected"]
    res.update((name, int(x)) for name, x in zip(MLM_COUNTS, info))
    return res


class _LabelRows:
    """What the label calls read of an encode_batch(..., return_offsets=True) result: NumPy arrays (the host forms) or torch
    tensors on the GPU (the `_dev` forms on the current stream), the side whose columns are token columns, and the layout of the
    rows -- whether they carry specials and on which side they are padded -- taken from the rows themselves."""

    def __init__(self, batch, side, pair_default):
        if not isinstance(batch, dict) or "input_ids" not in batch:
            raise TypeError("batch: a result of encode_batch(..., return_offsets=True)")
        if "word_ids" not in batch or "offset_mapping" not in batch:
            if "sample_ids" in batch:
                raise ValueError("packed batches have no word_ids: labels go with padded rows or windows")
            raise ValueError("the batch has no word_ids and offset_mapping: encode_batch(..., return_offsets=True) makes them")
        ids = batch["input_ids"]
        self.torch = None
        if not isinstance(ids, np.ndarray):
            import torch
            if not isinstance(ids, torch.Tensor) or not ids.is_cuda:
                raise TypeError("batch: NumPy arrays, or torch tensors on the GPU")
            self.torch = torch
        kind = np.ndarray if self.torch is None else self.torch.Tensor
        self.rows, self.width = int(ids.shape[0]), int(ids.shape[1])
        self.ids64 = "int64" in str(ids.dtype)
        self.word, self.spans, self.length, self.mask = batch["word_ids"], batch["offset_mapping"], batch["length"], batch["attention_mask"]
        self.seq, self.sample = batch.get("sequence_ids"), batch.get("overflow_to_sample_mapping")
        for a in (self.word, self.spans, self.length, self.mask, self.seq, self.sample):
            if a is not None and not isinstance(a, kind):
                raise TypeError("batch: every array a NumPy array, or every one a torch tensor on the GPU")
        if self.seq is None:
            if side not in (None, 0):
                raise ValueError("side: single rows have side 0 alone")
            self.side = 0
        else:
            if side is None:
                side = pair_default
            if side not in (0, 1):
                raise ValueError("side is 0 or 1: pair rows need to be told whose words the labels are")
            self.side = int(side)

    def layout(self):
        """-> (specials, pad_left), from attention_mask, word_ids and length: rows are padded on the left when a row shorter
        than the width starts with padding, and carry specials when a row's first column of content holds no word"""
        if not self.rows or not self.width:
            return False, False
        if self.torch is None:
            n = self.length.astype(np.int64)
            short = (n > 0) & (n < self.width)
            pad_left = bool(((self.mask[:, 0] == 0) & short).any())
            first = np.where(n > 0, self.width - n, 0) if pad_left else np.zeros(self.rows, dtype=np.int64)
            head = self.word[np.arange(self.rows), first]
            return bool(((head.astype(np.int64) & 0xFFFFFFFF == 0xFFFFFFFF) & (n > 0)).any()), pad_left
        n = self.length.long()
        short = (n > 0) & (n < self.width)
        pad_left = bool(((self.mask[:, 0] == 0) & short).any())
        first = self.torch.where(n > 0, self.width - n, 0) if pad_left else self.torch.zeros_like(n)
        head = self.word.gather(1, first.unsqueeze(1)).squeeze(1)
        return bool(((head == -1) & (n > 0)).any()), pad_left

    def upload(self, a):
        """a NumPy array of 32- or 64-bit integers as a tensor on the rows' device"""
        signed = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(a.dtype)
        return self.torch.from_numpy(np.ascontiguousarray(a.view(signed) if signed else a)).to(self.word.device)

    def ptr(self, a, spare):
        """the address of a tensor; `spare`'s for one of no element; None for no tensor"""
        return None if a is None else a.data_ptr() or spare.data_ptr()


def _word_labels(word_labels):
    """-> (lab_off uint64[n + 1], lab int32): a list of int lists, one per text, or (values, offsets) arrays"""
    if isinstance(word_labels, tuple) and len(word_labels) == 2:
        lab, off = np.ascontiguousarray(word_labels[0], dtype=np.int32), np.ascontiguousarray(word_labels[1], dtype=np.uint64)
        if off.ndim != 1 or off.size < 1 or lab.ndim != 1 or (np.diff(off.astype(np.int64)) < 0).any() or int(off[-1]) > lab.size:
            raise ValueError("word_labels: offsets hold n_texts + 1 entries that do not decrease and end inside the values")
        return off, lab
    if not isinstance(word_labels, list) or not all(isinstance(x, (list, tuple, np.ndarray)) for x in word_labels):
        raise TypeError("word_labels: a list of int lists, one per text, or (values, offsets) arrays")
    off = np.zeros(len(word_labels) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(x) for x in word_labels], dtype=np.uint64)
    lab = np.fromiter((int(v) for x in word_labels for v in x), dtype=np.int32, count=int(off[-1]))
    return off, lab


def align_word_labels(batch, word_labels, label_all_tokens=False, inside=None, side=None, ignore_index=N.LABEL_IGNORE):
    """SubwordTokenizer.align_word_labels: NumPy arrays through swt_label_words, torch tensors on the GPU through
    swt_label_words_dev on the current device and stream, with `info` the only read-back of a batch that is in order."""
    rows = _LabelRows(batch, side, None)
    lab_off, lab = _word_labels(word_labels)
    if inside is not None:
        inside = np.ascontiguousarray(inside, dtype=np.int32)
        if inside.ndim != 1:
            raise ValueError("inside: one label per label")
    n_texts = int(lab_off.size) - 1
    if rows.torch is None:
        out = N.label_words(rows.word, lab_off, lab, rows.seq, rows.side, rows.sample, inside, label_all_tokens, rows.ids64, ignore_index)
        labels, info, status, sample = out["labels"], out["info"], out["status"], rows.sample
    else:
        torch = rows.torch
        with torch.cuda.device(rows.word.device):
            d_off, d_lab, d_inside = rows.upload(lab_off), rows.upload(lab), None if inside is None else rows.upload(inside)
            labels = torch.empty((rows.rows, rows.width), dtype=torch.int64 if rows.ids64 else torch.int32, device=rows.word.device)
            d_status = torch.empty(max(rows.rows, 1), dtype=torch.uint8, device=rows.word.device)
            d_info = torch.empty(N.LABEL_COUNTS, dtype=torch.int64, device=rows.word.device)
            word, seq, sample = rows.word.contiguous(), None if rows.seq is None else rows.seq.contiguous(), rows.sample
            p = lambda a: rows.ptr(a, d_info)
            N.check(N.lib().swt_label_words_dev(p(word), p(seq), rows.side, p(sample), rows.rows, rows.width, p(d_off), p(d_lab), int(lab.size),
                                                n_texts, p(d_inside), 0 if inside is None else int(inside.size), int(ignore_index),
                                                (N.LABEL_ALL_TOKENS if label_all_tokens else 0) | (N.LABEL_IDS64 if rows.ids64 else 0),
                                                p(labels), d_status.data_ptr(), d_info.data_ptr(), torch.cuda.current_stream().cuda_stream))
            info = d_info.cpu().numpy()
            status = d_status[:rows.rows].cpu().numpy() if info[2] else None
            sample = sample.cpu().numpy() if info[2] and sample is not None else None
    if info[3]:
        raise ValueError("align_word_labels: %d rows name a text beyond the %d of word_labels" % (int(info[3]), n_texts))
    if info[2]:
        row = int(np.flatnonzero(status)[0])
        text = row if sample is None else int(sample[row])
        raise ValueError("align_word_labels: row %d names a word beyond the %d labels of text %d"
                         % (row, int(lab_off[text + 1]) - int(lab_off[text]), text))
    return {"labels": labels, "n_labelled": int(info[0]), "n_continuation": int(info[1])}


def _lower_positions(text, positions):
    """indices into `text` as indices into text.lower(): the running sum of len(ch.lower())"""
    at = np.zeros(len(text) + 1, dtype=np.int64)
    at[1:] = np.cumsum([len(ch.lower()) for ch in text])
    return [int(at[min(max(int(p), 0), len(text))]) for p in positions]


def _answers(answers, texts):
    """-> uint32[n, 2]: (a, e) per text in the unit of offset_mapping, (NO_ANSWER, NO_ANSWER) for None or a negative start"""
    if isinstance(answers, np.ndarray):
        answers = answers.tolist()
    if not isinstance(answers, (list, tuple)):
        raise TypeError("answers: one (start, end) per text, None or (-1, -1) for a text without an answer")
    if texts is not None and (not isinstance(texts, list) or len(texts) != len(answers) or not all(isinstance(t, str) for t in texts)):
        raise ValueError("texts holds one string for every answer")
    ans = np.full((len(answers), 2), N.NO_ANSWER, dtype=np.uint32)
    for i, x in enumerate(answers):
        if x is None:
            continue
        if len(x) != 2:
            raise ValueError("answers: one (start, end) per text")
        a, e = int(x[0]), int(x[1])
        if a < 0 or e < 0:
            continue
        if texts is not None and len(texts[i].lower()) != len(texts[i]):
            a, e = _lower_positions(texts[i], (a, e))
        if a >= N.NO_ANSWER or e > N.NO_ANSWER:
            raise ValueError("answers: a position of 2^32 - 1 or more")
        ans[i] = (a, e)
    return ans


def answer_positions(batch, answers, side=None, texts=None, ignore_index=N.LABEL_IGNORE):
    """SubwordTokenizer.answer_positions: NumPy arrays through swt_answer_positions, torch tensors on the GPU through its `_dev`
    form on the current device and stream; `info` and the rows' layout are the read-backs."""
    rows = _LabelRows(batch, side, 1)
    ans = _answers(answers, texts)
    specials, pad_left = rows.layout()
    pad_left = pad_left and specials  # without [CLS] the nothing column is ignore_index on either side
    if rows.torch is None:
        out = N.answer_positions(rows.spans, ans, rows.word, rows.seq, rows.side, rows.sample, rows.length, specials, pad_left, rows.ids64,
                                 ignore_index)
        info = out["info"]
    else:
        torch = rows.torch
        dev = rows.word.device
        with torch.cuda.device(dev):
            t = torch.int64 if rows.ids64 else torch.int32
            out = {"start": torch.empty(rows.rows, dtype=t, device=dev), "end": torch.empty(rows.rows, dtype=t, device=dev),
                   "has": torch.empty(rows.rows, dtype=torch.uint8, device=dev), "hit": torch.empty(ans.shape[0], dtype=torch.uint8, device=dev)}
            d_info, d_ans = torch.empty(N.ANSWER_COUNTS, dtype=torch.int64, device=dev), rows.upload(ans)
            p = lambda a: rows.ptr(a, d_info)
            seq = None if rows.seq is None else rows.seq.contiguous()
            flags = (N.ANSWER_CLS if specials else 0) | (N.ANSWER_PAD_LEFT if pad_left else 0) | (N.LABEL_IDS64 if rows.ids64 else 0)
            N.check(N.lib().swt_answer_positions_dev(p(rows.spans.contiguous()), p(rows.word.contiguous()), p(seq), rows.side, p(rows.sample),
                                                     rows.rows, rows.width, p(d_ans), int(ans.shape[0]), p(rows.length.contiguous()),
                                                     int(ignore_index), flags, p(out["start"]), p(out["end"]), p(out["has"]), p(out["hit"]),
                                                     d_info.data_ptr(), torch.cuda.current_stream().cuda_stream))
            info = d_info.cpu().numpy()
    if info[2]:
        raise ValueError("answer_positions: %d rows name a text beyond the %d of answers" % (int(info[2]), ans.shape[0]))
    return {"start_positions": out["start"], "end_positions": out["end"], "has_answer": out["has"], "sample_has_answer_row": out["hit"],
            "n_with": int(info[0]), "n_without": int(info[1])}


def best_answers(batch, start_logits, end_logits, max_answer_length=30, side=None, texts=None):
    """SubwordTokenizer.best_answers: NumPy arrays through swt_answer_best, torch tensors on the GPU through its `_dev` form on
    the current device and stream; the rows' layout and, without `texts`, the last row's text are the read-backs."""
    rows = _LabelRows(batch, side, 1)
    kind, f32 = (np.ndarray, np.float32) if rows.torch is None else (rows.torch.Tensor, rows.torch.float32)
    for name, a in (("start_logits", start_logits), ("end_logits", end_logits)):
        if not isinstance(a, kind) or a.dtype != f32 or (rows.torch is not None and not a.is_cuda):
            raise TypeError("%s: float32, a NumPy array or a torch tensor on the GPU as the batch is" % name)
        if tuple(a.shape) != (rows.rows, rows.width):
            raise ValueError("%s has the shape of input_ids" % name)
    if int(max_answer_length) < 1:
        raise ValueError("max_answer_length is 1 or more")
    if texts is not None and (not isinstance(texts, list) or not all(isinstance(t, str) for t in texts)):
        raise TypeError("texts: the strings of that side, one per text")
    if texts is not None:
        n_texts = len(texts)
    elif rows.sample is None or not rows.rows:
        n_texts = rows.rows
    else:
        n_texts = int(rows.sample[-1]) + 1
    specials, pad_left = rows.layout()
    pad_left = pad_left and specials
    max_len = min(int(max_answer_length), 0xFFFFFFFF)
    if rows.torch is None:
        out = N.answer_best(np.ascontiguousarray(start_logits), np.ascontiguousarray(end_logits), rows.spans, n_texts, rows.word, rows.seq,
                            rows.side, rows.sample, max_len, rows.length, specials, pad_left, per_row=False, info=False)
    else:
        torch = rows.torch
        dev = rows.word.device
        with torch.cuda.device(dev):
            types = {np.float32: torch.float32, np.int32: torch.int32, np.uint32: torch.int32}
            out = {name: torch.empty(n_texts, dtype=types[t], device=dev) for name, t in N.BEST_TEXT}
            spare = torch.empty(2, dtype=torch.int64, device=dev)
            p = lambda a: rows.ptr(a, spare)
            seq = None if rows.seq is None else rows.seq.contiguous()
            flags = (N.ANSWER_CLS if specials else 0) | (N.ANSWER_PAD_LEFT if pad_left else 0)
            N.check(N.lib().swt_answer_best_dev(p(start_logits.contiguous()), p(end_logits.contiguous()), p(rows.spans.contiguous()),
                                                p(rows.word.contiguous()), p(seq), rows.side, p(rows.sample), rows.rows, rows.width, n_texts,
                                                max_len, p(rows.length.contiguous()), flags, *[p(out[name]) for name, _ in N.BEST_TEXT],
                                                None, None, None, None, torch.cuda.current_stream().cuda_stream))
    res = {name: out[name] for name, _ in N.BEST_TEXT}
    if texts is not None:
        cs, ce = (x if rows.torch is None else x.cpu().numpy() for x in (out["char_start"], out["char_end"]))
        res["text"] = [t.lower()[int(a):int(b)] for t, a, b in zip(texts, cs.astype(np.int64), ce.astype(np.int64))]
    return res


def _n_texts(rows, n_texts):
    """the texts of a batch: what the caller says, else one per row, or with windows the last row's text + 1 (a read-back)"""
    if n_texts is not None:
        return int(n_texts)
    if rows.sample is None or not rows.rows:
        return rows.rows
    return int(rows.sample[-1]) + 1


def word_predictions(batch, logits, strategy="first", side=None, return_logits=False, n_texts=None):
    """SubwordTokenizer.word_predictions: NumPy arrays through swt_word_plan / swt_word_predict, torch tensors on the GPU through
    their `_dev` forms on the current device and stream; the word total and `info` are the read-backs."""
    rows = _LabelRows(batch, side, None)
    kind, f32 = (np.ndarray, np.float32) if rows.torch is None else (rows.torch.Tensor, rows.torch.float32)
    if not isinstance(logits, kind) or logits.dtype != f32 or (rows.torch is not None and not logits.is_cuda):
        raise TypeError("logits: float32, a NumPy array or a torch tensor on the GPU as the batch is")
    if len(logits.shape) != 3 or tuple(logits.shape[:2]) != (rows.rows, rows.width) or int(logits.shape[2]) < 1:
        raise ValueError("logits has the shape [rows, width, n_labels] over the rows of input_ids")
    if strategy not in N.TAG_STRATEGIES:
        raise ValueError("strategy is 'first', 'mean' or 'max'")
    n_texts, n_labels = _n_texts(rows, n_texts), int(logits.shape[2])
    if rows.torch is None:
        word_off, plan = N.word_plan(rows.word, n_texts, rows.seq, rows.side, rows.sample)
        out = N.word_predict(np.ascontiguousarray(logits), rows.word, rows.spans, word_off, rows.seq, rows.side, rows.sample,
                             N.TAG_STRATEGIES[strategy], word_logits=return_logits)
        info = out["info"]
    else:
        torch = rows.torch
        dev = rows.word.device
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream().cuda_stream
            d_off = torch.empty(n_texts + 1, dtype=torch.int64, device=dev)
            d_plan, d_info = torch.empty(N.PLAN_COUNTS, dtype=torch.int64, device=dev), torch.empty(N.PREDICT_COUNTS, dtype=torch.int64, device=dev)
            p = lambda a: rows.ptr(a, d_info)
            word, seq = rows.word.contiguous(), None if rows.seq is None else rows.seq.contiguous()
            N.check(N.lib().swt_word_plan_dev(p(word), p(seq), rows.side, p(rows.sample), rows.rows, rows.width, n_texts, d_off.data_ptr(),
                                              d_plan.data_ptr(), stream))
            plan = d_plan.cpu().numpy()  # the one read-back before the words: how many there are
            n_words = int(plan[0])
            types = {np.float32: torch.float32, np.int32: torch.int32, np.uint32: torch.int32}
            out = {name: torch.empty(n_words, dtype=types[t], device=dev) for name, t in N.WORD_OUT}
            out["logits"] = torch.empty((n_words, n_labels), dtype=torch.float32, device=dev) if return_logits else None
            N.check(N.lib().swt_word_predict_dev(p(logits.contiguous()), p(word), p(seq), rows.side, p(rows.sample), p(rows.spans.contiguous()),
                                                 rows.rows, rows.width, n_labels, d_off.data_ptr(), n_texts, n_words,
                                                 N.TAG_STRATEGIES[strategy], *[p(out[name]) for name, _ in N.WORD_OUT], p(out["logits"]),
                                                 d_info.data_ptr(), stream))
            info = d_info.cpu().numpy()
            word_off = d_off.view(torch.uint64)
    if plan[1]:
        raise ValueError("word_predictions: %d rows name a text beyond the %d of the batch" % (int(plan[1]), n_texts))
    res = {"word_offsets": word_off}
    res.update((name, out[name]) for name, _ in N.WORD_OUT)
    if return_logits:
        res["logits"] = out["logits"]
    res.update({"n_words": int(info[0]), "n_missing": int(info[1])})
    return res


def _label_scheme(id2label):
    """-> (etype int32[L], begins uint8[L], type_names): "B-x" and "I-x" are of type x and "B-x" begins; "O" is outside; any
    other name is its own type and never begins"""
    if not isinstance(id2label, (list, tuple)) or not id2label or not all(isinstance(x, str) for x in id2label):
        raise TypeError("id2label: a list of label names, the name of label i at index i")
    names, etype, begins = [], np.full(len(id2label), -1, dtype=np.int32), np.zeros(len(id2label), dtype=np.uint8)
    for i, name in enumerate(id2label):
        if name == "O":
            continue
        kind = name[2:] if name[:2] in ("B-", "I-") and len(name) > 2 else name
        if kind not in names:
            names.append(kind)
        etype[i], begins[i] = names.index(kind), name[:2] == "B-" and len(name) > 2
    return etype, begins, names


def entities(words, id2label, texts=None):
    """SubwordTokenizer.entities: the word arrays of word_predictions through swt_entity_spans (NumPy) or its `_dev` form (torch
    tensors on the GPU, on the current device and stream); the count is the read-back that cuts the arrays."""
    need = ("word_offsets", "label", "score", "char_start", "char_end")
    if not isinstance(words, dict) or not all(k in words for k in need):
        raise TypeError("words: a result of word_predictions")
    etype, begins, names = _label_scheme(id2label)
    if texts is not None and (not isinstance(texts, list) or not all(isinstance(t, str) for t in texts)):
        raise TypeError("texts: the strings of that side, one per text")
    label = words["label"]
    n_texts = int(words["word_offsets"].shape[0]) - 1
    if texts is not None and len(texts) != n_texts:
        raise ValueError("texts holds one string for every text of the words")
    if isinstance(label, np.ndarray):
        out = N.entity_spans(label, words["score"], words["char_start"], words["char_end"], words["word_offsets"], etype, begins)
        info = out["info"]
        n = int(info[0])
        res = {name: out[name][:n] for name, _ in N.ENTITY_OUT}
    else:
        import torch
        if not isinstance(label, torch.Tensor) or not label.is_cuda:
            raise TypeError("words: NumPy arrays, or torch tensors on the GPU")
        dev = label.device
        with torch.cuda.device(dev):
            n_words = int(label.shape[0])
            types = {np.float32: torch.float32, np.int32: torch.int32, np.uint32: torch.int32}
            out = {name: torch.empty(n_words, dtype=types[t], device=dev) for name, t in N.ENTITY_OUT}
            d_info = torch.empty(N.ENTITY_COUNTS, dtype=torch.int64, device=dev)
            d_etype, d_begins = torch.from_numpy(etype).to(dev), torch.from_numpy(begins).to(dev)
            p = lambda a: a.data_ptr() or d_info.data_ptr()
            N.check(N.lib().swt_entity_spans_dev(*[p(words[k].contiguous()) for k in need[1:]], p(words["word_offsets"].contiguous()), n_texts,
                                                 n_words, p(d_etype), p(d_begins), int(etype.size), *[p(out[name]) for name, _ in N.ENTITY_OUT],
                                                 d_info.data_ptr(), torch.cuda.current_stream().cuda_stream))
            info = d_info.cpu().numpy()
            n = int(info[0])
            res = {name: out[name][:n] for name, _ in N.ENTITY_OUT}
    res.update({"type_names": names, "n_entities": n, "n_entity_words": int(info[1])})
    if texts is not None:
        ti, cs, ce = (x if isinstance(x, np.ndarray) else x.cpu().numpy() for x in (res["text_index"], res["char_start"], res["char_end"]))
        res["text"] = [texts[int(i)].lower()[int(a):int(b)] for i, a, b in zip(ti, cs.astype(np.int64), ce.astype(np.int64))]
    return res


def _fill_predict(ids, value, not_equal, logits, labels, top_k, what):
    """What fill_mask and mlm_scores share: the cells of `ids` that equal `value` (or do not) through swt_mlm_positions, the scores
    of their rows of logits through swt_mlm_predict -- NumPy arrays through the host forms, torch tensors on the GPU through the
    `_dev` forms on the current device and stream, the position count and `info` the only read-backs.
    -> (dict: row, col, lse, top_id, top_logit, logprob, score, label_id, label_logit, label_rank; info)"""
    if isinstance(top_k, bool) or not isinstance(top_k, (int, np.integer)) or not 1 <= int(top_k) <= 64:
        raise ValueError("top_k lies in 1 .. 64")
    k = int(top_k)
    if isinstance(ids, np.ndarray):
        torch = None
        ok = ids.dtype in (np.int32, np.int64) and ids.ndim == 2 and ids.flags.c_contiguous
        logits_ok = isinstance(logits, np.ndarray) and logits.dtype == np.float32
    else:
        import torch
        ok = isinstance(ids, torch.Tensor) and ids.is_cuda and ids.dtype in (torch.int32, torch.int64) and ids.dim() == 2 and ids.is_contiguous()
        logits_ok = isinstance(logits, torch.Tensor) and logits.is_cuda and logits.dtype == torch.float32
    if not ok:
        raise TypeError("%s: a 2-D C-contiguous NumPy array, or torch tensor on the GPU, of int32 or int64" % what)
    if not logits_ok:
        raise TypeError("logits: float32, a NumPy array or a torch tensor on the GPU as %s is" % what)
    rows, width = int(ids.shape[0]), int(ids.shape[1])
    if len(logits.shape) != 3 or tuple(logits.shape[:2]) != (rows, width) or int(logits.shape[2]) < 1:
        raise ValueError("logits has the shape [rows, width, V] over the rows of %s" % what)
    if not (logits.flags.c_contiguous if torch is None else logits.is_contiguous()):
        raise ValueError("logits is C-contiguous: a copy of it is what these calls are there to avoid")
    if torch is None:
        pos, plan = N.mlm_positions(ids, value, not_equal)
        pos = pos[:int(plan[0])]
        out = N.mlm_predict(logits, pos, labels, k)
        info = out["info"]
        cell = pos.astype(np.int64)
        xp_exp = np.exp
    else:
        dev = ids.device
        if logits.device != dev:
            raise TypeError("logits: a torch tensor on the device of %s" % what)
        ids64 = ids.dtype == torch.int64
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream().cuda_stream
            d_plan, d_info = torch.empty(N.POSITION_COUNTS, dtype=torch.int64, device=dev), torch.empty(N.FILL_COUNTS, dtype=torch.int64, device=dev)
            d_pos = torch.empty(rows * width, dtype=torch.int64, device=dev)
            d_spare = torch.empty(2, dtype=torch.int64, device=dev)  # a tensor of no element still needs an address
            p = lambda a: None if a is None else a.data_ptr() or d_spare.data_ptr()
            N.check(N.lib().swt_mlm_positions_dev(p(ids), rows, width, int(value), N.FILL_NOT_EQUAL if not_equal else N.FILL_EQUAL,
                                                  N.FILL_IDS64 if ids64 else 0, p(d_pos), d_plan.data_ptr(), stream))
            n = int(d_plan.cpu().numpy()[0])  # the one read-back before the scores: how many positions there are
            types = {np.float32: torch.float32, np.int32: torch.int32}
            wanted = [name for name, _, _ in N.FILL_OUT if labels is not None or not name.startswith("label")]
            out = {name: torch.empty((n, k) if per_k else n, dtype=types[t], device=dev) if name in wanted else None
                   for name, t, per_k in N.FILL_OUT}
            N.check(N.lib().swt_mlm_predict_dev(p(logits), rows, width, int(logits.shape[2]), p(d_pos), n, p(labels),
                                                N.FILL_IDS64 if ids64 else 0, k, *[p(out[name]) for name, _, _ in N.FILL_OUT],
                                                d_info.data_ptr(), stream))
            info = d_info.cpu().numpy()
            cell = d_pos[:n]
            xp_exp = torch.exp
    out["row"], out["col"] = cell // width, cell % width
    out["logprob"] = out["top_logit"] - out["lse"][:, None]
    out["score"] = xp_exp(out["logprob"])
    return out, info


def _kept_sum(keep, x):
    """the sum of x where keep holds, as a 0-d tensor: what is not kept, a NaN included, adds nothing"""
    return x.where(keep, x.new_zeros(())).sum()


def _fill_top(out):
    return {"token_ids": out["top_id"], "logit": out["top_logit"], "logprob": out["logprob"], "score": out["score"], "lse": out["lse"]}


def fill_mask(tok, input_ids, logits, top_k=5, tokens=False):
    """SubwordTokenizer.fill_mask: the columns with input_ids == mask_id()."""
    voc = tok._batch_vocabulary()
    out, info = _fill_predict(input_ids, voc.mask_id, False, logits, None, top_k, "input_ids")
    res = {"row": out["row"], "col": out["col"]}
    res.update(_fill_top(out))
    res["n_positions"] = int(info[0])
    if tokens:
        ids = out["top_id"] if isinstance(out["top_id"], np.ndarray) else out["top_id"].cpu().numpy()
        names = list(voc.tokens) + ([MASK] if voc.mask_id == len(voc.tokens) else [])
        res["tokens"] = [[names[i] if 0 <= i < len(names) else None for i in row] for row in ids.tolist()]
    return res


def mlm_scores(logits, labels, top_k=1):
    """SubwordTokenizer.mlm_scores: the columns with labels != -100."""
    out, info = _fill_predict(labels, N.LABEL_IGNORE, True, logits, labels, top_k, "labels")
    res = {"row": out["row"], "col": out["col"], "label": out["label_id"], "label_logprob": out["label_logit"] - out["lse"],
           "label_rank": out["label_rank"]}
    res.update(_fill_top(out))
    n, n_in = int(info[0]), int(info[0]) - int(info[4])
    lp, known = res["label_logprob"], out["label_id"] >= 0  # a masked sum: no gather, and on the device no read-back
    if isinstance(lp, np.ndarray):
        loss = float(np.where(known, -lp.astype(np.float64), 0.0).sum() / n_in) if n_in else float("nan")
        perplexity = float(np.exp(loss))
    else:
        neg = -lp.double()
        loss = _kept_sum(known, neg) / n_in if n_in else neg.new_full((), float("nan"))
        perplexity = loss.exp()
    res.update({"loss": loss, "perplexity": perplexity, "accuracy": int(info[1]) / n if n else float("nan"),
                "accuracy_at_k": int(info[2]) / n if n else float("nan"), "n_positions": n, "n_correct": int(info[1]),
                "n_correct_at_k": int(info[2]), "n_nan": int(info[3]), "n_out_of_range": int(info[4])})
    return res


def _raise_decode_status(status, row):
    """the ValueError of a plan whose info counts reported rows: the first such row and its cause"""
    causes = [text for bit, text in ((N.DECODE_BAD_ID, "an id outside the vocabulary on a kept column"),
                                     (N.DECODE_BAD_TOKEN, "a token that is empty or holds whitespace, which recover_sentence does not spell"))
              if status & bit]
    raise ValueError("decode_batch: row %d holds %s" % (row, " and ".join(causes)))


def decode_batch_bytes(tok, input_ids, attention_mask=None, skip_special_tokens=True):
    """SubwordTokenizer.decode_batch_bytes: a NumPy array through swt_decode_plan / swt_decode_rows, a torch tensor on the GPU
    through their `_dev` forms on the current device and stream, with `info` the only read-back."""
    if isinstance(input_ids, np.ndarray):
        if input_ids.dtype not in (np.int32, np.int64) or input_ids.ndim != 2 or not input_ids.flags.c_contiguous:
            raise TypeError("input_ids: a 2-D C-contiguous array of int32 or int64")
        voc = tok._batch_vocabulary()
        tok_bytes, tok_off, tok_flags, n_tok = voc.decode_tables
        mask = attention_mask
        if mask is not None:
            mask = np.asarray(mask)
            if mask.shape != input_ids.shape:
                raise ValueError("attention_mask has the shape of input_ids")
            mask = np.ascontiguousarray(mask if mask.dtype == np.uint8 else mask != 0, dtype=np.uint8)
        text_off, status, info = N.decode_plan(input_ids, mask, tok_off, tok_flags, n_tok, skip_special_tokens)
        if info[1]:
            row = int(np.flatnonzero(status)[0])
            _raise_decode_status(int(status[row]), row)
        return N.decode_rows(input_ids, mask, tok_bytes, tok_off, tok_flags, n_tok, text_off, skip_special_tokens), text_off
    import torch
    if not isinstance(input_ids, torch.Tensor) or not input_ids.is_cuda or input_ids.dtype not in (torch.int32, torch.int64) \
            or input_ids.dim() != 2 or not input_ids.is_contiguous():
        raise TypeError("input_ids: a 2-D C-contiguous NumPy array, or torch tensor on the GPU, of int32 or int64")
    dev = input_ids.device
    voc = tok._batch_vocabulary()
    tok_bytes, tok_off, tok_flags, n_tok = voc.decode_tables
    flags = (N.DECODE_SKIP_SPECIAL if skip_special_tokens else 0) | (N.DECODE_IDS64 if input_ids.dtype == torch.int64 else 0)
    with torch.cuda.device(dev):
        mask = attention_mask
        if mask is not None:
            if not isinstance(mask, torch.Tensor) or mask.device != dev or mask.shape != input_ids.shape:
                raise TypeError("attention_mask: a torch tensor on the device of input_ids and of its shape")
            mask = (mask if mask.dtype == torch.uint8 else (mask != 0).to(torch.uint8)).contiguous()
        if voc.d_decode is None or voc.d_decode[0] != dev:
            voc.d_decode = (dev, torch.from_numpy(tok_bytes.copy()).to(dev), torch.from_numpy(tok_off.view(np.int32)).to(dev),
                            torch.from_numpy(tok_flags).to(dev))
        _, d_bytes, d_off, d_flags = voc.d_decode
        rows, width = input_ids.shape
        stream = torch.cuda.current_stream().cuda_stream
        d_text_off = torch.empty(rows + 1, dtype=torch.int64, device=dev)
        d_status = torch.empty(max(rows, 1), dtype=torch.uint8, device=dev)
        d_info = torch.empty(3, dtype=torch.int64, device=dev)
        head = (input_ids.data_ptr() or d_info.data_ptr(), mask.data_ptr() or d_info.data_ptr() if mask is not None else None, rows, width)
        lib = N.lib()
        N.check(lib.swt_decode_plan_dev(*head, d_off.data_ptr(), d_flags.data_ptr(), n_tok, flags, d_text_off.data_ptr(), d_status.data_ptr(),
                                        d_info.data_ptr(), stream))
        info = d_info.cpu().numpy()  # the one read-back: the size of the text, and whether a row is reported
        if info[1]:
            status = d_status[:rows].cpu().numpy()
            row = int(np.flatnonzero(status)[0])
            _raise_decode_status(int(status[row]), row)
        total = int(info[0])
        text = torch.empty(total, dtype=torch.uint8, device=dev)
        if total:
            N.check(lib.swt_decode_rows_dev(*head, d_bytes.data_ptr(), d_off.data_ptr(), d_flags.data_ptr(), n_tok, flags, d_text_off.data_ptr(),
                                            text.data_ptr(), total, stream))
    return text, d_text_off.view(torch.uint64)


def decode_batch(tok, input_ids, attention_mask=None, skip_special_tokens=True):
    text, off = decode_batch_bytes(tok, input_ids, attention_mask, skip_special_tokens)
    if not isinstance(text, np.ndarray):
        text, off = text.cpu().numpy(), off.cpu().numpy()
    raw, off = text.tobytes(), off.astype(np.int64).tolist()
    return [raw[a:b].decode("utf-8") for a, b in zip(off[:-1], off[1:])]
