"""The reference's tokenizer classes with the inner loops on the MI355X.

Same names, constructor, methods, attributes and error behaviour as phtryll/subword-tokenizers
(`source/bpe.py`, `source/wordpiece.py`, `source/utils.py`; citations below are relative to /root/reference):

    SubwordTokenizer   utils.py:5-41      preprocessing(), vocab_length()
    NaiveBPE           bpe.py:9-189       train() on the device; encode_word()/tokenize() stay the slow didactic loop, the batch calls run it on the device
    FastBPE            bpe.py:192-263     train() + tokenize()/encode_word() on the device
    NaiveWP            wordpiece.py:8-208 train() on the device; tokenize() stays the Python loop, the batch calls run it on the device
    FastWP             wordpiece.py:211-330  trie build in C++, tokenize() on the device

plus batch entry points the reference lacks (`tokenize_batch`, `encode_ids_batch`), because one sentence per
call cannot feed a GPU.  Python keeps exactly what the reference does in Python: `str.lower()`, JSON I/O, the
id <-> string maps and the stop test of the training loop.  Everything else goes through libswt_hip.so; there
is no CPU fallback -- without a GPU the compute calls raise `NoDeviceError`.
"""
import json
import os
import weakref
from collections import Counter
from typing import Dict, List, Optional, Tuple

import ctypes as C

import numpy as np

from . import _native as N
from . import batching

__all__ = ["SubwordTokenizer", "NaiveBPE", "FastBPE", "NaiveWP", "FastWP", "TrieView"]


def _is_bert_pretokenizer(tokenizer) -> bool:
    try:
        pt = tokenizer.backend_tokenizer.pre_tokenizer
    except AttributeError:
        return False
    return type(pt).__name__ == "BertPreTokenizer"


class SubwordTokenizer:
    """Parent class (utils.py:5-41).

    `tokenizer` is the HF tokenizer object the reference takes (cli.py:163,194); it is only ever used for its
    BertPreTokenizer (utils.py:27).  It may be None: the split is restated from the probed class table that is
    compiled into libswt_hip.so (White_Space removed, each punctuation code point isolated).
    """

    def __init__(self, tokenizer=None) -> None:
        if tokenizer is not None and not _is_bert_pretokenizer(tokenizer):
            raise ValueError("only a BertPreTokenizer-backed tokenizer (the reference's default, cli.py:85) is supported")
        self.tokenizer = tokenizer
        self._added: List[Tuple[str, bool]] = []  # the added tokens (content, special) in the order of addition
        self._added_gen = 0  # counts the changes of the list: part of the vocabulary's cache key
        self._added_handle: Optional[N.AddedPatterns] = None

    # -- utils.py:15-29
    def preprocessing(self, corpus: List[str]) -> List[List[Tuple[str, Tuple[int, int]]]]:
        return [self._split(example.lower()) for example in corpus]

    @staticmethod
    def _split(text: str) -> List[Tuple[str, Tuple[int, int]]]:
        out = []
        i, n = 0, len(text)
        cls = _class_of
        while i < n:
            c = cls(text[i])
            if c & N.CLS_BERT_WS:
                i += 1
                continue
            j = i + 1
            if not c & N.CLS_BERT_PUNCT:
                while j < n and not cls(text[j]) & (N.CLS_BERT_WS | N.CLS_BERT_PUNCT):
                    j += 1
            out.append((text[i:j], (i, j)))
            i = j
        return out

    # -- utils.py:31-41
    def vocab_length(self, corpus: List[str]) -> int:
        return len({symbol for example in corpus for symbol in example})

    # -- model-ready batches (not in the reference; batching.py).  A class supplies its _Encoder as `_enc` and
    # encode_ids_batch; the hooks of batching.py are at the end of this class.
    def vocab_list(self) -> List[str]:
        """The token strings in dense-id order: row i of a model's embedding table belongs to vocab_list()[i].  It depends on
        nothing but what save_resources keeps."""
        return list(self._batch_vocabulary().tokens)

    def token_to_id(self, token: str) -> int:
        """dense id of a token string; [UNK]'s for a string the vocabulary does not hold"""
        voc = self._batch_vocabulary()
        return voc.index.get(token, voc.special["unk"])

    def special_ids(self) -> Dict[str, int]:
        """{"pad", "unk", "cls", "sep"} -> dense id"""
        return dict(self._batch_vocabulary().special)

    def encode_batch(self, texts: List[str], max_length: Optional[int] = None, stride: int = 0, padding: str = "longest",
                     pad_to_multiple_of: Optional[int] = None, add_special_tokens: bool = True, padding_side: str = "right",
                     return_overflowing: bool = False, return_offsets: bool = False, int64: bool = False, device: bool = False,
                     text_pairs: Optional[List[str]] = None, truncation: str = "longest_first",
                     return_token_type_ids: Optional[bool] = None, return_special_tokens_mask: bool = False,
                     packing: Optional[str] = None, drop_last: bool = False, mlm: Optional[dict] = None,
                     dropout: Optional[dict] = None, maxmatch_dropout: Optional[dict] = None) -> dict:
        """texts -> {"input_ids" [rows, width], "attention_mask", "length", "n_unknown"} with dense ids (vocab_list), [CLS] and
        [SEP] around every row and [PAD] up to the width, made on the device (swt_batch_rows).  padding="longest": width =
        min(max_length, longest row + specials); "max_length": max_length; both rounded up to pad_to_multiple_of.  A longer row
        is truncated, or with return_overflowing cut into windows that overlap by `stride` tokens ("overflow_to_sample_mapping"
        names each row's text).  return_offsets adds "offset_mapping" [rows, width, 2] and "word_ids" [rows, width] (-1 on
        specials and padding) from this class's span call.  device=False: NumPy arrays; device=True: torch tensors on the
        current device and stream, the ids never leaving the device.

        text_pairs (one text per text) makes every row a pair, [CLS] text [SEP] pair [SEP] (swt_batch_pair_rows): the result
        gains "sequence_ids" (0 on the text's tokens, 1 on the pair's, -1 elsewhere), "token_type_ids" (unless
        return_token_type_ids=False) and with return_special_tokens_mask "special_tokens_mask"; offsets and word ids are each
        side's own.  truncation: "longest_first" takes from the longer side, "only_first" / "only_second" cut the named side
        and spare the other; with return_overflowing the cut side is windowed and the other repeated in every row
        ("longest_first" has no windows).  A pair whose spared side leaves the other no room raises ValueError.  Without
        text_pairs these keywords have nothing to act on and any value but the default raises ValueError.

        packing="whole" or "split" (swt_pack_rows; needs max_length, the width) puts several texts into one row: "whole" next-fit
        in the order given, no text split and a text longer than the width truncated; "split" all texts end to end, cut every
        width columns, with drop_last without a last row that is not full.  The result holds "input_ids", "attention_mask",
        "position_ids" (the column's position inside its text's segment), "sequence_ids" (the segment's number in its row, -1 on
        padding), "sample_ids" (the text's index, -1 on padding), "length", "n_unknown", "n_truncated", per text "segment_row",
        "segment_col" and "segment_length", and "density", the share of columns that are not padding.  Pairs, windows, offsets
        and left padding do not go with packing: ValueError.

        mlm, a dict of mask_tokens keywords ({} for its defaults), masks the finished rows of any of these forms for the masked-LM
        objective: "input_ids" are the masked ids and the result gains "labels" and the five counts of mask_tokens.

        dropout = {"probability": p, "seed": 0, "epoch": 0} (FastBPE; any other class raises ValueError) encodes with BPE-dropout,
        as FastBPE.encode_ids_batch: every form above -- pairs, windows, offsets, packing, mlm, device -- then works on those ids.
        The sentence index of the draws is the text's index, and len(texts) + j for text_pairs[j].

        maxmatch_dropout, a dict of the same three keys (NaiveWP; any other class raises ValueError), encodes with MaxMatch-Dropout
        as NaiveWP.encode_ids_batch does, with the same reach and the same sentence indices."""
        return batching.encode_batch(self, texts, max_length, stride, padding, pad_to_multiple_of, add_special_tokens, padding_side,
                                     return_overflowing, return_offsets, int64, device, text_pairs, truncation, return_token_type_ids,
                                     return_special_tokens_mask, packing, drop_last, mlm, self._enc.channel(dropout, maxmatch_dropout))

    # -- added and special tokens written in the text (not in the reference; include/swt.h)
    def add_tokens(self, tokens: List[str], special: bool = False) -> int:
        """Registers strings that encode_batch keeps whole wherever they stand in a text -- "<user>", a domain term; with
        special=True (add_special_tokens) a control token such as "[MASK]" or "[SEP]".  They are found on the device in the
        lowercased text the encoders see (swt_added_find: leftmost-longest, not overlapping, also inside a word), hidden from the
        encoder and spliced into its output (swt_added_splice), each a word of its own.  The text is lowercased before anything
        else (utils.py:27), so a token is recognised in any case: "[mask]" in a text is "[MASK]".
        The dense id of a token -- its string is `content` for a special one, content.lower() for an ordinary one -- is the
        string's index where the vocabulary holds it (a typed "[SEP]" is [SEP]), mask_id() for "[MASK]", and else the next free id
        from max(len(vocab_list()), mask_id() + 1) on; no other dense id moves and vocab_list() grows by the appended ones.  A
        special token is never masked nor a random replacement (mask_tokens) and is skipped by decode_batch(...,
        skip_special_tokens=True); an ordinary one is a word like any other.
        -> the number of tokens newly added; one whose lowercased form is registered already is not new.  ValueError, naming the
        token: the empty string, whitespace inside, a code point past U+FFFF, a lowercased form of more than 64 bytes, more than
        4096 tokens; on a FastWP whose vocabulary holds a token with whitespace, any token.  The list survives train,
        load_resources and reset (the dense ids follow the new vocabulary); save_resources does not write it: re-add after loading.
        tokenize, tokenize_batch, encode_ids_batch, encode_spans_batch and fast_encode_spans_batch keep the reference's behaviour
        and do not see added tokens."""
        if isinstance(tokens, str) or not isinstance(tokens, (list, tuple)):
            raise TypeError("tokens: a list of strings")
        self._refuse_added()
        staged, have, new = list(self._added), {content.lower() for content, _ in self._added}, 0
        for token in tokens:
            batching.check_added_token(token, 0)
            if token.lower() in have:
                continue
            batching.check_added_token(token, len(staged))
            staged.append((token, bool(special)))
            have.add(token.lower())
            new += 1
        if new:
            self._set_added(staged)
        return new

    def add_special_tokens(self, tokens: List[str]) -> int:
        """add_tokens(tokens, special=True)"""
        return self.add_tokens(tokens, special=True)

    def added_tokens(self) -> List[Tuple[str, bool]]:
        """[(content, special)] in the order of addition"""
        return list(self._added)

    def clear_added_tokens(self) -> None:
        """forgets every added token: encode_batch and vocab_list() are what they were before the first add_tokens"""
        if self._added:
            self._set_added([])

    def _set_added(self, added) -> None:
        self._added, self._added_gen = added, self._added_gen + 1
        if self._added_handle is not None:
            self._added_handle.close()
        self._added_handle = None

    def _added_patterns(self) -> N.AddedPatterns:
        """the device handle of the list's patterns, content.lower() as UTF-8, built on first use"""
        self._refuse_added()
        if self._added_handle is None:
            self._added_handle = N.AddedPatterns([content.lower().encode("utf-8") for content, _ in self._added])
        return self._added_handle

    def _refuse_added(self) -> None:
        """a class that cannot take added tokens over its present vocabulary raises ValueError here (FastWP)"""

    def mask_id(self) -> int:
        """The dense id of "[MASK]": its index where the vocabulary holds the string, else len(vocab_list()), one past the end,
        so that no other dense id moves.  An embedding table needs max(len(vocab_list()), mask_id() + 1) rows."""
        return int(self._batch_vocabulary().mask_id)

    def mask_tokens(self, input_ids, probability: float = 0.15, whole_word: bool = True, seed: int = 0, epoch: int = 0,
                    mask_share: float = 0.8, random_share: float = 0.1, return_selected: bool = False) -> dict:
        """Rows of dense ids (any "input_ids" of encode_batch) masked for the masked-LM objective, on the device (swt_mlm_mask).
        A word -- a token and the '##' tokens after it; with whole_word=False every token by itself -- is selected with
        `probability`; of the selected tokens a mask_share becomes mask_id(), a random_share a random token of the vocabulary
        that is no special, the rest stay.  [PAD], [UNK], [CLS], [SEP] and [MASK] are never selected.  The draws are
        Philox4x32-10 by (seed, epoch, row, column): the same call gives the same masks whatever the batch around a row, a
        new epoch new ones over the same rows.
        input_ids: a 2-D C-contiguous int32 or int64 NumPy array, or such a torch tensor on the GPU (masked on the current
        stream, the ids never leaving the device); anything else raises TypeError.
        -> {"input_ids", "labels" (the id before masking on selected columns, -100 elsewhere), with return_selected "selected"
        (uint8), "n_eligible", "n_selected", "n_masked", "n_random", "n_kept"}.  ValueError: a probability or share outside
        [0, 1], mask_share + random_share > 1, a seed outside [0, 2^64) or an epoch outside [0, 2^32)."""
        return batching.mask_tokens(self, input_ids, probability, whole_word, seed, epoch, mask_share, random_share, return_selected)

    # -- fine-tuning labels (not in the reference; batching.py).  They read a batch and no encoder state.
    def align_word_labels(self, batch: dict, word_labels, label_all_tokens: bool = False, inside=None, side: Optional[int] = None,
                          ignore_index: int = -100) -> dict:
        """The labels of a token-classification task (NER, POS) on the rows of `batch`, a result of
        encode_batch(..., return_offsets=True), on the device (swt_label_words).  word_labels: a list of int lists, one per text
        and one label per word of it (the words of pre_tokenize, which "word_ids" count), or (values, offsets) arrays.  The
        first token of a word in its row takes the word's label -- a word cut by a window's edge is labelled again in the next
        window --, every other token ignore_index, or with label_all_tokens the label too; where `inside` is given, such a token
        takes inside[label] for 0 <= label < len(inside): the B-x to I-x map of BIO tagging.  Specials, padding and the other
        side of a pair get ignore_index.  side: whose words the labels are, 0 or 1; required for pair rows.
        batch: NumPy arrays, or torch tensors on the GPU (labelled on the current stream, nothing leaving the device but the
        counts); anything else raises TypeError.  A packed batch has no word_ids: ValueError.
        -> {"labels" [rows, width] of the dtype of input_ids, "n_labelled", "n_continuation": the tokens left at ignore_index as
        no first token}.  ValueError, naming the first such row and its text: a row that names a word beyond its text's labels."""
        return batching.align_word_labels(batch, word_labels, label_all_tokens, inside, side, ignore_index)

    def answer_positions(self, batch: dict, answers, side: Optional[int] = None, texts: Optional[List[str]] = None,
                         ignore_index: int = -100) -> dict:
        """The start and end columns of an extractive-QA answer in every row of `batch`, a result of
        encode_batch(..., return_offsets=True), on the device (swt_answer_positions).  answers: [n_texts, 2], the (start, end)
        of each text's answer, None or (-1, -1) for none, in the unit of "offset_mapping" -- code points of text.lower().  With
        texts, the original strings of that side, the positions are indices into the original string: where
        len(t.lower()) != len(t) ("İ") they are mapped on the host by the running sum of len(ch.lower()).  side: where the
        answer lies, 1 (the context) by default for pair rows.
        A row holds the answer when its first token of that side starts at or before it and its last ends at or behind it: then
        the start position is the last token that starts at or before the answer's start, the end position the first that ends
        at or behind its end.  Every other row gets the [CLS] column twice when the rows have specials (wherever the padding
        is), ignore_index when not.  The usual recipe lets its first scan run on into [SEP] and the padding when the answer
        starts in a window's last token; this does not.
        -> {"start_positions", "end_positions" [rows] of the dtype of input_ids, "has_answer" uint8[rows],
        "sample_has_answer_row" uint8[n_texts], "n_with", "n_without"}.  TypeError and ValueError as align_word_labels."""
        return batching.answer_positions(batch, answers, side, texts, ignore_index)

    def best_answers(self, batch: dict, start_logits, end_logits, max_answer_length: int = 30, side: Optional[int] = None,
                     texts: Optional[List[str]] = None) -> dict:
        """One best answer span per text from a QA model's start and end logits ([rows, width], float32, NumPy or torch on the
        GPU as `batch` is; another dtype raises TypeError) over the rows of `batch`, on the device (swt_answer_best).  A span is
        a pair of token columns (i, j) of that side in one row, i <= j < i + max_answer_length; its score start_logits[i] +
        end_logits[j] in float32; a NaN score is no span.  The best: higher score, then smaller i, then smaller j, and between
        the windows of a text the earlier row.
        -> per text {"score" (-inf without a span), "null_score" (the least [CLS] score of the text's rows when the rows have
        specials, +inf when not), "row", "start_col", "end_col" (-1 without a span), "char_start", "char_end" (the span in
        "offset_mapping"'s unit)}, and with texts "text": texts[i].lower()[char_start:char_end], sliced on the host."""
        return batching.best_answers(batch, start_logits, end_logits, max_answer_length, side, texts)

    # -- token-classification inference (not in the reference; batching.py)
    def word_predictions(self, batch: dict, logits, strategy: str = "first", side: Optional[int] = None, return_logits: bool = False,
                         n_texts: Optional[int] = None) -> dict:
        """One label and softmax score per word of every text from a token-classification model's logits ([rows, width,
        n_labels], float32, NumPy or torch on the GPU as `batch` is; another dtype or kind raises TypeError, another shape
        ValueError) over the rows of `batch`, a result of encode_batch(..., return_offsets=True), on the device (swt_word_plan,
        swt_word_predict): the way back from align_word_labels.  A word's tokens in a row are a run of columns; where a word
        shows up in several overlapping windows, the run with the most context speaks for it -- min(tokens to its left, tokens
        to its right) in its row, then the earlier row --, so that a word cut by a window's edge is read from its whole copy.
        strategy: "first" takes the logits of the run's first token, "mean" their float32 mean over the run in column order,
        "max" their maximum.  The label is the first argmax, the score its softmax probability.  side: whose words, 0 or 1;
        required for pair rows.  n_texts: the texts of the batch; by default one per row, or with windows the last row's + 1.
        -> {"word_offsets" uint64[n_texts + 1]: the words of text s are [word_offsets[s], word_offsets[s + 1]); per word "label"
        (-1 for a word no row holds), "score", "row", "col", "n_tokens" (where the run lies; -1), "char_start", "char_end" (the
        word in "offset_mapping"'s unit); "n_words": the words with a run, "n_missing": those without}, and with return_logits
        "logits" [words, n_labels], the word's vector.  A packed batch raises ValueError.  With torch tensors everything stays
        on the device and the current stream; the word total and the counts are read back."""
        return batching.word_predictions(batch, logits, strategy, side, return_logits, n_texts)

    def entities(self, words: dict, id2label, texts: Optional[List[str]] = None) -> dict:
        """The words of word_predictions grouped into entities on the device (swt_entity_spans).  id2label: the label names by
        id, as "O", "B-PER", "I-PER": "B-x" and "I-x" are of type x, "O" is outside, any other name is a type of its own that
        never begins.  A word heads an entity when it has a type and is its text's first word, follows a word of another type
        (or none), or its label begins; the entity runs on over the words of the same type that head none.
        -> per entity, in order, {"text_index", "type" (an index into "type_names"), "first_word", "last_word" (in the text),
        "char_start", "char_end", "score": the float32 mean of the words' scores}, "type_names", "n_entities",
        "n_entity_words", and with texts (one string per text) "text": texts[i].lower()[char_start:char_end], sliced on the host."""
        return batching.entities(words, id2label, texts)

    # -- masked-LM inference (not in the reference; batching.py)
    def fill_mask(self, input_ids, logits, top_k: int = 5, tokens: bool = False) -> dict:
        """The top_k best tokens of every [MASK] column -- input_ids == mask_id() -- from a masked-LM's logits ([rows, width, V],
        float32), on the device (swt_mlm_positions, swt_mlm_predict), which reads the logits of those columns and of no other
        and makes no copy of them.  The order: the greater logit, then the smaller id; a NaN logit is no candidate.
        input_ids: a 2-D C-contiguous int32 or int64 NumPy array, or such a torch tensor on the GPU, and C-contiguous logits of
        the same kind (then everything stays on the device and the current stream; the number of columns and the counts are
        read back); logits that are not float32 or not of that kind raise TypeError; a shape other than [rows, width, V],
        logits that are not contiguous or a top_k outside 1 .. 64 ValueError.
        -> per [MASK] column, in row-major order, {"row", "col", "token_ids" [n, top_k] (-1 where the row has fewer entries
        that are no NaN), "logit", "logprob" (logit - the row's log-sum-exp), "score" (exp(logprob)), "lse"}, "n_positions",
        and with tokens=True "tokens": per column a list of vocab_list() strings made on the host, "[MASK]" for mask_id() past
        the list's end and None for -1."""
        return batching.fill_mask(self, input_ids, logits, top_k, tokens)

    def mlm_scores(self, logits, labels, top_k: int = 1) -> dict:
        """A masked-LM's logits ([rows, width, V], float32) scored against `labels` of encode_batch(..., mlm=...) or mask_tokens
        at the columns with labels != -100, on the device (swt_mlm_positions, swt_mlm_predict).  Kinds, TypeError and
        ValueError as fill_mask.
        -> per such column {"row", "col", "label" (-1 for a label outside [0, V)), "label_logprob", "label_rank" (the entries
        that come before the label's: 0 for the argmax; -1 for a label out of range or with a NaN logit), "lse", and the top_k
        as fill_mask gives them}; "loss": the mean of -label_logprob over the labels in range, "perplexity" = exp(loss),
        "accuracy" and "accuracy_at_k" over all columns, "n_positions", "n_correct", "n_correct_at_k", "n_nan" (columns whose
        logits hold a NaN), "n_out_of_range"."""
        return batching.mlm_scores(logits, labels, top_k)

    def decode_batch_bytes(self, input_ids, attention_mask=None, skip_special_tokens: bool = True):
        """Rows of dense ids (any "input_ids" of encode_batch or mask_tokens, a model's output) back to text on the device
        (swt_decode_plan / swt_decode_rows), as the reference's recover_sentence (utils.py:141-154) spells the rows' tokens: '##'
        tokens glued to what precedes them, no space before . , ) ] \\ ’ - ' / nor after ( [ \\ ’ - ' /, one space elsewhere.
        A column is kept where attention_mask (if given) is nonzero and, with skip_special_tokens, its id is not [PAD], [CLS],
        [SEP] or mask_id(); [UNK] stands for a word of the text and is spelled "[UNK]" (WordPiece's "['UNK']" has the same
        dense id and comes back as "[UNK]" too).  Like the reference this does not restore the text: whitespace and case are gone.
        input_ids: a 2-D C-contiguous int32 or int64 NumPy array, or such a torch tensor on the GPU (decoded on the current
        stream, the ids never leaving the device; the byte count is the one read-back); anything else raises TypeError.
        -> (text uint8, offsets uint64[rows + 1]): row r is text[offsets[r]:offsets[r + 1]], UTF-8, no terminator.
        ValueError, naming the first such row: a kept id outside the vocabulary, or a kept token that is empty or holds
        whitespace (its spelling under the reference's regular expressions is not guessed)."""
        return batching.decode_batch_bytes(self, input_ids, attention_mask, skip_special_tokens)

    def decode_batch(self, input_ids, attention_mask=None, skip_special_tokens: bool = True) -> List[str]:
        """decode_batch_bytes as one str per row"""
        return batching.decode_batch(self, input_ids, attention_mask, skip_special_tokens)

    def decode(self, ids, skip_special_tokens: bool = True) -> str:
        """one sequence of dense ids (a list, a 1-D array or tensor) -> its text, as decode_batch"""
        if not hasattr(ids, "dim"):  # no torch tensor
            ids = np.asarray(ids)
            if ids.ndim != 1 or (ids.size and ids.dtype.kind not in "iu"):
                raise TypeError("ids: one sequence of integers")
            ids = np.ascontiguousarray(ids if ids.dtype in (np.int32, np.int64) else ids.astype(np.int64))
        elif ids.dim() != 1:
            raise TypeError("ids: one sequence of integers")
        if len(ids) == 0:
            return ""
        return batching.decode_batch(self, ids.reshape(1, -1), None, skip_special_tokens)[0]

    def _batch_vocabulary(self):
        return self._enc.vocabulary()

    def _batch_encode_ids(self, texts, dropout=None):
        return self.encode_ids_batch(texts) if dropout is None else _encode_ids(self._enc, texts, dropout)

    def _batch_encode_spans(self, texts, dropout=None):
        return self.encode_spans_batch(texts) if dropout is None else _encode_spans(self._enc, texts, dropout)

    def _batch_encode_spans_packed(self, text, off, texts, dropout=None):
        """_batch_encode_spans over a packed, lowercased text the caller has made (and may have blanked); texts: for the errors"""
        return _encode_spans_packed(self._enc, text, off, texts, self._enc.draw(dropout))

    def _batch_encode_dev(self, *args, dropout=None):
        return _encode_dev(self._enc, *args, dropout=dropout)


_CLS_CACHE: Dict[str, int] = {}


def _class_of(ch: str) -> int:
    c = _CLS_CACHE.get(ch)
    if c is None:
        c = _CLS_CACHE[ch] = N.class_of(ord(ch))
    return c


# ------------------------------------------------------------------------------------------------------
# BPE

class _SymbolTable:
    """Symbol string <-> id, by STRING identity (bpe.py:41,103,227): one code point -> its ordinal, anything
    else -> 0x110000 + k in order of first appearance."""

    def __init__(self):
        self.strings: List[str] = []
        self.index: Dict[str, int] = {}

    def intern(self, s: str) -> int:
        if len(s) == 1:
            return ord(s)
        k = self.index.get(s)
        if k is None:
            k = self.index[s] = len(self.strings)
            self.strings.append(s)
        return N.SYM_BASE + k

    def string(self, sid: int) -> str:
        sid &= 0x7FFFFFFF
        return chr(sid) if sid < N.SYM_BASE else self.strings[sid - N.SYM_BASE]


def _raise_span_mismatch(status: int, i: int, text: str) -> None:
    raise RuntimeError("token spans: the tokens of text %d do not tile it (a bug in this library)" % i)


_PLAIN_INTERN = _SymbolTable.intern  # (a test swaps intern() for another to force the collision replay: then the Python loop runs)


# ------------------------------------------------------------------------------------------------------
# The batch calls: one body per operation, written against what a class says about its encoder

class _Encoder:
    """What the batch calls of one tokenizer class differ in (the Python side of csrc/swt_tile.h's HostEncoder).  A tokenizer
    makes one in __init__ and keeps it as `_enc`.  The record owns nothing but its caches: the handle and what spells its ids
    stay the tokenizer's attributes, read by name every time, and are built, rebuilt and closed where they always were.

    ensure: the tokenizer's method that returns the live N.BpeTable / N.WpTrie; spelling: its attribute that spells the ids,
    a _SymbolTable (BPE) or the token list (WordPiece); naive: the `encode_naive*` entries instead of `encode*`; complain:
    what raises for a sentence's status (WordPiece; None: BPE, which has no statuses); corner: an id past "[UNK]" stands for
    the several tokens of encode_word("##") (FastWP); first: the handle is built before the items are looked at (FastBPE);
    dropout: the handle has the `encode_dropout*` entries, a third set beside the two (FastBPE); maxmatch: that third set is
    `encode_naive_dropout*`, MaxMatch-Dropout (NaiveWP).  Either way the set is reached through drop_host / drop_dev, and the
    argument travels through one channel: a `dropout=` dict as it is, a `maxmatch_dropout=` dict inside a batching.MaxMatch."""

    def __init__(self, tok, ensure, spelling, naive, error="Text to tokenize must be a string.", complain=None, corner=False,
                 first=False, dropout=False, maxmatch=False):
        self._tok, self._ensure, self._spelling = weakref.proxy(tok), ensure, spelling  # (no cycle: a tokenizer dies with its last name)
        self.host = "encode_naive" if naive else "encode"  # the three call forms on the handle, by name
        self.joined, self.dev = self.host + "_joined", self.host + "_dev"
        # BPE-dropout: a host and a `_dev` form, no joined one -- a word's draws go by its byte offset in pack_and_lower's text,
        # so every dropout call takes the long way
        self.drop_host, self.drop_dev = ("encode_dropout", "encode_dropout_dev") if dropout else (None, None)
        if maxmatch:  # MaxMatch-Dropout: the same two forms, for the same reason
            self.drop_host, self.drop_dev = self.host + "_dropout", self.host + "_dropout_dev"
        self.bpe_dropout, self.maxmatch = bool(dropout), bool(maxmatch)
        self.error, self.complain, self.corner, self.first = error, complain, corner, first
        self.flagged = complain is None  # BPE ids carry SWT_BPE_CONT over SYM_BASE + k; WordPiece ids index the token list
        self.len_base = N.SYM_BASE if self.flagged else 0
        self._cache: dict = {}

    def handle(self):
        return getattr(self._tok, self._ensure)()

    def spelling(self):
        """as the last handle() left it"""
        return getattr(self._tok, self._spelling)

    def draw(self, dropout):
        """a `dropout` argument -> None, or the (drop_below, seed, epoch) of this encoder's dropout entries; ValueError for an
        encoder that has none, and for arguments that give no draw (batching.dropout_draw)"""
        if dropout is None:
            return None
        if isinstance(dropout, batching.MaxMatch):
            if not self.maxmatch:
                raise ValueError("maxmatch_dropout: only NaiveWP drops matches (MaxMatch-Dropout); this tokenizer takes "
                                 "maxmatch_dropout=None")
            return batching.dropout_draw(dropout.spec, "maxmatch_dropout")
        if not self.bpe_dropout:
            raise ValueError("dropout: only FastBPE drops merges (BPE-dropout); this tokenizer takes dropout=None")
        return batching.dropout_draw(dropout)

    def channel(self, dropout, maxmatch_dropout):
        """the two keywords of the public calls -> what travels on as `dropout`.  Both given: whichever this class does not have
        raises, and no class has both."""
        if maxmatch_dropout is None:
            return dropout
        self.draw(dropout)
        return batching.MaxMatch(maxmatch_dropout)

    def names(self) -> List[str]:
        """WordPiece: the token of every id below the corner's"""
        return self.spelling() + ["['UNK']", "[UNK]"]

    def id_cap(self) -> int:
        """one past the largest id (without SWT_BPE_CONT) an encode can return"""
        sp = self.spelling()
        return N.SYM_BASE + len(sp.strings) + 1 if self.flagged else len(sp) + 2 + self.corner

    def _cached(self, what, make, spelling=None, *more):
        """make(spelling) once per spelling object and its length: a rebuilt handle comes with a new one"""
        sp = self.spelling() if spelling is None else spelling
        key = (len(sp.strings) if self.flagged else len(sp),) + more
        hit = self._cache.get(what)
        if hit is None or hit[0] is not sp or hit[1] != key:
            hit = self._cache[what] = (sp, key, make(sp))
        return hit[2]

    def lengths(self, spelling=None) -> np.ndarray:
        """the length table of swt_token_spans for ids spelled by `spelling` (None: this encoder's own)"""
        return self._cached("lengths", (lambda sp: N.bpe_length_table(sp.strings)) if self.flagged else N.wp_length_table, spelling)

    def vocabulary(self):
        """the dense ids of batching.py over the live handle's ids, the added tokens behind them"""
        self.handle()
        if not self.flagged:
            base = self._cached("base_vocabulary", batching.wp_vocabulary)
        else:
            merges = self._tok.merges_list
            base = self._cached("base_vocabulary", lambda sp: batching.bpe_vocabulary(merges, sp), None, len(merges))
        added = self._tok._added
        if not added:
            return base
        return self._cached("vocabulary", lambda sp: batching.with_added(base, added), None, id(base), self._tok._added_gen)


def _raise_flagged(enc: _Encoder, status, texts) -> None:
    """what tokenize() raises for the first text with a status; a status FastWP's complain does not know passes"""
    for i in np.flatnonzero(status):
        enc.complain(int(status[i]), texts[int(i)])


def _encode_ids(enc: _Encoder, texts, dropout=None):
    """encode_ids_batch of every class: the argument checks in the class's order, then the route -- past 64 texts the joined
    call (strings -> joined bytes -> ids: the device splits, lowercases (utils.py:27) and encodes, the prepared
    text never comes back); texts with U+0000 inside, or that only str.lower() lowercases, and small batches go the long way.
    dropout (FastBPE; None: everything above, untouched): BPE-dropout through the encoder's dropout entry, always the long way."""
    draw = enc.draw(dropout)
    if not isinstance(texts, list):
        raise TypeError(enc.error)
    if enc.first:
        handle = enc.handle()
    few = len(texts) <= 64  # past that join_texts raises for an item that is no str, on its way through them
    if few and not all(isinstance(t, str) for t in texts):
        raise TypeError(enc.error)
    if not enc.first:
        try:
            handle = enc.handle()
        except AttributeError:  # FastWP before load/train, as the reference: but the argument's TypeError goes first
            if not all(isinstance(t, str) for t in texts):
                raise TypeError(enc.error) from None
            raise
    if not few:
        joined, n_nul = N.join_texts(texts, enc.error)
        if draw is None and n_nul == 0 and joined.size + 1 != len(texts) and N.device_lower_ok():
            got = getattr(handle, enc.joined)(joined, len(texts))
            if got is not None:
                return got
    text, off = N.pack_and_lower(texts)  # utils.py:27 / wordpiece.py:248 lower()
    if draw is not None:
        return getattr(handle, enc.drop_host)(text, off, draw)
    return getattr(handle, enc.host)(text, off)


def _bpe_tokens(enc: _Encoder, ids, off=None):
    """BPE ids -> their token strings, one list per sentence of `off` (None: one flat list)"""
    st = enc.spelling()
    ids = np.asarray(ids, dtype=np.uint32)
    if ids.size < 4096:
        toks = [("##" + st.string(t)) if t & N.BPE_CONT else st.string(t) for t in map(int, ids)]
        return toks if off is None else [toks[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]
    # large outputs: spell each DISTINCT id once (found by a presence map over the id space, not a sort), then hand out references
    # (the per-token Python loop was 1.5 s per 2 M tokens)
    key = (ids << np.uint32(1)) | (ids >> np.uint32(31))  # symbol * 2 + the BPE_CONT bit
    spell = lambda k: ("##" + st.string(k >> 1)) if k & 1 else st.string(k >> 1)
    cap = 2 * (N.SYM_BASE + len(st.strings))
    if off is None:
        return N.nested_lists_by_key(key, cap, spell, np.array([0, ids.size], dtype=np.uint64))[0]
    return N.nested_lists_by_key(key, cap, spell, off)


def _encode_spans(enc: _Encoder, texts, dropout=None):
    """encode_spans_batch by tiling (NaiveBPE, FastBPE, NaiveWP): the host encode's results with (spans, word ids) behind them.
    The text is packed once and sent to the device twice, for the encode and for swt_token_spans.  dropout: as _encode_ids --
    any segmentation of a word tiles it, so the spans need nothing more."""
    draw = enc.draw(dropout)
    if not isinstance(texts, list) or not all(isinstance(t, str) for t in texts):
        raise TypeError("Text to tokenize must be a string.")
    return _encode_spans_packed(enc, *N.pack_and_lower(texts), texts, draw)


def _encode_spans_packed(enc: _Encoder, text, off, texts, draw=None):
    """_encode_spans from the packed text on: `text` is lowercased UTF-8, `off` its offsets, `texts` what the errors quote"""
    handle = enc.handle()
    got = getattr(handle, enc.host)(text, off) if draw is None else getattr(handle, enc.drop_host)(text, off, draw)
    if enc.complain is not None:
        _raise_flagged(enc, got[2], texts)
    spans, word, status = N.token_spans(text, off, got[0], got[1], enc.lengths(), enc.len_base, enc.flagged)
    if status.any():
        _raise_span_mismatch(1, int(np.flatnonzero(status)[0]), "")
    return got + (spans, word)


def _encode_dev(enc: _Encoder, d_text, n_bytes, d_off, n_sent, d_ids, d_tok_off, d_ntok, d_spans, d_word, stream, empty, dropout=None):
    """the `_dev` encode on the caller's torch buffers (dropout: its dropout form), then swt_token_spans_dev when spans are wanted
    -> [(status tensor, what to raise for a status)]"""
    import torch
    draw = enc.draw(dropout)
    call, checks = getattr(enc.handle(), enc.dev), []
    if enc.complain is None:
        if draw is not None:
            getattr(enc.handle(), enc.drop_dev)(d_text, n_bytes, d_off, n_sent, d_ids, d_tok_off, d_ntok, draw, 0, stream)
        else:
            call(d_text, n_bytes, d_off, n_sent, d_ids, d_tok_off, d_ntok, 0, stream)
    else:
        d_status = empty(n_sent + 8, torch.uint8)
        if draw is not None:
            getattr(enc.handle(), enc.drop_dev)(d_text, n_bytes, d_off, n_sent, d_ids, d_tok_off, d_status.data_ptr(), d_ntok, draw, stream)
        else:
            call(d_text, n_bytes, d_off, n_sent, d_ids, d_tok_off, d_status.data_ptr(), d_ntok, stream)
        checks.append((d_status, lambda st, i, text: enc.complain(st, text)))
    if d_spans is not None:
        lengths = enc.lengths()
        d_len = empty(lengths.size + 4, torch.int32)
        d_len[:lengths.size].copy_(torch.from_numpy(lengths.view(np.int32)))
        d_span_status = empty(n_sent + 8, torch.uint8)
        N.check(N.lib().swt_token_spans_dev(d_text, n_bytes, d_off, n_sent, d_ids, d_tok_off, d_len.data_ptr(), enc.len_base,
                                            int(lengths.size), int(enc.flagged), N.SPAN_CODEPOINTS, d_spans, d_word,
                                            d_span_status.data_ptr(), stream))
        checks.append((d_span_status, _raise_span_mismatch))
    return checks


class NaiveBPE(SubwordTokenizer):
    """Byte-Pair Encoding (bpe.py:9-189).  `train` runs on the device; `encode_word`/`tokenize` keep the
    reference's didactic O(merges x length) loop in Python (out of the GPU scope);
    `encode_ids_batch`/`tokenize_batch` run the same loop -- the merges in LIST order -- on the device (swt_bpe_encode_naive)."""

    def __init__(self, tokenizer=None) -> None:
        super().__init__(tokenizer)
        self.merges_list: List[Tuple[str, str]] = []
        self.vocab: set = set()
        self._trainer: Optional[N.BpeTrainer] = None
        self._train_syms: Optional[_SymbolTable] = None
        self._train_ids = None  # (left, right, merged) ids of merges_list as the device named them, when no replay was needed
        self._corpus_cache = None
        self._naive_table: Optional[N.BpeTable] = None  # built from merges_list on the first batch call
        self._naive_syms = _SymbolTable()
        self._naive_merges: Optional[list] = None  # the list the handle was built from
        self._train_merges: Optional[list] = None  # the merges _train_ids name (merges_list itself may be changed later)
        self._enc = _Encoder(self, "_ensure_naive_table", "_naive_syms", naive=True)

    # -- bpe.py:25-48
    def _replace_pair(self, pair: Tuple[str, str], word: List[str]) -> List[str]:
        left, right = pair
        joined = left + right
        out: List[str] = []
        k, n = 0, len(word)
        while k < n:
            if k + 1 < n and word[k] == left and word[k + 1] == right:
                out.append(joined)
                k += 2
            else:
                out.append(word[k])
                k += 1
        return out

    # -- bpe.py:50-112: the merge loop, on the device
    def train(self, corpus: List[str], max_vocab: int = 30_000) -> None:
        if not isinstance(corpus, list):
            raise TypeError("Corpus must be a list of strings.")
        joined = None
        if len(corpus) > 64:
            joined = N.join_texts(corpus, "Corpus must be a list of strings.")  # checks the items on its way through them
        elif not all(isinstance(example, str) for example in corpus):
            raise TypeError("Corpus must be a list of strings.")
        if not isinstance(max_vocab, int):
            raise TypeError("Maximum vocabulary size must be an integer.")
        self.reset()
        text = off = None
        trainer = N.BpeTrainer.from_texts(corpus, joined)  # bpe.py:70-81 (lower, split, Counter, symbolise), the text staying on the device
        if trainer is None:
            text, off = N.pack_and_lower(corpus)
            trainer = N.BpeTrainer.from_text(text, off)
        syms = _SymbolTable()
        self.vocab.update(chr(int(c)) for c in trainer.base_symbols())  # bpe.py:75
        applied_l: List[int] = []  # (left, right, merged) ids of every merge so far, for the collision replay
        applied_r: List[int] = []
        applied_m: List[int] = []
        done = set()  # left << 32 | right of every merge so far
        exhausted = False
        runs, clean = [], True  # the id arrays of every device run, as long as no string collision forced a replay
        while len(self.vocab) < max_vocab and not exhausted:  # bpe.py:88
            # The device runs `want` iterations of bpe.py:90-111 back to back; it names the merged symbol of step i
            # SYM_BASE + (strings so far) + i, which is right as long as every merged string is new (bpe.py:103).
            want = max_vocab - len(self.vocab)
            first = N.SYM_BASE + len(syms.strings)
            lefts, rights, counts = trainer.run(want, first)
            if len(lefts) < want:
                exhausted = True  # bpe.py:98-99: no pair left
            runs.append((lefts, rights, first))
            # (plain Python ints and local names: this loop runs once per merge, beside a device that needs ~10 us for one;
            # what can be done for the whole run at once -- the replay record, the "never twice" check -- is done after it)
            strings, intern, base = syms.strings, syms.intern, N.SYM_BASE
            vocab_add, merges_append = self.vocab.add, self.merges_list.append
            ll, rl = lefts.tolist(), rights.tolist()
            taken, collided = len(ll), None
            host = N.pyhost() if _SymbolTable.intern is _PLAIN_INTERN and "intern" not in vars(syms) else None
            if host is not None:  # the same loop in C (csrc/swt_pyhost.c), unless someone has put another intern() in place
                la, ra = np.ascontiguousarray(lefts, dtype=np.uint32), np.ascontiguousarray(rights, dtype=np.uint32)
                hit = C.c_uint32()
                at = host.swt_py_bpe_merge_strings(la.ctypes.data, ra.ctypes.data, len(ll), base, first, strings, syms.index, self.vocab,
                                                   self.merges_list, C.byref(hit))
                if at >= 0:
                    taken, collided = at + 1, int(hit.value)
            for i, (left, right) in enumerate(zip(ll, rl) if host is None else ()):
                ls = chr(left) if left < base else strings[left - base]   # _SymbolTable.string
                rs = chr(right) if right < base else strings[right - base]
                joined = ls + rs
                merged = intern(joined)
                vocab_add(joined)  # bpe.py:103
                merges_append((ls, rs))  # bpe.py:104
                if merged != first + i:
                    taken, collided = i + 1, merged
                    break
            keys = ((lefts[:taken].astype(np.uint64) << np.uint64(32)) | rights[:taken].astype(np.uint64)).tolist()
            fresh = set(keys)
            if len(fresh) != len(keys) or not done.isdisjoint(fresh):  # symbols only ever merge: a merged pair cannot come back
                raise RuntimeError("pair histogram inconsistent: a pair was selected twice")
            done |= fresh
            applied_l.extend(ll[:taken])
            applied_r.extend(rl[:taken])
            applied_m.extend(range(first, first + taken))
            if collided is not None:
                # two different merges spelled the same string (never observed).  The device
                # continued with a fresh id; rebuild the state with the right one and carry on from here.
                applied_m[-1] = collided
                clean = False
                trainer.close()
                if text is None:
                    text, off = N.pack_and_lower(corpus)
                trainer = N.BpeTrainer.from_text(text, off)
                for l_, r_, m_ in zip(applied_l, applied_r, applied_m):
                    trainer.apply(l_, r_, m_)
                exhausted = False
        self._trainer, self._train_syms, self._corpus_cache = trainer, syms, None
        self._train_merges = list(self.merges_list)
        if clean:
            self._train_ids = (np.concatenate([l for l, _, _ in runs]) if runs else np.zeros(0, np.uint32),
                               np.concatenate([r for _, r, _ in runs]) if runs else np.zeros(0, np.uint32),
                               np.concatenate([f + np.arange(len(l), dtype=np.uint32) for l, _, f in runs]) if runs else np.zeros(0, np.uint32))

    @property
    def corpus_as_symbols(self) -> List[Tuple[List[str], int]]:
        """bpe.py:23,108-111: the unique words as symbol lists with their frequency (read back on demand)."""
        if self._trainer is None:
            return []
        if self._corpus_cache is None:
            ids, woff, freq = self._trainer.export()
            st = self._train_syms
            self._corpus_cache = ([st.string(int(x)) for x in ids], woff, freq)
        strs, woff, freq = self._corpus_cache
        return [(strs[int(woff[w]):int(woff[w + 1])], int(freq[w])) for w in range(len(woff) - 1)]

    # -- bpe.py:114-134
    def encode_word(self, word: str) -> List[str]:
        pieces = list(word)
        for pair in self.merges_list:
            pieces = self._replace_pair(pair, pieces)
        if len(pieces) > 1:
            pieces[1:] = ["##" + p for p in pieces[1:]]
        return pieces

    # -- bpe.py:136-158
    def tokenize(self, text: str) -> List[str]:
        if not isinstance(text, str):
            raise TypeError("Text to tokenize must be a string.")
        words = [w for w, _ in self.preprocessing([text])[0]]
        out: List[str] = []
        for w in words:
            out += self.encode_word(w)
        return out

    # -- batch entry points (not in the reference): tokenize() of every text on the device, the merges in list order
    def _drop_naive_table(self) -> None:
        if self._naive_table is not None:
            self._naive_table.close()
        self._naive_table, self._naive_syms, self._naive_merges = None, _SymbolTable(), None

    def _ensure_naive_table(self) -> N.BpeTable:
        # rebuilt when merges_list was assigned or changed in place since the last build (train/reset/load_resources drop it)
        if self._naive_table is None or self.merges_list != self._naive_merges:
            self._drop_naive_table()
            merges = [tuple(pair) for pair in self.merges_list]
            syms = _SymbolTable()
            if self._train_ids is not None and self._train_syms is not None and merges == self._train_merges:
                # the device named the symbols of the merges it chose exactly as the loop below would (FastBPE.train)
                syms.strings, syms.index = list(self._train_syms.strings), dict(self._train_syms.index)
                left, right, merged = self._train_ids
            else:
                intern = syms.intern  # the interning order of FastBPE._build_table
                ids = np.array([x for l, r in merges for x in (intern(l), intern(r), intern(l + r))], dtype=np.uint32).reshape(-1, 3)
                left, right, merged = ids[:, 0], ids[:, 1], ids[:, 2]
            self._naive_table, self._naive_syms, self._naive_merges = N.BpeTable(left, right, merged), syms, merges
        return self._naive_table

    def encode_ids_batch(self, texts: List[str], dropout: Optional[dict] = None,
                         maxmatch_dropout: Optional[dict] = None) -> Tuple[np.ndarray, np.ndarray]:
        """texts -> (token ids uint32, sentence offsets uint64[n+1]): tokenize() of every text; ids as defined in include/swt.h
        over this object's own symbol table (decode_ids spells them).  dropout: None; anything else is FastBPE's (ValueError).
        maxmatch_dropout: None; anything else is NaiveWP's (ValueError).  Added tokens (add_tokens) are not looked for here: only encode_batch honours them."""
        return _encode_ids(self._enc, texts, self._enc.channel(dropout, maxmatch_dropout))

    def decode_ids(self, ids) -> List[str]:
        return _bpe_tokens(self._enc, ids)

    def tokenize_batch(self, texts: List[str], dropout: Optional[dict] = None,
                       maxmatch_dropout: Optional[dict] = None) -> List[List[str]]:
        """[tokenize(t) for t in texts].  Added tokens (add_tokens) are not looked for here: only encode_batch honours them."""
        return _bpe_tokens(self._enc, *self.encode_ids_batch(texts, dropout, maxmatch_dropout))

    # -- token spans (not in the reference): preprocessing's (start, end) carried on from the words to their tokens
    def _span_parts(self):
        """-> (the host-buffer encode of this class, the symbol table its ids are spelled from)"""
        return getattr(self._enc.handle(), self._enc.host), self._enc.spelling()

    def _span_lengths(self, spelling=None) -> np.ndarray:
        return self._enc.lengths(spelling)

    def encode_spans_batch(self, texts: List[str]):
        """texts -> (ids, offsets, spans uint32[n, 2], word_ids uint32[n]): encode_ids_batch plus, per token, its (start, end) in
        code points of text.lower() -- preprocessing's convention (utils.py:27-29) -- and the index of its word in the sentence.
        The text is packed once and sent to the device twice, for the encode and for swt_token_spans.  Added tokens (add_tokens) are not looked for here: only encode_batch honours them."""
        return _encode_spans(self._enc, texts)

    def tokenize_with_offsets(self, text: str) -> List[Tuple[str, Tuple[int, int]]]:
        """[(token, (start, end)), ...]: tokenize(text) in the shape of one preprocessing row"""
        if not isinstance(text, str):
            raise TypeError("Text to tokenize must be a string.")
        ids, _, spans, _ = self.encode_spans_batch([text])
        return [(tok, (int(s), int(e))) for tok, (s, e) in zip(self.decode_ids(ids), spans.tolist())]

    # -- bpe.py:160-164
    def reset(self) -> None:
        self.merges_list.clear()
        self.vocab.clear()
        self._drop_naive_table()
        if self._trainer is not None:
            self._trainer.close()
        self._trainer, self._train_syms, self._corpus_cache = None, None, None
        self._train_ids = self._train_merges = None

    # -- bpe.py:167-189
    def save_resources(self, path: str) -> None:
        os.makedirs(path, exist_ok=True)
        with open(os.path.join(path, "merges.json"), "w", encoding="utf-8") as f:
            json.dump(self.merges_list, f, ensure_ascii=False)

    def load_resources(self, path: str) -> None:
        merges_file = os.path.join(path, "merges.json")
        if os.path.isfile(merges_file):  # a missing file is silently ignored (bpe.py:187)
            with open(merges_file, "r", encoding="utf-8") as f:
                self.merges_list = [tuple(pair) for pair in json.load(f)]
            self._drop_naive_table()


class FastBPE(NaiveBPE):
    """bpe.py:192-263 with the rank table and the encode loop on the device."""

    def __init__(self, tokenizer=None):
        super().__init__(tokenizer)
        self._bpe_ranks: Dict[Tuple[str, str], int] = {}
        self._table: Optional[N.BpeTable] = None
        self._syms = _SymbolTable()
        self._enc = _Encoder(self, "_ensure_table", "_syms", naive=False, error="Text must be a string.", first=True, dropout=True)

    def _build_table(self) -> None:
        # bpe.py:200 / :257
        self._bpe_ranks = {pair: i for i, pair in enumerate(self.merges_list)}
        syms = _SymbolTable()
        intern = syms.intern
        ids = [x for l, r in self.merges_list for x in (intern(l), intern(r), intern(l + r))]
        ids = np.array(ids, dtype=np.uint32).reshape(-1, 3)
        self._set_table(syms, ids[:, 0], ids[:, 1], ids[:, 2])

    def _set_table(self, syms, left, right, merged) -> None:
        if self._table is not None:
            self._table.close()
        self._syms = syms
        self._table = N.BpeTable(left, right, merged)

    def _ensure_table(self) -> N.BpeTable:
        # like _bpe_ranks, the table only changes in train()/load_resources() (bpe.py:200,257)
        if self._table is None:
            self._table = N.BpeTable([], [], [])
        return self._table

    def train(self, corpus: List[str], max_vocab: int = 30_000) -> None:
        super().train(corpus, max_vocab)
        if self._train_ids is None or len(self._train_ids[0]) != len(self.merges_list):
            self._build_table()
            return
        # the device named the symbols exactly as _build_table would (a merged string gets the next id the first time it is
        # spelled, and in training every merge spells a new one): its ids go to the rank table as they are
        self._bpe_ranks = {pair: i for i, pair in enumerate(self.merges_list)}
        syms = _SymbolTable()
        syms.strings = list(self._train_syms.strings)
        syms.index = dict(self._train_syms.index)
        self._set_table(syms, *self._train_ids)

    def _pairs(self, seq: List[str]) -> set:
        return {(seq[i], seq[i + 1]) for i in range(len(seq) - 1)}

    def decode_ids(self, ids) -> List[str]:
        return _bpe_tokens(self._enc, ids)

    # -- batch entry points (not in the reference); FastBPE's own, like the reference's methods of the same class
    def encode_ids_batch(self, texts: List[str], dropout: Optional[dict] = None,
                         maxmatch_dropout: Optional[dict] = None) -> Tuple[np.ndarray, np.ndarray]:
        """texts -> (token ids uint32, sentence offsets uint64[n+1]); ids as defined in include/swt.h.

        dropout = {"probability": p, "seed": 0, "epoch": 0}: BPE-dropout (Provilkov et al. 2020) on the device
        (swt_bpe_encode_dropout, where the rule stands in full).  At every merge step of a word each candidate merge is skipped
        with probability p, so a text gets another segmentation per (seed, epoch) -- and the same one for the same (seed, epoch,
        index in `texts`), whatever the other texts are.  The draws are Philox4x32-10, as mask_tokens'.  p = 0 is the plain
        encode, p = 1 leaves every word as its characters.  ValueError: a probability outside [0, 1] or a NaN, a seed outside
        [0, 2^64), an epoch outside [0, 2^32), an unknown key.  maxmatch_dropout: None; anything else is NaiveWP's (ValueError).
        Added tokens (add_tokens) are not looked for here: only encode_batch honours them."""
        return _encode_ids(self._enc, texts, self._enc.channel(dropout, maxmatch_dropout))

    def tokenize_batch(self, texts: List[str], dropout: Optional[dict] = None,
                       maxmatch_dropout: Optional[dict] = None) -> List[List[str]]:
        return _bpe_tokens(self._enc, *self.encode_ids_batch(texts, dropout, maxmatch_dropout))

    # -- bpe.py:205-243, one word = one device "sentence" with the pre-tokenizer split switched off
    def encode_word(self, word: str) -> List[str]:
        if word == "":
            return [""]  # bpe.py:207-208
        table = self._ensure_table()
        text, off = N.pack_utf8([word])
        ids, _ = table.encode(text, off, flags=N.BPE_RAW_WORDS)
        return self.decode_ids(ids)

    # -- bpe.py:245-249
    def tokenize(self, text: str, dropout: Optional[dict] = None, maxmatch_dropout: Optional[dict] = None) -> List[str]:
        if not isinstance(text, str):
            raise TypeError("Text must be a string.")
        return self.tokenize_batch([text], dropout, maxmatch_dropout)[0]

    # -- bpe.py:251-263
    def load_resources(self, path: str) -> None:
        super().load_resources(path)
        self._build_table()

    def save_resources(self, path: str) -> None:
        super().save_resources(path)


# ------------------------------------------------------------------------------------------------------
# WordPiece

class _WpSymbols:
    """WordPiece trainer symbol id <-> string: c -> ord(c); '##c' -> WP_CONT + ord(c); a merged string -> WP_MERGED_BASE + k
    in order of first appearance (symbols are identified by their STRING, wordpiece.py:95-96,121)."""

    def __init__(self):
        self.strings: List[str] = []
        self.index: Dict[str, int] = {}

    def intern_merged(self, s: str) -> int:
        k = self.index.get(s)
        if k is None:
            k = self.index[s] = len(self.strings)
            self.strings.append(s)
        return N.WP_MERGED_BASE + k

    def string(self, sid: int) -> str:
        if sid < N.WP_CONT:
            return chr(sid)
        if sid < N.WP_MERGED_BASE:
            return "##" + chr(sid - N.WP_CONT)
        return self.strings[sid - N.WP_MERGED_BASE]


class NaiveWP(SubwordTokenizer):
    """WordPiece by the likelihood score (wordpiece.py:8-208).  `train` runs on the device: the
    BPE trainer's stream, histogram and merge-apply with exact symbol frequencies and the score as the argmax key;
    `encode_word`/`tokenize` keep the reference's longest-prefix loop in Python; `encode_ids_batch`/`tokenize_batch` run the
    same loop on the device over the vocabulary's trie (swt_wp_encode_naive)."""

    def __init__(self, tokenizer=None):
        super().__init__(tokenizer)
        self.vocab: set = set()
        self._trainer: Optional[N.BpeTrainer] = None
        self._train_syms: Optional[_WpSymbols] = None
        self._corpus_cache = None
        self._naive_trie: Optional[N.WpTrie] = None  # built from sorted(vocab) on the first batch call
        self._naive_tokens: List[str] = []
        self._naive_vocab: Optional[frozenset] = None  # the vocabulary the handle was built from
        # (FastWP puts its own in `_enc`; the methods it inherits that answer with NaiveWP's tokens keep to `_naive_enc`)
        self._enc = self._naive_enc = _Encoder(self, "_ensure_naive_trie", "_naive_tokens", naive=True, complain=self._raise_naive_status,
                                                   maxmatch=True)

    # -- wordpiece.py:29-103: the merge loop, on the device
    def train(self, corpus, max_vocab: int = 30_000):
        if not isinstance(corpus, list):
            raise TypeError("corpus must be a list of strings.")
        joined = None
        if len(corpus) > 64:
            joined = N.join_texts(corpus, "corpus must be a list of strings.")  # checks the items on its way
        elif not all(isinstance(example, str) for example in corpus):
            raise TypeError("corpus must be a list of strings.")
        if not isinstance(max_vocab, int):
            raise TypeError("max_vocab must be an int.")
        self.reset()
        text = off = None
        # wordpiece.py:44-58 (lower, split, Counter, '##' symbols), the text staying on the device where it can
        trainer = N.BpeTrainer.from_texts(corpus, joined, wordpiece=True)
        if trainer is None:
            text, off = N.pack_and_lower(corpus)
            trainer = N.BpeTrainer.from_text_wordpiece(text, off)
        syms = _WpSymbols()
        self.vocab |= {syms.string(int(c)) for c in trainer.base_symbols()}  # wordpiece.py:62-63
        applied: List[Tuple[int, int, int]] = []
        done = set()
        exhausted = False
        while len(self.vocab) < max_vocab and not exhausted:  # wordpiece.py:69
            # `want` iterations of wordpiece.py:70-102 back to back on the device; step i merges into WP_MERGED_BASE +
            # (strings so far) + i, which is right as long as every merged string is new (wordpiece.py:96)
            want = max_vocab - len(self.vocab)
            first = N.WP_MERGED_BASE + len(syms.strings)
            lefts, rights, _scores = trainer.run(want, first)
            if len(lefts) < want:
                exhausted = True  # wordpiece.py:75-76: no pair left
            for i in range(len(lefts)):
                left, right = int(lefts[i]), int(rights[i])
                if (left, right) in done:
                    raise RuntimeError("pair histogram inconsistent: %r selected twice" % ((left, right),))
                done.add((left, right))
                token = syms.string(left) + syms.string(right)[2:]  # wordpiece.py:95
                merged = syms.intern_merged(token)
                self.vocab.add(token)  # wordpiece.py:96
                applied.append((left, right, merged))
                if merged != first + i:
                    # two different merges spelled the same string: the device went on with a fresh id; rebuild the state
                    # with the shared one and carry on from here
                    trainer.close()
                    if text is None:
                        text, off = N.pack_and_lower(corpus)
                    trainer = N.BpeTrainer.from_text_wordpiece(text, off)
                    for l_, r_, m_ in applied:
                        trainer.apply(l_, r_, m_)
                    exhausted = False
                    break
        self._trainer, self._train_syms, self._corpus_cache = trainer, syms, None
        self._merge_order = [(syms.string(l), syms.string(r)) for l, r, _ in applied]

    @property
    def corpus_as_symbols(self) -> List[Tuple[List[str], int]]:
        """wordpiece.py:27,99-102: the unique words as symbol lists with their frequency (read back on demand)."""
        if self._trainer is None:
            return []
        if self._corpus_cache is None:
            ids, woff, freq = self._trainer.export()
            st = self._train_syms
            self._corpus_cache = ([st.string(int(x)) for x in ids], woff, freq)
        strs, woff, freq = self._corpus_cache
        return [(strs[int(woff[w]):int(woff[w + 1])], int(freq[w])) for w in range(len(woff) - 1)]

    # -- wordpiece.py:105-130
    def _replace_pair(self, pair, word):
        left, right = pair
        joined = left + right[2:]
        out = []
        k, n = 0, len(word)
        while k < n:
            if k + 1 < n and word[k] == left and word[k + 1] == right:
                out.append(joined)
                k += 2
            else:
                out.append(word[k])
                k += 1
        return out

    # -- wordpiece.py:132-159 (longest prefix in vocab, '##' on the remainder)
    def encode_word(self, word):
        pieces = []
        while word:
            cut = len(word)
            while cut > 0 and word[:cut] not in self.vocab:
                cut -= 1
            if cut == 0:
                return ["[UNK]"]
            pieces.append(word[:cut])
            word = word[cut:]
            if word:
                word = "##" + word
        return pieces

    # -- wordpiece.py:161-181
    def tokenize(self, text, maxmatch_dropout: Optional[dict] = None):
        """maxmatch_dropout: as encode_ids_batch, on the device, `text` being sentence 0; None: the reference's walk, here.
        Added tokens (add_tokens) are not looked for here: only encode_batch honours them."""
        if not isinstance(text, str):
            raise TypeError("Text to tokenize must be a string.")
        if maxmatch_dropout is not None:
            return self.tokenize_batch([text], maxmatch_dropout=maxmatch_dropout)[0]
        out = []
        for w, _ in self.preprocessing([text])[0]:
            out.extend(self.encode_word(w))
        return out

    # -- batch entry points (not in the reference)
    def _drop_naive_trie(self) -> None:
        if self._naive_trie is not None:
            self._naive_trie.close()
        self._naive_trie, self._naive_tokens, self._naive_vocab = None, [], None

    def _ensure_naive_trie(self) -> N.WpTrie:
        # ids = position in the sorted vocabulary, as FastWP's; rebuilt when `vocab` was changed in place since the last build
        if self._naive_trie is None or self.vocab != self._naive_vocab:
            self._drop_naive_trie()
            self._naive_vocab = frozenset(self.vocab)
            self._naive_tokens = sorted(self._naive_vocab)
            self._naive_trie = N.WpTrie(self._naive_tokens)
        return self._naive_trie

    def encode_ids_batch(self, texts: List[str], dropout: Optional[dict] = None, maxmatch_dropout: Optional[dict] = None):
        """texts -> (ids uint32, offsets uint64[n+1], status uint8[n]): tokenize() of every text on the device.  ids index
        sorted(vocab); len(vocab) + 1 is "[UNK]"; status WP_NONTERMINATING marks a text on which the reference never returns.
        dropout: None; anything else is FastBPE's (ValueError).

        maxmatch_dropout = {"probability": p, "seed": 0, "epoch": 0}: MaxMatch-Dropout (Hiraoka 2022) on the device
        (swt_wp_encode_naive_dropout, where the rule stands in full).  In the longest-match search a vocabulary match of two or
        more characters of the word is thrown away with probability p, so the search falls back to a shorter piece and a text
        gets another segmentation per (seed, epoch) -- and the same one for the same (seed, epoch, index in `texts`), whatever
        the other texts are.  The draws are Philox4x32-10, as mask_tokens'.  p = 0 is the plain encode, p = 1 leaves every word
        as its characters where each is a token in its position.  A word whose every match is dropped or missing is "[UNK]", and
        the status of a text is that of the thinned walk: over an odd vocabulary it can depend on the draw.  Errors as dropout's.
        Added tokens (add_tokens) are not looked for here: only encode_batch honours them."""
        return _encode_ids(self._enc, texts, self._enc.channel(dropout, maxmatch_dropout))

    def tokenize_batch(self, texts: List[str], dropout: Optional[dict] = None, maxmatch_dropout: Optional[dict] = None) -> List[List[str]]:
        """[tokenize(t) for t in texts], except that a text on which the reference never returns raises RuntimeError (documented
        deviation: the reference hangs).  Added tokens (add_tokens) are not looked for here: only encode_batch honours them."""
        ids, off, status = self.encode_ids_batch(texts, dropout, maxmatch_dropout)
        _raise_flagged(self._enc, status, texts)
        return N.nested_lists(self._enc.names(), ids, off)

    # -- token spans (not in the reference): preprocessing's (start, end) carried on from the words to their tokens
    def _span_lengths(self, spelling=None) -> np.ndarray:
        return self._naive_enc.lengths(spelling)

    def encode_spans_batch(self, texts: List[str]):
        """texts -> (ids, offsets, status, spans uint32[n, 2], word_ids uint32[n]): encode_ids_batch plus, per token, its
        (start, end) in code points of text.lower() (utils.py:27-29; "[UNK]" spans its whole word) and the index of its word in
        the sentence.  A text on which the reference never returns raises as in tokenize_batch.  The text is packed once and sent
        to the device twice, for the encode and for swt_token_spans.  FastWP inherits this method unchanged: called on a FastWP
        it answers with NaiveWP's tokens over the same vocabulary; FastWP's own tokens come from fast_encode_spans_batch.
        Added tokens (add_tokens) are not looked for here: only encode_batch honours them."""
        return _encode_spans(self._naive_enc, texts)

    def tokenize_with_offsets(self, text: str) -> List[Tuple[str, Tuple[int, int]]]:
        """[(token, (start, end)), ...]: NaiveWP.tokenize(text) in the shape of one preprocessing row (on a FastWP too, which
        inherits it: FastWP.tokenize with offsets is fast_tokenize_with_offsets)"""
        if not isinstance(text, str):
            raise TypeError("Text to tokenize must be a string.")
        ids, _, _, spans, _ = self.encode_spans_batch([text])
        names = self._naive_enc.names()
        return [(names[i], (int(s), int(e))) for i, (s, e) in zip(ids.tolist(), spans.tolist())]

    @staticmethod
    def _raise_naive_status(st: int, text: str) -> None:
        raise RuntimeError("NaiveWP.tokenize: the reference does not terminate on this input (status %d): %r" % (st, text[:80]))

    # -- wordpiece.py:183-208
    def reset(self) -> None:
        self.vocab.clear()
        self._drop_naive_trie()
        if self._trainer is not None:
            self._trainer.close()
        self._trainer, self._train_syms, self._corpus_cache = None, None, None

    def save_resources(self, path: str) -> None:
        os.makedirs(path, exist_ok=True)
        with open(os.path.join(path, "vocab.json"), "w", encoding="utf-8") as f:
            json.dump(list(self.vocab), f, ensure_ascii=False)

    def load_resources(self, path: str) -> None:
        vocab_file = os.path.join(path, "vocab.json")
        if os.path.isfile(vocab_file):
            with open(vocab_file, "r", encoding="utf-8") as f:
                self.vocab = set(json.load(f))
            self._drop_naive_trie()


class TrieNodeView:
    """Read-only view of one node of the flattened trie (utils.py:44-63 attribute names)."""

    def __init__(self, trie: "TrieView", node_id: int, path: Optional[str]):
        self._trie, self.node_id, self.chars_seen = trie, node_id, path

    def _info(self):
        return self._trie._native.node(self.chars_seen)

    @property
    def char(self):
        return self.chars_seen[-1:] if self.chars_seen else ""

    @property
    def is_end(self):
        return False if self.node_id == 1 else self._info()[2]

    @property
    def failure_link(self):
        if self.node_id == 1:
            return None
        link = self._info()[1]
        return None if link < 0 else self._trie.node_by_id(link)

    @property
    def failure_pops(self):
        if self.node_id == 1:
            return []
        return self._trie._decode(self._info()[3])

    def child(self, ch: str):
        if self.node_id == 1:
            return None
        info = self._trie._native.node(self.chars_seen + ch)
        return None if info is None else TrieNodeView(self._trie, info[0], self.chars_seen + ch)

    def __eq__(self, other):
        return isinstance(other, TrieNodeView) and other.node_id == self.node_id and other._trie is self._trie

    def __hash__(self):
        return hash(self.node_id)


class TrieView:
    """`vocab_trie` as the reference exposes it (utils.py:66-85): .root, .root_sharp, .root_p."""

    def __init__(self, native: N.WpTrie, tokens: List[str]):
        self._native, self._tokens = native, tokens
        self.root = TrieNodeView(self, 0, "")
        self.root_p = TrieNodeView(self, 1, "")
        self.root_sharp = TrieNodeView(self, native.node("##")[0], "##")

    def _decode(self, ids):
        return [self._tokens[int(t)] for t in ids]

    def node_by_id(self, node_id: int) -> TrieNodeView:
        if node_id == 0:
            return self.root
        if node_id == 1:
            return self.root_p
        return TrieNodeView(self, node_id, self._native.node_path(node_id))


class FastWP(NaiveWP):
    """wordpiece.py:211-330: LinMaxMatch end-to-end WordPiece; trie built in C++, matched on the device."""

    UNK = "['UNK']"  # wordpiece.py:257 (sic)

    def __init__(self, tokenizer=None):
        super().__init__(tokenizer)
        self._trie: Optional[N.WpTrie] = None
        self._tokens: List[str] = []
        self._corner: Optional[List[str]] = None
        self.vocab_trie: Optional[TrieView] = None
        self._enc = _Encoder(self, "_ensure_trie", "_tokens", naive=False, complain=self._raise_for_status, corner=True)

    def _ensure_trie(self) -> N.WpTrie:
        if self._trie is None:
            raise AttributeError("'FastWP' object has no attribute 'vocab_trie'")  # as the reference before load/train
        return self._trie

    def _build_trie(self) -> None:
        # utils.py:75-85; ids = position in the sorted vocabulary (vocab.json order is arbitrary, wordpiece.py:196)
        self._tokens = sorted(self.vocab)
        self._decode_table = self._decode_list = None
        if self._trie is not None:
            self._trie.close()
        self._trie = N.WpTrie(self._tokens)
        c = self._trie.corner()
        self._corner = None if c is None else self._decode(c)
        self.vocab_trie = TrieView(self._trie, self._tokens)

    def _decode(self, ids) -> List[str]:
        toks, n = self._tokens, len(self._tokens)
        ids = np.asarray(ids)
        if ids.size >= 4096 and int(ids.max()) <= n + 1:  # large outputs without the multi-token corner: one gather
            if getattr(self, "_decode_table", None) is None or self._decode_table.size != n + 2:
                self._decode_table = np.empty(n + 2, dtype=object)
                self._decode_table[:] = list(toks) + [self.UNK, "[UNK]"]
            return self._decode_table[ids.astype(np.int64)].tolist()
        out = []
        for t in map(int, ids):
            if t < n:
                out.append(toks[t])
            elif t == n:
                out.append(self.UNK)
            elif t == n + 1:
                out.append("[UNK]")  # wordpiece.py:149 via :261
            else:
                out.extend(self._corner)  # multi-token NaiveWP.encode_word("##")
        return out

    # -- wordpiece.py:227-231
    def train(self, corpus, max_vocab=30_000):
        super().train(corpus, max_vocab)
        self._build_trie()

    # -- batch entry points (not in the reference)
    def encode_ids_batch(self, texts: List[str], dropout: Optional[dict] = None, maxmatch_dropout: Optional[dict] = None):
        """texts -> (ids uint32, offsets uint64[n+1], status uint8[n]); see include/swt.h for ids and status.
        dropout: None; anything else is FastBPE's (ValueError).  maxmatch_dropout: None; anything else is NaiveWP's (ValueError:
        this class walks failure links, not MaxMatch -- a NaiveWP over the same vocabulary gives this class's ids).
        Added tokens (add_tokens) are not looked for here: only encode_batch honours them."""
        return _encode_ids(self._enc, texts, self._enc.channel(dropout, maxmatch_dropout))

    def tokenize_batch(self, texts: List[str], dropout: Optional[dict] = None, maxmatch_dropout: Optional[dict] = None) -> List[List[str]]:
        ids, off, status = self.encode_ids_batch(texts, dropout, maxmatch_dropout)
        _raise_flagged(self._enc, status, texts)
        if ids.size and int(ids.max()) <= len(self._tokens) + 1:  # no multi-token corner: one table, references handed out
            if ids.size < 4096:
                toks = self._decode(ids)
                return [toks[int(off[i]):int(off[i + 1])] for i in range(len(texts))]
            if getattr(self, "_decode_list", None) is None or len(self._decode_list) != len(self._tokens) + 2:
                self._decode_list = list(self._tokens) + [self.UNK, "[UNK]"]
            return N.nested_lists(self._decode_list, ids, off)
        return [self._decode(ids[int(off[i]):int(off[i + 1])]) for i in range(len(texts))]

    # -- token spans (not in the reference): they come out of the trie walk itself (swt_wp_encode_spans).
    # The inherited encode_spans_batch / tokenize_with_offsets are NaiveWP's: they answer with NaiveWP's tokens over this
    # vocabulary, not with FastWP's.  FastWP's own are the two methods below.
    def fast_encode_spans_batch(self, texts: List[str]):
        """texts -> (ids, offsets, status, spans uint32[n, 2], word_ids uint32[n]): encode_ids_batch plus, per token, its
        (start, end) in code points of text.lower() and the index of its segment among those of the sentence that emit a token
        (include/swt.h: a valid segment's tokens cover a prefix of it, "['UNK']" reaches to the next boundary, the '##' corner
        covers two).  A multi-token corner is one id (len(vocab) + 2) with the corner's span.  A text the reference does not
        return from raises as in tokenize_batch.  One pack, one trip to the device.  Added tokens (add_tokens) are not looked for here: only encode_batch honours them."""
        if not isinstance(texts, list) or not all(isinstance(t, str) for t in texts):
            raise TypeError("Text to tokenize must be a string.")
        return self._batch_encode_spans_packed(*N.pack_and_lower(texts), texts)

    def _batch_encode_spans_packed(self, text, off, texts, dropout=None):
        self._enc.draw(dropout)  # (this class has none: anything but None raises)
        ids, tok_off, status, spans, word = self._ensure_trie().encode_spans(text, off, codepoints=True)
        _raise_flagged(self._enc, status, texts)
        return ids, tok_off, status, spans, word

    def _refuse_added(self) -> None:
        # A token with whitespace inside is matched across the words of a text by this class's walk (wordpiece.py:233-270 runs
        # over the whole text): the blanks that hide an added token would become part of such a match.
        if self._trie is not None and self._enc._cached("ws_token", lambda sp: any(_class_of(ch) & N.CLS_BERT_WS for t in sp for ch in t)):
            raise ValueError("FastWP: the vocabulary holds a token with whitespace inside, which added tokens do not go with")

    def fast_tokenize_with_offsets(self, text: str) -> List[Tuple[str, Tuple[int, int]]]:
        """[(token, (start, end)), ...]: FastWP.tokenize(text) with the code points of text.lower() every token covers; a
        multi-token '##' corner is spelled as its tokens, each with the corner's span"""
        if not isinstance(text, str):
            raise TypeError("Text to tokenize must be a string.")
        ids, _, _, spans, _ = self.fast_encode_spans_batch([text])
        out = []
        for i, (s, e) in zip(ids.tolist(), spans.tolist()):
            out.extend((tok, (int(s), int(e))) for tok in self._decode([i]))
        return out

    # -- model-ready batches: FastWP's own ids and, with offsets, the spans of its trie walk
    def _batch_encode_spans(self, texts):
        return self.fast_encode_spans_batch(texts)

    def _batch_encode_dev(self, d_text, n_bytes, d_off, n_sent, d_ids, d_tok_off, d_ntok, d_spans, d_word, stream, empty):
        import torch
        trie, d_status = self._ensure_trie(), empty(n_sent + 8, torch.uint8)
        if d_spans is None:
            trie.encode_dev(d_text, n_bytes, d_off, n_sent, d_ids, d_tok_off, d_status.data_ptr(), d_ntok, stream)
        else:
            trie.encode_spans_dev(d_text, n_bytes, d_off, n_sent, d_ids, d_tok_off, d_status.data_ptr(), d_ntok, d_spans, d_word, True, stream)
        return [(d_status, lambda st, i, text: self._raise_for_status(st, text))]

    @staticmethod
    def _raise_for_status(st: int, text: str) -> None:
        if st == N.WP_NONTERMINATING:
            # documented deviation: the reference spins forever here; we refuse instead
            raise RuntimeError("FastWP.tokenize: the reference does not terminate on this input: %r" % text[:80])
        if st == N.WP_INDEXERROR:
            raise IndexError("string index out of range")  # wordpiece.py:285 with i == len(seq)

    # -- wordpiece.py:233-270
    def tokenize(self, text, maxmatch_dropout: Optional[dict] = None):
        if not isinstance(text, str):
            raise TypeError("Text to tokenize must be a string.")
        return self.tokenize_batch([text], maxmatch_dropout=maxmatch_dropout)[0]

    # -- wordpiece.py:318-330
    def load_resources(self, path: str) -> None:
        super().load_resources(path)
        self._build_trie()

    def save_resources(self, path: str) -> None:
        super().save_resources(path)
