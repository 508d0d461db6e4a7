"""ctypes binding of libswt_hip.so (include/swt.h).

The library is the product: there is no Python or CPU implementation of the hot path behind it.  If the
shared object has not been built, or a call needs a GPU that is not there, this module raises -- loudly.
"""
import ctypes as C
import os

import numpy as np

from . import _build

SYM_BASE = 0x110000
WP_CONT = 0x110000  # '##c' = WP_CONT + ord(c) in a WordPiece trainer
WP_MERGED_BASE = 0x220000
BPE_CONT = 0x80000000
BPE_RAW_WORDS = 1
BPE_NO_DEDUP = 2
WP_OK, WP_NONTERMINATING, WP_INDEXERROR = 0, 1, 2
ERR_NO_DEVICE, ERR_INVALID, ERR_CAPACITY, ERR_HIP, ERR_UNSUPPORTED, ERR_STATE, ERR_NOMEM, ERR_INTERNAL = -1, -2, -3, -4, -5, -6, -7, -8
CLS_BERT_WS, CLS_BERT_PUNCT, CLS_PY_SPACE, CLS_PY_ALNUM = 1, 2, 4, 8
NO_POS = 0xFFFFFFFFFFFFFFFF
SPAN_CODEPOINTS = 1
SPAN_OK, SPAN_MISMATCH = 0, 1
SPAN_WHOLE_WORD = 0  # a length-table entry: the token stands for its whole word ("[UNK]")
SPAN_LEN_CONT = 0x80000000  # a length-table entry of an unflagged stream: the token continues its word ('##')
BATCH_NONE = 0xFFFFFFFF  # swt_batch_spec: an absent cls_id / sep_id; a map entry without a dense id
BATCH_WINDOWS, BATCH_PAD_LEFT, BATCH_IDS64 = 1, 2, 4
PAIR_LONGEST_FIRST, PAIR_ONLY_FIRST, PAIR_ONLY_SECOND = 0, 1, 2  # the truncation strategies of swt_batch_pair_*
PAIR_OK, PAIR_REFUSED = 0, 1
PACK_WHOLE, PACK_SPLIT, PACK_DROP_LAST = 1, 2, 4  # the mode of swt_pack_*: one of the first two, DROP_LAST or-ed to SPLIT

u8p = C.POINTER(C.c_uint8)
u32p = C.POINTER(C.c_uint32)
i32p = C.POINTER(C.c_int32)
u64p = C.POINTER(C.c_uint64)
i64p = C.POINTER(C.c_int64)
vpp = C.POINTER(C.c_void_p)


class BatchSpec(C.Structure):
    """swt_batch_spec (include/swt.h): the shape of a padded batch"""
    _fields_ = [(name, C.c_uint32) for name in ("width", "stride", "flags", "pad_id", "unk_id", "cls_id", "sep_id")]


bsp = C.POINTER(BatchSpec)
MLM_WHOLE_WORD, MLM_IDS64 = 1, 4  # the flags of swt_mlm_spec
MLM_IGNORE = -100  # the label of a column that is not selected


class MlmSpec(C.Structure):
    """swt_mlm_spec (include/swt.h): the draws and thresholds of a masked-LM call"""
    _fields_ = [(name, C.c_uint64) for name in ("seed", "select_below", "mask_below", "random_below")] + \
               [(name, C.c_uint32) for name in ("epoch", "flags", "mask_id", "n_class")]


msp = C.POINTER(MlmSpec)

# every symbol include/swt.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "swt_last_error": (C.c_char_p, []),
    "swt_version": (C.c_int, []),
    "swt_abi_selftest": (C.c_int, [C.c_int]),
    "swt_init": (C.c_int, [C.c_int]),
    "swt_device_count": (C.c_int, []),
    "swt_device_info": (C.c_int, [C.POINTER(C.c_int), C.c_char_p, C.c_size_t]),
    "swt_profile_enable": (C.c_int, [C.c_int]),
    "swt_profile_read": (C.c_int, [C.POINTER(C.c_double), u64p]),
    "swt_class_of": (C.c_uint, [C.c_uint32]),
    "swt_bpe_table_create": (C.c_int, [u32p, u32p, u32p, C.c_uint32, vpp]),
    "swt_bpe_table_destroy": (None, [C.c_void_p]),
    "swt_bpe_table_set_option": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "swt_wp_trie_set_option": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "swt_bpe_encode": (C.c_int, [C.c_void_p, u8p, u64p, C.c_uint64, u32p, C.c_uint64, u64p, u64p, C.c_uint32]),
    "swt_bpe_encode_joined": (C.c_int, [C.c_void_p, u8p, C.c_uint64, C.c_uint64, u32p, C.c_uint64, u64p, u64p, u8p, C.c_uint32]),
    "swt_bpe_encode_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_uint32, C.c_void_p]),
    "swt_bpe_encode_naive": (C.c_int, [C.c_void_p, u8p, u64p, C.c_uint64, u32p, C.c_uint64, u64p, u64p, C.c_uint32]),
    "swt_bpe_encode_naive_joined": (C.c_int, [C.c_void_p, u8p, C.c_uint64, C.c_uint64, u32p, C.c_uint64, u64p, u64p, u8p, C.c_uint32]),
    "swt_bpe_encode_naive_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_uint32, C.c_void_p]),
    "swt_bpe_encode_dropout": (C.c_int, [C.c_void_p, u8p, u64p, C.c_uint64, u32p, C.c_uint64, u64p, u64p, C.c_uint32, C.c_uint64, C.c_uint64,
                                         C.c_uint32]),
    "swt_bpe_encode_dropout_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p]),
    "swt_wp_trie_create": (C.c_int, [u32p, u64p, C.c_uint32, vpp]),
    "swt_wp_trie_destroy": (None, [C.c_void_p]),
    "swt_wp_trie_stats": (C.c_int, [C.c_void_p, u32p, u32p, u32p]),
    "swt_wp_trie_corner": (C.c_int64, [C.c_void_p, u32p, C.c_uint64]),
    "swt_wp_trie_node": (C.c_int, [C.c_void_p, u32p, C.c_uint64, u32p, i32p, u8p, u32p, C.c_uint32, u32p]),
    "swt_wp_trie_node_path": (C.c_int, [C.c_void_p, C.c_uint32, u32p, C.c_uint64, u64p]),
    "swt_wp_encode": (C.c_int, [C.c_void_p, u8p, u64p, C.c_uint64, u32p, C.c_uint64, u64p, u8p, u64p]),
    "swt_wp_encode_joined": (C.c_int, [C.c_void_p, u8p, C.c_uint64, C.c_uint64, u32p, C.c_uint64, u64p, u8p, u64p, u8p]),
    "swt_wp_encode_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p]),
    "swt_wp_encode_naive": (C.c_int, [C.c_void_p, u8p, u64p, C.c_uint64, u32p, C.c_uint64, u64p, u8p, u64p]),
    "swt_wp_encode_naive_joined": (C.c_int, [C.c_void_p, u8p, C.c_uint64, C.c_uint64, u32p, C.c_uint64, u64p, u8p, u64p, u8p]),
    "swt_wp_encode_naive_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p]),
    "swt_wp_encode_naive_dropout": (C.c_int, [C.c_void_p, u8p, u64p, C.c_uint64, u32p, C.c_uint64, u64p, u8p, u64p, C.c_uint64, C.c_uint64,
                                              C.c_uint32]),
    "swt_wp_encode_naive_dropout_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p]),
    "swt_lower_of": (C.c_uint32, [C.c_uint32]),
    "swt_unidata_version": (C.c_char_p, []),
    "swt_utf8_lower": (C.c_int, [u8p, u64p, C.c_uint64, u8p]),
    "swt_utf8_prepare": (C.c_int, [u8p, C.c_uint64, u64p, C.c_uint64, u64p, u8p]),
    "swt_utf8_prepare_joined": (C.c_int, [u8p, C.c_uint64, C.c_uint64, u8p, u64p, u8p]),
    "swt_utf8_lower_dev": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    "swt_token_histogram": (C.c_int, [u32p, C.c_uint64, C.c_uint32, u64p, u64p]),
    "swt_token_histogram_dev": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "swt_token_equivalence": (C.c_int, [u32p, u64p, u32p, C.c_uint32, C.c_uint32, C.c_int, u32p, u64p, u32p, C.c_uint32, C.c_uint32, C.c_int,
                                        C.c_uint64, u32p, u64p, u32p]),
    "swt_token_equivalence_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p]),
    "swt_token_equivalence_capacity": (C.c_int, [u32p, u32p]),
    "swt_token_spans": (C.c_int, [u8p, u64p, C.c_uint64, u32p, u64p, u32p, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, u32p, u32p, u8p]),
    "swt_token_spans_dev": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                      C.c_uint32, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "swt_token_spans_capacity": (C.c_int, [u32p, u32p, u32p]),
    "swt_wp_encode_spans": (C.c_int, [C.c_void_p, u8p, u64p, C.c_uint64, u32p, C.c_uint64, u64p, u8p, u64p, C.c_uint32, u32p, u32p]),
    "swt_wp_encode_spans_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "swt_wp_encode_spans_capacity": (C.c_int, [u32p, u32p, u32p, u32p, u32p]),
    "swt_bpe_train_create_text": (C.c_int, [u8p, u64p, C.c_uint64, vpp]),
    "swt_bpe_train_create_joined": (C.c_int, [u8p, C.c_uint64, C.c_uint64, u8p, vpp]),
    "swt_wp_train_create_text": (C.c_int, [u8p, u64p, C.c_uint64, vpp]),
    "swt_wp_train_create_joined": (C.c_int, [u8p, C.c_uint64, C.c_uint64, u8p, vpp]),
    "swt_bpe_train_create_words": (C.c_int, [u32p, u64p, u32p, C.c_uint64, vpp]),
    "swt_bpe_train_destroy": (None, [C.c_void_p]),
    "swt_bpe_train_set_pos_base": (C.c_int, [C.c_void_p, C.c_uint64]),
    "swt_bpe_train_info": (C.c_int, [C.c_void_p, u64p, u64p, u32p, u64p]),
    "swt_bpe_train_base_symbols": (C.c_int, [C.c_void_p, u32p, C.c_uint32]),
    "swt_bpe_train_best": (C.c_int, [C.c_void_p, u32p, u32p, u64p, u64p, u64p]),
    "swt_bpe_train_apply": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32]),
    "swt_bpe_train_run": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, u32p, u32p, u64p, u32p]),
    "swt_bpe_train_export": (C.c_int, [C.c_void_p, u32p, C.c_uint64, u64p, u32p]),
    "swt_bpe_train_histogram": (C.c_int, [C.c_void_p, u64p, u64p, C.c_uint64, u64p]),
    "swt_bpe_train_stats": (C.c_int, [C.c_void_p, u64p, C.c_uint32]),
    "swt_bpe_train_trace": (C.c_int, [C.c_void_p, u64p, C.c_uint64, u64p]),
    "swt_dist_unique_id": (C.c_int, [u8p]),
    "swt_dist_init": (C.c_int, [C.c_int, C.c_int, u8p, vpp]),
    "swt_dist_init_local": (C.c_int, [C.c_int, vpp]),
    "swt_dist_destroy": (None, [C.c_void_p]),
    "swt_dist_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "swt_bpe_train_shard_begin": (C.c_int, [vpp, C.c_uint32, C.c_void_p, u32p, C.c_uint32, u32p]),
    "swt_bpe_train_run_sharded": (C.c_int, [vpp, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, u32p, u32p, u64p, u32p]),
    "swt_batch_plan": (C.c_int, [u64p, C.c_uint64, bsp, u64p, u64p]),
    "swt_batch_plan_dev": (C.c_int, [C.c_void_p, C.c_uint64, bsp, C.c_void_p, C.c_void_p, C.c_void_p]),
    "swt_batch_rows": (C.c_int, [u32p, u64p, C.c_uint64, u32p, C.c_uint32, C.c_int, u32p, u32p, bsp, u64p, C.c_uint64, C.c_void_p, u8p, u32p,
                                 u32p, u32p, u32p, u64p]),
    "swt_batch_rows_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, bsp,
                                     C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p]),
    "swt_batch_capacity": (C.c_int, [u32p, u32p]),
    "swt_batch_pair_plan": (C.c_int, [u64p, u64p, C.c_uint64, bsp, C.c_uint32, u64p, u8p, u64p]),
    "swt_batch_pair_plan_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, bsp, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "swt_batch_pair_rows": (C.c_int, [u32p, u64p, u64p, C.c_uint64, u32p, C.c_uint32, C.c_int, u32p, u32p, bsp, C.c_uint32, u64p, u8p, C.c_uint64,
                                      C.c_void_p, u8p, C.c_void_p, u8p, C.c_void_p, u32p, u32p, u32p, u32p, u64p]),
    "swt_batch_pair_rows_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p,
                                          bsp, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64] + [C.c_void_p] * 11),
    "swt_batch_pair_capacity": (C.c_int, [u32p, u32p]),
    "swt_pack_plan": (C.c_int, [u64p, C.c_uint64, bsp, C.c_uint32, u64p, u64p, u64p]),
    "swt_pack_plan_dev": (C.c_int, [C.c_void_p, C.c_uint64, bsp, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "swt_pack_rows": (C.c_int, [u32p, u64p, C.c_uint64, u32p, C.c_uint32, C.c_int, bsp, C.c_uint32, u64p, u64p, C.c_uint64, C.c_void_p, u8p,
                                u32p, u32p, u32p, u32p, u64p]),
    "swt_pack_rows_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_int, bsp, C.c_uint32, C.c_void_p,
                                    C.c_void_p, C.c_uint64] + [C.c_void_p] * 8),
    "swt_pack_capacity": (C.c_int, [u32p, u32p, u32p]),
    "swt_mlm_mask": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, u8p, u32p, C.c_uint32, msp, C.c_void_p, C.c_void_p, u8p, u64p]),
    "swt_mlm_mask_dev": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, msp] + [C.c_void_p] * 5),
    "swt_mlm_capacity": (C.c_int, [u32p, u32p]),
    "swt_decode_plan": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32] + [C.c_void_p] * 3),
    "swt_decode_plan_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32] +
                            [C.c_void_p] * 4),
    "swt_decode_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                  C.c_void_p, C.c_void_p, C.c_uint64]),
    "swt_decode_rows_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                      C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
    "swt_decode_capacity": (C.c_int, [u32p, u32p]),
    "swt_label_words": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64,
                                  C.c_uint64, C.c_void_p, C.c_uint32, C.c_int32, C.c_uint32] + [C.c_void_p] * 3),
    "swt_label_words_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64,
                                      C.c_uint64, C.c_void_p, C.c_uint32, C.c_int32, C.c_uint32] + [C.c_void_p] * 4),
    "swt_answer_positions": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64,
                                       C.c_void_p, C.c_int32, C.c_uint32] + [C.c_void_p] * 5),
    "swt_answer_positions_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p,
                                           C.c_uint64, C.c_void_p, C.c_int32, C.c_uint32] + [C.c_void_p] * 6),
    "swt_answer_best": (C.c_int, [C.c_void_p] * 5 + [C.c_int32, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint32, C.c_void_p,
                                  C.c_uint32] + [C.c_void_p] * 11),
    "swt_answer_best_dev": (C.c_int, [C.c_void_p] * 5 + [C.c_int32, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint32, C.c_void_p,
                                      C.c_uint32] + [C.c_void_p] * 12),
    "swt_label_capacity": (C.c_int, [u32p, u32p]),
    "swt_word_plan": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p]),
    "swt_word_plan_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64] + [C.c_void_p] * 3),
    "swt_word_predict": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32,
                                   C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32] + [C.c_void_p] * 9),
    "swt_word_predict_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32,
                                       C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32] + [C.c_void_p] * 10),
    "swt_entity_spans": (C.c_int, [C.c_void_p] * 5 + [C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32] + [C.c_void_p] * 8),
    "swt_entity_spans_dev": (C.c_int, [C.c_void_p] * 5 + [C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32] + [C.c_void_p] * 9),
    "swt_tag_capacity": (C.c_int, [u32p, u32p, u32p]),
    "swt_mlm_positions": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_int64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "swt_mlm_positions_dev": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_int64, C.c_uint32, C.c_uint32] + [C.c_void_p] * 3),
    "swt_mlm_predict": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint32] +
                        [C.c_void_p] * 7),
    "swt_mlm_predict_dev": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32,
                                      C.c_uint32] + [C.c_void_p] * 8),
    "swt_fill_capacity": (C.c_int, [u32p, u32p, u32p, u32p]),
    "swt_added_create": (C.c_int, [u8p, u64p, C.c_uint32, vpp]),
    "swt_added_destroy": (None, [C.c_void_p]),
    "swt_added_find": (C.c_int, [C.c_void_p, u8p, u64p, C.c_uint64, u8p, u64p, u32p, u32p, C.c_uint64, u64p]),
    "swt_added_find_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64] + [C.c_void_p] * 6),
    "swt_added_splice": (C.c_int, [u32p, u64p, u32p, u32p, C.c_uint64, u64p, u32p, u32p, C.c_uint32, u32p, u64p, u32p, u32p]),
    "swt_added_splice_dev": (C.c_int, [C.c_void_p] * 4 + [C.c_uint64] + [C.c_void_p] * 3 + [C.c_uint32] + [C.c_void_p] * 5),
    "swt_added_capacity": (C.c_int, [u32p] * 5),
}


class SwtError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("libswt_hip error %d: %s" % (code, message))
        self.code = code


class NoDeviceError(SwtError):
    """Raised when a compute call is made without a HIP device: there is no CPU path."""


_lib = None


def lib():
    """Load libswt_hip.so (built by `_build.build()`); never falls back to anything else."""
    global _lib
    if _lib is None:
        path = _build.LIB_PATH
        if not os.path.exists(path):
            raise ImportError(
                "libswt_hip.so is not built (%s). Run `python -c \"import __graft_entry__ as g; g.build()\"` "
                "or `python subword-tokenizers_amd/_build.py`; there is no Python/CPU fallback." % path)
        # One HIP runtime per process: PyTorch ships its own libamdhip64.so.7 (same SONAME as /opt/rocm's).  When
        # torch is importable, load it FIRST so that libswt_hip.so binds to the runtime torch already holds;
        # the other order leaves torch unable to see the GPU ("No HIP GPUs are available").
        if not os.environ.get("SWT_NO_TORCH_PRELOAD"):
            try:
                import torch  # noqa: F401
            except ImportError:
                pass
        L = C.CDLL(path)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)  # AttributeError here = the .so is stale against include/swt.h
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc):
    if rc == 0:
        return
    msg = lib().swt_last_error().decode("utf-8", "replace")
    if rc == ERR_NO_DEVICE:
        raise NoDeviceError(rc, msg)
    raise SwtError(rc, msg)


def ptr(a, typ):
    return a.ctypes.data_as(typ)


def class_of(cp):
    return lib().swt_class_of(cp)


def device_count():
    return lib().swt_device_count()


def init(device=0):
    check(lib().swt_init(device))


OPT_DEDUP, OPT_DEDUP_TABLE_BITS, OPT_UNIQUE_TILE, OPT_LANE_SPAN, OPT_LANE_TAPER, OPT_LANE_SLOTS = 1, 2, 3, 4, 5, 6
DEDUP_AUTO, DEDUP_NEVER, DEDUP_ALWAYS = 0, 1, 2


def profile_enable(on=True):
    """True/1 = time the dominant kernel of each path, 2 = time all kernels of a call, 3 = bracket only the wordref_kernel launch
    of the word-level dedup (profile_read then counts the dedup pipelines that ran: one per encode call that took that path, none
    for a direct one), False/0 = off"""
    check(lib().swt_profile_enable(int(on)))


def profile_read():
    """-> (summed milliseconds of the dominant kernel, launches) since the last read"""
    ms, n = C.c_double(), C.c_uint64()
    check(lib().swt_profile_read(C.byref(ms), C.byref(n)))
    return ms.value, n.value


def device_info():
    n = C.c_int()
    name = C.create_string_buffer(256)
    check(lib().swt_device_info(C.byref(n), name, 256))
    return n.value, name.value.decode()


# --------------------------------------------------------------------------------------------------
# packing: what the reference does per sentence in Python (str.lower(), utils.py:27 / wordpiece.py:248)
# stays in Python; the device consumes the lowercased UTF-8 bytes of the whole batch.

def lower_of(cp):
    """the device lowercase table: lowercase code point, or 0xFFFFFFFF for the code points left to the host"""
    return int(lib().swt_lower_of(cp))


_lower_ok = None


def device_lower_ok():
    """The device's lowercase table speaks for this interpreter's str.lower(): both follow the same Unicode database.  If not,
    every batch is lowercased on the host, so that a text tokenizes the same whatever the size of the batch it comes in."""
    global _lower_ok
    if _lower_ok is None:
        import unicodedata
        _lower_ok = lib().swt_unidata_version().decode() == unicodedata.unidata_version
    return _lower_ok


_pyhost = None


def pyhost():
    """csrc/swt_pyhost.c through ctypes.PyDLL (the GIL stays held), or None where it could not be built."""
    global _pyhost
    if _pyhost is None:
        path = _build.build_pyhost()
        dll = False
        if path:
            try:
                dll = C.PyDLL(path)
                dll.swt_py_join_bound.argtypes = [C.py_object]
                dll.swt_py_join_bound.restype = C.c_longlong
                dll.swt_py_join_fill.argtypes = [C.py_object, C.c_void_p, C.c_longlong, C.POINTER(C.c_longlong)]
                dll.swt_py_join_fill.restype = C.c_longlong
                dll.swt_py_nested.argtypes = [C.py_object, C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong]
                dll.swt_py_nested.restype = C.py_object
                dll.swt_py_bpe_merge_strings.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_uint32, C.c_uint32, C.py_object, C.py_object,
                                                         C.py_object, C.py_object, C.POINTER(C.c_uint32)]
                dll.swt_py_bpe_merge_strings.restype = C.c_longlong
                dll.swt_py_distinct.argtypes = [C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong, C.c_void_p]
                dll.swt_py_distinct.restype = C.c_longlong
                dll.swt_py_nested_via.argtypes = [C.py_object, C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong]
                dll.swt_py_nested_via.restype = C.py_object
            except OSError:
                dll = False
        _pyhost = dll
    return _pyhost or None


def join_texts(texts, error="Text must be a string."):
    """list[str] -> (uint8 array: the UTF-8 (surrogatepass) of the texts with ONE zero byte between neighbours, the number of
    U+0000 inside the texts).  TypeError(error) when an item is not a str.  One pass over the strings in C where
    csrc/swt_pyhost.c could be built, str.join + str.encode otherwise."""
    h = pyhost()
    if h is not None:
        bound = h.swt_py_join_bound(texts)
        if bound < 0:
            raise TypeError(error)
        buf = np.empty(bound + 32, dtype=np.uint8)
        n_nul = C.c_longlong()
        w = h.swt_py_join_fill(texts, buf.ctypes.data, bound + 32, C.byref(n_nul))
        if w < 0:
            raise RuntimeError("swt_py_join_fill: the list changed during the call")
        return buf[:w], int(n_nul.value)
    if not all(isinstance(t, str) for t in texts):
        raise TypeError(error)
    data = "\x00".join(texts).encode("utf-8", "surrogatepass")
    return np.frombuffer(data, dtype=np.uint8), data.count(0) - max(len(texts) - 1, 0)


def nested_lists(table, inv, off):
    """[[table[inv[k]] for k in range(off[s], off[s + 1])] for s in range(len(off) - 1)]: token strings per sentence, the
    reference's output shape, from a list of strings, int32 indices into it and uint64 sentence offsets"""
    inv = np.ascontiguousarray(inv, dtype=np.int32)
    off = np.ascontiguousarray(off, dtype=np.uint64)
    n_sent = int(off.size - 1)
    h = pyhost()
    if h is not None:
        return h.swt_py_nested(table, inv.ctypes.data, int(inv.size), off.ctypes.data, n_sent)
    if inv.size and (int(inv.min()) < 0 or int(inv.max()) >= len(table)):
        raise IndexError("token index outside the table")
    arr = np.empty(len(table), dtype=object)
    arr[:] = table
    toks = arr[inv].tolist()
    return [toks[int(off[i]):int(off[i + 1])] for i in range(n_sent)]


def nested_lists_by_key(key, cap, spell, off):
    """The same for tokens named by sparse keys in [0, cap): spell(k) is called once per DISTINCT key (in order of first
    appearance) and every sentence gets references to those strings.  key: uint32 array."""
    key = np.ascontiguousarray(key, dtype=np.uint32)
    off = np.ascontiguousarray(off, dtype=np.uint64)
    h = pyhost()
    if h is None:
        if key.size and int(key.max()) >= cap:
            raise IndexError("token outside the table")
        uniq, inv = np.unique(key, return_inverse=True)
        return nested_lists([spell(int(k)) for k in uniq.tolist()], inv, off)
    pos = np.full(cap, -1, dtype=np.int32)
    uniq = np.empty(min(cap, max(int(key.size), 1)), dtype=np.uint32)
    n = h.swt_py_distinct(key.ctypes.data, int(key.size), pos.ctypes.data, cap, uniq.ctypes.data)
    if n < 0:
        raise IndexError("token outside the table")
    table = [spell(k) for k in uniq[:n].tolist()]
    return h.swt_py_nested_via(table, key.ctypes.data, int(key.size), pos.ctypes.data, cap, off.ctypes.data, int(off.size - 1))


def pack_and_lower(texts):
    """list[str] -> (uint8 bytes of the LOWERCASED texts, uint64 byte offsets[n+1]).  The host joins (with U+0000 between the
    texts) and encodes once; the sentence offsets and str.lower() come from the device (swt_utf8_prepare_joined; texts that
    hold U+0000 themselves go by their code-point lengths, swt_utf8_prepare); the few sentences the device flags are lowercased
    here and spliced in."""
    n = len(texts)
    if (n <= 64 and sum(map(len, texts)) <= 16384) or not device_lower_ok():
        # the reference-style call (one sentence, or a few): a device round trip costs more than str.lower() here
        return pack_utf8([t.lower() for t in texts])
    off = np.zeros(n + 1, dtype=np.uint64)
    if n == 0:
        return np.zeros(0, dtype=np.uint8), off
    need = np.zeros(n, dtype=np.uint8)
    # one join with U+0000 between the texts; the device finds the separators (as long as the texts hold no U+0000 of their
    # own), closes the gaps, lowercases
    joined, n_nul = join_texts(texts)
    if joined.size + 1 == n:  # nothing but separators: every text is empty
        return np.zeros(0, dtype=np.uint8), off
    if n_nul == 0:
        buf = np.empty(joined.size - (n - 1), dtype=np.uint8)
        check(lib().swt_utf8_prepare_joined(ptr(joined, u8p), int(joined.size), n, ptr(buf, u8p), ptr(off, u64p), ptr(need, u8p)))
    else:
        # a text with U+0000 in it: code-point lengths tell the sentences apart (len(str) is free, byte lengths are not)
        cp_off = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum(np.fromiter(map(len, texts), dtype=np.uint64, count=n), out=cp_off[1:])
        data = "".join(texts).encode("utf-8", "surrogatepass")
        buf = np.frombuffer(data, dtype=np.uint8).copy()
        check(lib().swt_utf8_prepare(ptr(buf, u8p), int(buf.size), ptr(cp_off, u64p), n, ptr(off, u64p), ptr(need, u8p)))
    if need.any():
        data = buf.tobytes()
        parts = [texts[i].lower().encode("utf-8", "surrogatepass") if need[i] else data[int(off[i]):int(off[i + 1])] for i in range(n)]
        off = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum(np.fromiter(map(len, parts), dtype=np.uint64, count=n), out=off[1:])
        buf = np.frombuffer(b"".join(parts), dtype=np.uint8)
    return buf, off


def pack_utf8(lowered):
    """list[str] (already lowercased) -> (uint8 bytes, uint64 offsets[n+1])."""
    enc = [s.encode("utf-8", "surrogatepass") for s in lowered]
    off = np.zeros(len(enc) + 1, dtype=np.uint64)
    if enc:
        np.cumsum(np.fromiter(map(len, enc), dtype=np.uint64, count=len(enc)), out=off[1:])
    buf = np.frombuffer(b"".join(enc), dtype=np.uint8)
    if buf.size == 0:
        buf = np.zeros(1, dtype=np.uint8)[:0]
    return buf, off


def pack_utf32(strings):
    """list[str] -> (uint32 code points, uint64 offsets[n+1])."""
    off = np.zeros(len(strings) + 1, dtype=np.uint64)
    if strings:
        np.cumsum(np.fromiter(map(len, strings), dtype=np.uint64, count=len(strings)), out=off[1:])
    blob = np.frombuffer("".join(strings).encode("utf-32-le", "surrogatepass"), dtype=np.uint32)
    return blob, off


def token_histogram_counts(ids, id_cap):
    """swt_token_histogram as it is: -> (uint64 counts[2 * id_cap], how many ids lie outside [0, id_cap): they are counted nowhere)"""
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    counts = np.zeros(2 * int(id_cap), dtype=np.uint64)
    oor = C.c_uint64()
    check(lib().swt_token_histogram(ptr(ids, u32p) if ids.size else None, int(ids.size), int(id_cap), ptr(counts, u64p), C.byref(oor)))
    return counts, oor.value


def token_histogram(ids, id_cap):
    """uint32 token ids -> uint64 counts[2 * id_cap] (second half: ids carrying BPE_CONT), counted on the device"""
    counts, oor = token_histogram_counts(ids, id_cap)
    if oor:
        raise ValueError("%d token ids are outside [0, %d)" % (oor, id_cap))
    return counts


def token_equivalence_capacity():
    """-> (wave_cap, block_cap): the shorter side's length up to which one wavefront counts a row of token_equivalence, and the
    distinct tokens one pass of the workgroup kernel holds for the longer rows (csrc/swt_metrics.hip)"""
    a, b = C.c_uint32(), C.c_uint32()
    check(lib().swt_token_equivalence_capacity(C.byref(a), C.byref(b)))
    return a.value, b.value


def token_equivalence(side_a, side_b, weight=None, per_row=False):
    """The counting of benchmarks.py:113-183 over two id streams with the same rows, on the device (swt_token_equivalence).
    side = (ids uint32, offsets uint64[n_rows + 1], map uint32, map_base, flagged): see include/swt.h for the canonical id a
    map gives a token; a flagged map has two halves.  weight: uint32 per row, or None = 1.
    -> totals uint64[4] = (positions, pos_matches, unordered, has_common), each row times its weight; with per_row also the
    uint32[n_rows, 4] of the rows themselves.  ValueError when an id lies beyond its map."""
    args, keep = [], []
    n_rows = int(np.asarray(side_a[1]).size) - 1
    for ids, off, cmap, base, flagged in (side_a, side_b):
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        cmap = np.ascontiguousarray(cmap, dtype=np.uint32)
        if int(off.size) - 1 != n_rows or n_rows < 0:
            raise ValueError("the two streams must have the same rows")
        if off[0] != 0 or int(off[-1]) != ids.size:
            raise ValueError("offsets must run from 0 to the number of ids")
        if flagged and cmap.size % 2:
            raise ValueError("a flagged map has two halves of equal size")
        keep += [ids, off, cmap]
        args += [ptr(ids, u32p) if ids.size else None, ptr(off, u64p), ptr(cmap, u32p) if cmap.size else None, int(base),
                 int(cmap.size) // 2 if flagged else int(cmap.size), int(bool(flagged))]
    if weight is not None:
        weight = np.ascontiguousarray(weight, dtype=np.uint32)
        if weight.size != n_rows:
            raise ValueError("one weight per row")
    totals = np.zeros(5, dtype=np.uint64)
    rows = np.zeros((n_rows, 4), dtype=np.uint32) if per_row else None
    check(lib().swt_token_equivalence(*args, n_rows, ptr(weight, u32p) if weight is not None and n_rows else None, ptr(totals, u64p),
                                      ptr(rows, u32p) if per_row and n_rows else None))
    if totals[4]:
        raise ValueError("%d token ids are outside their canonical maps" % int(totals[4]))
    return (totals[:4], rows) if per_row else totals[:4]


def token_spans_capacity():
    """-> (block, chunk, tile): the byte sizes at which the span kernel changes form (csrc/swt_spans.hip): what one wavefront
    classifies per step and stages at a time, both counted from a sentence's first byte, and the window of text whose sentence
    starts one workgroup owns"""
    a, b, c = C.c_uint32(), C.c_uint32(), C.c_uint32()
    check(lib().swt_token_spans_capacity(C.byref(a), C.byref(b), C.byref(c)))
    return a.value, b.value, c.value


def token_spans(text_u8, off, ids, tok_off, len_table, len_base, flagged, codepoints=True):
    """Where every token came from, on the device (swt_token_spans): lowercased UTF-8 text with byte offsets[n_sent + 1], ids with
    their CSR offsets, a length table (include/swt.h) -> (spans uint32[n, 2] = start and end inside the sentence, in code points
    or bytes; word uint32[n] = index of the token's word in its sentence; status uint8[n_sent], SPAN_OK or SPAN_MISMATCH)."""
    text_u8 = np.ascontiguousarray(text_u8, dtype=np.uint8)
    off = np.ascontiguousarray(off, dtype=np.uint64)
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    tok_off = np.ascontiguousarray(tok_off, dtype=np.uint64)
    len_table = np.ascontiguousarray(len_table, dtype=np.uint32)
    n_sent = int(off.size) - 1
    if n_sent < 0 or tok_off.size != off.size:
        raise ValueError("text and ids must have the same sentences")
    if n_sent and (int(off[-1]) > text_u8.size or int(tok_off[-1]) > ids.size):
        raise ValueError("offsets run past their array")
    spans = np.zeros((ids.size, 2), dtype=np.uint32)
    word = np.zeros(ids.size, dtype=np.uint32)
    status = np.zeros(n_sent, dtype=np.uint8)
    check(lib().swt_token_spans(ptr(text_u8, u8p) if text_u8.size else None, ptr(off, u64p), n_sent, ptr(ids, u32p) if ids.size else None,
                                ptr(tok_off, u64p), ptr(len_table, u32p) if len_table.size else None, int(len_base), int(len_table.size),
                                int(bool(flagged)), SPAN_CODEPOINTS if codepoints else 0, ptr(spans, u32p) if ids.size else None,
                                ptr(word, u32p) if ids.size else None, ptr(status, u8p) if n_sent else None))
    return spans, word, status


def batch_spec(width, stride=0, windows=False, pad_left=False, ids64=False, pad_id=0, unk_id=1, cls_id=None, sep_id=None):
    """-> BatchSpec; cls_id / sep_id None: the row has no such token"""
    flags = (BATCH_WINDOWS if windows else 0) | (BATCH_PAD_LEFT if pad_left else 0) | (BATCH_IDS64 if ids64 else 0)
    return BatchSpec(int(width), int(stride), flags, int(pad_id), int(unk_id), BATCH_NONE if cls_id is None else int(cls_id),
                     BATCH_NONE if sep_id is None else int(sep_id))


def batch_capacity():
    """-> (cols_per_step, scan_group): the columns one wavefront of the batch kernel writes per step, and the rows of one scan
    group of the plan (csrc/swt_batch.hip)"""
    a, b = C.c_uint32(), C.c_uint32()
    check(lib().swt_batch_capacity(C.byref(a), C.byref(b)))
    return a.value, b.value


def batch_plan(tok_off, spec):
    """token offsets uint64[n_rows + 1] and a BatchSpec -> (row_base uint64[n_rows + 1] = the first output row of every source row,
    closed by the number of output rows; the longest source row in tokens), from the device (swt_batch_plan).  Without
    BATCH_WINDOWS the spec's width is not looked at."""
    tok_off = np.ascontiguousarray(tok_off, dtype=np.uint64)
    if tok_off.size < 1:
        raise ValueError("offsets hold n_rows + 1 entries")
    row_base = np.zeros(tok_off.size, dtype=np.uint64)
    info = np.zeros(2, dtype=np.uint64)
    check(lib().swt_batch_plan(ptr(tok_off, u64p), int(tok_off.size) - 1, C.byref(spec), ptr(row_base, u64p), ptr(info, u64p)))
    return row_base, int(info[1])


def batch_rows(ids, tok_off, spec, cmap=None, n_map=None, flagged=False, spans=None, word=None, row_base=None, rows_cap=None):
    """An id stream as padded rows, on the device (swt_batch_rows).  ids uint32 with offsets uint64[n_rows + 1]; cmap: the dense
    id of every sparse id (two halves of n_map entries when flagged), None = the identity below n_map; spans uint32[n, 2] and
    word uint32[n]: what the span calls return, carried along.  row_base: batch_plan's, needed with BATCH_WINDOWS.
    -> dict: input_ids int32 or int64 [rows, width], attention_mask uint8, length and sample uint32[rows], info uint64[3]
    (rows, source rows that lost tokens, tokens sent to unk_id), and offset_mapping uint32[rows, width, 2] / word_ids
    int32[rows, width] when the payloads were given."""
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    tok_off = np.ascontiguousarray(tok_off, dtype=np.uint64)
    n_rows = int(tok_off.size) - 1
    if n_rows < 0 or (n_rows and int(tok_off[-1]) > ids.size):
        raise ValueError("offsets run past their array")
    n_tok = int(tok_off[-1]) if n_rows else 0
    cmap, n_map, spans, word, row_base, rows_cap, out = _batch_rows_setup(n_rows, n_tok, spec, cmap, n_map, flagged, spans, word, row_base,
                                                                          rows_cap, 3)
    if rows_cap == 0 and n_rows == 0:
        return out  # no row in, no row out: nothing for the device to do
    check(lib().swt_batch_rows(_cast(ids, u32p), ptr(tok_off, u64p), n_rows, _cast(cmap, u32p), n_map, int(bool(flagged)),
                               ptr(spans, u32p) if spans is not None else None, ptr(word, u32p) if word is not None else None,
                               C.byref(spec), ptr(row_base, u64p) if row_base is not None else None, rows_cap,
                               out["input_ids"].ctypes.data_as(C.c_void_p), ptr(out["attention_mask"], u8p),
                               ptr(out["offset_mapping"], u32p) if spans is not None else None,
                               C.cast(out["word_ids"].ctypes.data_as(C.c_void_p), u32p) if word is not None else None,
                               ptr(out["sample"], u32p), ptr(out["length"], u32p), ptr(out["info"], u64p)))
    return out


def _vp(a):
    """the data of a NumPy array as void *; None for no array and for an empty one"""
    return a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None


def _cast(a, typ):
    return C.cast(_vp(a), typ) if a is not None and a.size else None


def _batch_rows_setup(n_rows, n_tok, spec, cmap, n_map, flagged, spans, word, row_base, rows_cap, n_info):
    """What batch_rows and batch_pair_rows do alike with their arguments: the map, the payloads of n_tok tokens and row_base as
    contiguous arrays of their types, each held to its size; n_map and rows_cap where they were left out; and the outputs both
    return, zeroed.  -> (cmap, n_map, spans, word, row_base, rows_cap, out)"""
    if cmap is not None:
        cmap = np.ascontiguousarray(cmap, dtype=np.uint32)
        if n_map is None:
            n_map = int(cmap.size) // 2 if flagged else int(cmap.size)
        if cmap.size != (2 * n_map if flagged else n_map):
            raise ValueError("a flagged map has two halves of n_map entries")
    elif n_map is None:
        n_map = 0x80000000
    if spans is not None:
        spans = np.ascontiguousarray(spans, dtype=np.uint32)
        if spans.size < 2 * n_tok:
            raise ValueError("two span words per token")
    if word is not None:
        word = np.ascontiguousarray(word, dtype=np.uint32)
        if word.size < n_tok:
            raise ValueError("one word index per token")
    if row_base is not None:
        row_base = np.ascontiguousarray(row_base, dtype=np.uint64)
        if row_base.size != n_rows + 1:
            raise ValueError("row_base holds n_rows + 1 entries")
    if rows_cap is None:
        rows_cap = int(row_base[-1]) if row_base is not None else n_rows
    rows_cap, width = int(rows_cap), int(spec.width)
    out = {
        "input_ids": np.zeros((rows_cap, width), dtype=np.int64 if spec.flags & BATCH_IDS64 else np.int32),
        "attention_mask": np.zeros((rows_cap, width), dtype=np.uint8),
        "length": np.zeros(rows_cap, dtype=np.uint32),
        "sample": np.zeros(rows_cap, dtype=np.uint32),
        "info": np.zeros(n_info, dtype=np.uint64),
    }
    if spans is not None:
        out["offset_mapping"] = np.zeros((rows_cap, width, 2), dtype=np.uint32)
    if word is not None:
        out["word_ids"] = np.zeros((rows_cap, width), dtype=np.int32)
    return cmap, int(n_map), spans, word, row_base, rows_cap, out


def batch_pair_capacity():
    """-> (cols_per_step, scan_group) of the pair kernels, as batch_capacity"""
    a, b = C.c_uint32(), C.c_uint32()
    check(lib().swt_batch_pair_capacity(C.byref(a), C.byref(b)))
    return a.value, b.value


def _pair_offsets(off_a, off_b):
    off_a, off_b = np.ascontiguousarray(off_a, dtype=np.uint64), np.ascontiguousarray(off_b, dtype=np.uint64)
    if off_a.size < 1 or off_a.size != off_b.size:
        raise ValueError("both offset arrays hold n_rows + 1 entries")
    return off_a, off_b


def batch_pair_plan(off_a, off_b, spec, strategy):
    """The offsets of both sides into one id stream (uint64[n_rows + 1] each), a BatchSpec and a PAIR_* strategy -> (row_base
    uint64[n_rows + 1], status uint8[n_rows] = PAIR_OK / PAIR_REFUSED, info uint64[5]: rows out, the largest na + nb, 0, refused
    pairs, 0), from the device (swt_batch_pair_plan).  A spec of width 0 asks for the largest pair alone."""
    off_a, off_b = _pair_offsets(off_a, off_b)
    row_base = np.zeros(off_a.size, dtype=np.uint64)
    status = np.zeros(off_a.size, dtype=np.uint8)  # one entry to spare: never an empty array
    info = np.zeros(5, dtype=np.uint64)
    check(lib().swt_batch_pair_plan(ptr(off_a, u64p), ptr(off_b, u64p), int(off_a.size) - 1, C.byref(spec), int(strategy), ptr(row_base, u64p),
                                    ptr(status, u8p), ptr(info, u64p)))
    return row_base, status[:-1], info


def batch_pair_rows(ids, off_a, off_b, spec, strategy, cmap=None, n_map=None, flagged=False, spans=None, word=None, row_base=None,
                    status=None, rows_cap=None):
    """Pairs of one id stream as padded rows [cls] A [sep] B [sep], on the device (swt_batch_pair_rows).  The arguments of
    batch_rows with two offset arrays, the strategy and the plan's status.  -> the dict of batch_rows and token_type_ids (the
    type of input_ids), special_tokens_mask uint8, sequence_ids int8 [rows, width]; info uint64[5] (rows, the largest na + nb,
    tokens sent to unk_id, refused pairs, pairs that lost tokens)."""
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    off_a, off_b = _pair_offsets(off_a, off_b)
    n_rows = int(off_a.size) - 1
    n_tok = max(int(off_a[-1]), int(off_b[-1])) if n_rows else 0
    if n_tok > ids.size:
        raise ValueError("offsets run past their array")
    cmap, n_map, spans, word, row_base, rows_cap, out = _batch_rows_setup(n_rows, n_tok, spec, cmap, n_map, flagged, spans, word, row_base,
                                                                          rows_cap, 5)
    if status is not None:
        status = np.ascontiguousarray(status, dtype=np.uint8)
        if status.size != n_rows:
            raise ValueError("status holds n_rows entries")
    shape = out["input_ids"].shape
    out["token_type_ids"] = np.zeros(shape, dtype=out["input_ids"].dtype)
    out["special_tokens_mask"] = np.zeros(shape, dtype=np.uint8)
    out["sequence_ids"] = np.zeros(shape, dtype=np.int8)
    if rows_cap == 0 and n_rows == 0:
        return out  # no pair in, no row out: nothing for the device to do
    check(lib().swt_batch_pair_rows(_cast(ids, u32p), ptr(off_a, u64p), ptr(off_b, u64p), n_rows, _cast(cmap, u32p), n_map,
                                    int(bool(flagged)), ptr(spans, u32p) if spans is not None else None,
                                    ptr(word, u32p) if word is not None else None, C.byref(spec), int(strategy),
                                    ptr(row_base, u64p) if row_base is not None else None, _cast(status, u8p), rows_cap,
                                    _vp(out["input_ids"]), _cast(out["attention_mask"], u8p), _vp(out["token_type_ids"]),
                                    _cast(out["special_tokens_mask"], u8p), _vp(out["sequence_ids"]),
                                    ptr(out["offset_mapping"], u32p) if spans is not None else None,
                                    C.cast(_vp(out["word_ids"]), u32p) if word is not None else None,
                                    ptr(out["sample"], u32p), ptr(out["length"], u32p), ptr(out["info"], u64p)))
    return out


def pack_capacity():
    """-> (cols_per_step, scan_group, orbit_group): the columns one wavefront of the packing kernel writes per step, the rows
    of one scan group of its plan and the rows of one group of the WHOLE plan's orbit step (csrc/swt_pack.hip)"""
    a, b, c = C.c_uint32(), C.c_uint32(), C.c_uint32()
    check(lib().swt_pack_capacity(C.byref(a), C.byref(b), C.byref(c)))
    return a.value, b.value, c.value


def pack_plan(tok_off, spec, mode):
    """token offsets uint64[n_rows + 1], a BatchSpec and a PACK_* mode -> (slot uint64[n_rows + 1]: the flat output position of
    every source row's segment, closed by the end of the last one; row_first uint64[n_rows + 1]: the source row that owns column 0
    of each packed row, n_rows from the last packed row on; info uint64[4]: packed rows, the longest source row in tokens, 0,
    the columns of all segments), from the device (swt_pack_plan)."""
    tok_off = np.ascontiguousarray(tok_off, dtype=np.uint64)
    if tok_off.size < 1:
        raise ValueError("offsets hold n_rows + 1 entries")
    slot, row_first = np.zeros(tok_off.size, dtype=np.uint64), np.zeros(tok_off.size, dtype=np.uint64)
    info = np.zeros(4, dtype=np.uint64)
    check(lib().swt_pack_plan(ptr(tok_off, u64p), int(tok_off.size) - 1, C.byref(spec), int(mode), ptr(slot, u64p), ptr(row_first, u64p),
                              ptr(info, u64p)))
    return slot, row_first, info


def pack_rows(ids, tok_off, spec, mode, slot, row_first, cmap=None, n_map=None, flagged=False, rows_cap=None):
    """An id stream as packed rows, on the device (swt_pack_rows).  ids, tok_off, cmap, n_map, flagged as batch_rows takes them;
    slot and row_first: pack_plan's.  rows_cap: the rows of the outputs; None = what the plan needs.
    -> dict: input_ids int32 or int64 [rows, width], attention_mask uint8, position_ids uint32, sequence_ids and sample_ids int32
    (-1 on padding), length uint32[rows], info uint64[3] (rows, source rows that lost tokens, tokens sent to unk_id)."""
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    tok_off = np.ascontiguousarray(tok_off, dtype=np.uint64)
    slot, row_first = np.ascontiguousarray(slot, dtype=np.uint64), np.ascontiguousarray(row_first, dtype=np.uint64)
    n_rows = int(tok_off.size) - 1
    if n_rows < 0 or (n_rows and int(tok_off[-1]) > ids.size):
        raise ValueError("offsets run past their array")
    if slot.size != n_rows + 1 or row_first.size != n_rows + 1:
        raise ValueError("slot and row_first hold n_rows + 1 entries")
    cmap, n_map = _batch_rows_setup(n_rows, 0, spec, cmap, n_map, flagged, None, None, None, 0, 3)[:2]
    width = int(spec.width)
    if rows_cap is None:
        rows_cap = 0
        if n_rows:
            end = int(slot[-1])
            rows_cap = end // width if mode & PACK_DROP_LAST else -(-end // width)
            if mode & PACK_WHOLE:
                rows_cap = max(rows_cap, 1)
    rows_cap = int(rows_cap)
    out = {
        "input_ids": np.zeros((rows_cap, width), dtype=np.int64 if spec.flags & BATCH_IDS64 else np.int32),
        "attention_mask": np.zeros((rows_cap, width), dtype=np.uint8),
        "position_ids": np.zeros((rows_cap, width), dtype=np.uint32),
        "sequence_ids": np.zeros((rows_cap, width), dtype=np.int32),
        "sample_ids": np.zeros((rows_cap, width), dtype=np.int32),
        "length": np.zeros(rows_cap, dtype=np.uint32),
        "info": np.zeros(3, dtype=np.uint64),
    }
    if rows_cap == 0 and n_rows == 0:
        return out
    one = np.zeros(4, dtype=np.uint64)  # an output of no row still needs an address
    at = lambda a, typ: C.cast(_vp(a) if a.size else _vp(one), typ)
    check(lib().swt_pack_rows(_cast(ids, u32p), ptr(tok_off, u64p), n_rows, _cast(cmap, u32p), n_map, int(bool(flagged)), C.byref(spec),
                              int(mode), ptr(slot, u64p), ptr(row_first, u64p), rows_cap, at(out["input_ids"], C.c_void_p),
                              at(out["attention_mask"], u8p), at(out["position_ids"], u32p), at(out["sequence_ids"], u32p),
                              at(out["sample_ids"], u32p), at(out["length"], u32p), ptr(out["info"], u64p)))
    return out


def mlm_capacity():
    """-> (cols_per_step, rows_per_wave_max): the columns of a row one step of the masking kernel covers, and the most rows
    that share one of its wavefronts (csrc/swt_mlm.hip)"""
    a, b = C.c_uint32(), C.c_uint32()
    check(lib().swt_mlm_capacity(C.byref(a), C.byref(b)))
    return a.value, b.value


def mlm_spec(n_class, mask_id, select_below, mask_below, random_below, seed=0, epoch=0, whole_word=True, ids64=False):
    """an MlmSpec; the thresholds are integers in [0, 2^32]"""
    return MlmSpec(int(seed), int(select_below), int(mask_below), int(random_below), int(epoch),
                   (MLM_WHOLE_WORD if whole_word else 0) | (MLM_IDS64 if ids64 else 0), int(mask_id), int(n_class))


def mlm_mask(ids, cls_tab, rand_ids, spec, selected=True, info=True):
    """Rows of dense ids (a 2-D C-contiguous int32 or int64 array; the spec's MLM_IDS64 says which) masked for the masked-LM
    objective on the device (swt_mlm_mask).  cls_tab uint8[spec.n_class]; rand_ids uint32 or None.
    -> dict: input_ids and labels as ids, selected uint8 (or None), info uint64[5] (or None): eligible, selected, masked, random, kept."""
    want = np.int64 if spec.flags & MLM_IDS64 else np.int32
    if not isinstance(ids, np.ndarray) or ids.dtype != want or ids.ndim != 2 or not ids.flags.c_contiguous:
        raise TypeError("ids: a 2-D C-contiguous array of %s" % np.dtype(want).name)
    cls_tab = np.ascontiguousarray(cls_tab, dtype=np.uint8)
    if cls_tab.size < spec.n_class:
        raise ValueError("cls_tab holds n_class entries")
    if rand_ids is not None:
        rand_ids = np.ascontiguousarray(rand_ids, dtype=np.uint32)
    rows, width = ids.shape
    out = {"input_ids": np.zeros_like(ids), "labels": np.zeros_like(ids),
           "selected": np.zeros(ids.shape, dtype=np.uint8) if selected else None, "info": np.zeros(5, dtype=np.uint64) if info else None}
    one = np.zeros(4, dtype=np.uint64)  # an array of no element still needs an address
    at = lambda a, typ: None if a is None else C.cast(_vp(a) if a.size else _vp(one), typ)
    check(lib().swt_mlm_mask(at(ids, C.c_void_p), rows, width, at(cls_tab, u8p), at(rand_ids, u32p), 0 if rand_ids is None else int(rand_ids.size),
                             C.byref(spec), at(out["input_ids"], C.c_void_p), at(out["labels"], C.c_void_p), at(out["selected"], u8p),
                             at(out["info"], u64p)))
    return out


DECODE_SKIP_SPECIAL, DECODE_IDS64 = 1, 4  # the flags of swt_decode_*
TOK_GLUE, TOK_NO_SPACE_BEFORE, TOK_NO_SPACE_AFTER, TOK_SPECIAL, TOK_BAD = 1, 2, 4, 8, 16  # the bits of tok_flags
DECODE_BAD_ID, DECODE_BAD_TOKEN = 1, 2  # the bits of a row's status


def decode_capacity():
    """-> (cols_per_step, scan_group): the columns of a row one step of the decode kernel covers, the rows of one scan group of
    its plan (csrc/swt_decode.hip)"""
    a, b = C.c_uint32(), C.c_uint32()
    check(lib().swt_decode_capacity(C.byref(a), C.byref(b)))
    return a.value, b.value


def _decode_args(ids, mask, tok_off, tok_flags, n_tok):
    if not isinstance(ids, np.ndarray) or ids.dtype not in (np.int32, np.int64) or ids.ndim != 2 or not ids.flags.c_contiguous:
        raise TypeError("ids: a 2-D C-contiguous array of int32 or int64")
    if mask is not None:
        mask = np.ascontiguousarray(mask, dtype=np.uint8)
        if mask.shape != ids.shape:
            raise ValueError("mask has the shape of ids")
    tok_off, tok_flags = np.ascontiguousarray(tok_off, dtype=np.uint32), np.ascontiguousarray(tok_flags, dtype=np.uint8)
    if tok_off.size < n_tok + 1 or tok_flags.size < n_tok:
        raise ValueError("tok_off holds n_tok + 1 entries, tok_flags n_tok")
    return mask, tok_off, tok_flags


def decode_plan(ids, mask, tok_off, tok_flags, n_tok, skip_special=True):
    """Rows of dense ids (a 2-D C-contiguous int32 or int64 array) and their mask (uint8 of the same shape, or None) planned for
    decoding (swt_decode_plan) -> (text_off uint64[rows + 1], status uint8[rows], info uint64[3]: total bytes, rows with a
    nonzero status, kept columns)"""
    mask, tok_off, tok_flags = _decode_args(ids, mask, tok_off, tok_flags, n_tok)
    rows, width = ids.shape
    flags = (DECODE_SKIP_SPECIAL if skip_special else 0) | (DECODE_IDS64 if ids.dtype == np.int64 else 0)
    text_off, status, info = np.zeros(rows + 1, dtype=np.uint64), np.zeros(max(rows, 1), dtype=np.uint8), np.zeros(3, dtype=np.uint64)
    one = np.zeros(4, dtype=np.uint64)  # an array of no element still needs an address
    check(lib().swt_decode_plan(_vp(ids) or _vp(one), _vp(mask), rows, width, _vp(tok_off), _vp(tok_flags), n_tok, flags, _vp(text_off),
                                _vp(status), _vp(info)))
    return text_off, status[:rows], info


def decode_rows(ids, mask, tok_bytes, tok_off, tok_flags, n_tok, text_off, skip_special=True, text_cap=None):
    """The bytes of a plan (swt_decode_rows) -> text uint8[text_off[-1]]; text_cap, for the tests, in place of the plan's total"""
    mask, tok_off, tok_flags = _decode_args(ids, mask, tok_off, tok_flags, n_tok)
    tok_bytes, text_off = np.ascontiguousarray(tok_bytes, dtype=np.uint8), np.ascontiguousarray(text_off, dtype=np.uint64)
    rows, width = ids.shape
    if text_off.size != rows + 1:
        raise ValueError("text_off holds rows + 1 entries")
    flags = (DECODE_SKIP_SPECIAL if skip_special else 0) | (DECODE_IDS64 if ids.dtype == np.int64 else 0)
    cap = int(text_off[-1]) if text_cap is None else int(text_cap)
    text = np.zeros(cap, dtype=np.uint8)
    one = np.zeros(4, dtype=np.uint64)
    check(lib().swt_decode_rows(_vp(ids) or _vp(one), _vp(mask), rows, width, _vp(tok_bytes) or _vp(one), _vp(tok_off), _vp(tok_flags), n_tok,
                                flags, _vp(text_off), _vp(text) or _vp(one), cap))
    return text


LABEL_ALL_TOKENS, LABEL_IDS64 = 1, 4  # the flags of swt_label_words; IDS64 also of swt_answer_positions
ANSWER_CLS, ANSWER_PAD_LEFT = 1, 2  # the flags of swt_answer_positions and swt_answer_best
LABEL_IGNORE = -100  # what the Python layer passes as `ignore`
NO_ANSWER = 0xFFFFFFFF  # ans[s, 0] of a text without an answer
LABEL_COUNTS, ANSWER_COUNTS, BEST_COUNTS = 4, 3, 2  # the entries of info of the three calls


def label_capacity():
    """-> (cols_per_step, scan_rows): the columns of a row one step of the label kernels covers, the rows of one workgroup of the
    reduction over a text's rows (csrc/swt_labels.hip)"""
    a, b = C.c_uint32(), C.c_uint32()
    check(lib().swt_label_capacity(C.byref(a), C.byref(b)))
    return a.value, b.value


def _as_u32(a):
    """an array of 32-bit integers as contiguous uint32, whatever its sign (-1 is 0xFFFFFFFF); None stays None"""
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype in (np.int32, np.uint32) else a.astype(np.uint32)


def _label_rows(shape_of, word, seq, sample, spans=None, length=None):
    """the row arrays of the label calls as the C ABI takes them, each held to the shape of `shape_of` [rows, width]"""
    rows, width = shape_of.shape[:2]
    word, sample, spans, length = _as_u32(word), _as_u32(sample), _as_u32(spans), _as_u32(length)
    seq = None if seq is None else np.ascontiguousarray(seq, dtype=np.int8)
    for name, a, shape in (("word", word, (rows, width)), ("seq", seq, (rows, width)), ("sample", sample, (rows,)),
                           ("spans", spans, (rows, width, 2)), ("length", length, (rows,))):
        if a is not None and a.shape != shape:
            raise ValueError("%s has the shape %s, the rows want %s" % (name, a.shape, shape))
    return int(rows), int(width), word, seq, sample, spans, length


_ONE = np.zeros(4, dtype=np.uint64)  # an array of no element still needs an address


def _at(a):
    return None if a is None else _vp(a) if a.size else _vp(_ONE)


def label_words(word, lab_off, lab, seq=None, side=0, sample=None, inside=None, all_tokens=False, ids64=False, ignore=LABEL_IGNORE,
                status=True, info=True):
    """Word labels onto token rows (swt_label_words).  word [rows, width] (int32 or uint32), lab_off uint64[n + 1], lab int32.
    -> dict: labels int32 or int64 [rows, width], status uint8[rows] (or None), info uint64[4] (or None)"""
    if not isinstance(word, np.ndarray) or word.ndim != 2:
        raise TypeError("word: a 2-D array")
    rows, width, word, seq, sample, _, _ = _label_rows(word, word, seq, sample)
    lab_off, lab = np.ascontiguousarray(lab_off, dtype=np.uint64), np.ascontiguousarray(lab, dtype=np.int32)
    if lab_off.size < 1:
        raise ValueError("lab_off holds n_samples + 1 entries")
    inside = None if inside is None else np.ascontiguousarray(inside, dtype=np.int32)
    out = {"labels": np.zeros((rows, width), dtype=np.int64 if ids64 else np.int32), "status": np.zeros(rows, dtype=np.uint8) if status else None,
           "info": np.zeros(LABEL_COUNTS, dtype=np.uint64) if info else None}
    check(lib().swt_label_words(_at(word), _at(seq), int(side), _at(sample), rows, width, _at(lab_off), _at(lab), int(lab.size),
                                int(lab_off.size) - 1, _at(inside), 0 if inside is None else int(inside.size), int(ignore),
                                (LABEL_ALL_TOKENS if all_tokens else 0) | (LABEL_IDS64 if ids64 else 0), _at(out["labels"]), _at(out["status"]),
                                _at(out["info"])))
    return out


def answer_positions(spans, ans, word=None, seq=None, side=0, sample=None, length=None, cls=False, pad_left=False, ids64=False,
                     ignore=LABEL_IGNORE, has=True, hit=True, info=True):
    """Answer character spans to start and end columns (swt_answer_positions).  spans [rows, width, 2], ans uint32[n, 2].
    -> dict: start, end int32 or int64 [rows], has uint8[rows], hit uint8[n], info uint64[3] (each of the last three or None)"""
    if not isinstance(spans, np.ndarray) or spans.ndim != 3:
        raise TypeError("spans: a 3-D array [rows, width, 2]")
    rows, width, word, seq, sample, spans, length = _label_rows(spans, word, seq, sample, spans, length)
    ans = np.ascontiguousarray(ans, dtype=np.uint32).reshape(-1, 2)
    t = np.int64 if ids64 else np.int32
    out = {"start": np.zeros(rows, dtype=t), "end": np.zeros(rows, dtype=t), "has": np.zeros(rows, dtype=np.uint8) if has else None,
           "hit": np.zeros(ans.shape[0], dtype=np.uint8) if hit else None, "info": np.zeros(ANSWER_COUNTS, dtype=np.uint64) if info else None}
    flags = (ANSWER_CLS if cls else 0) | (ANSWER_PAD_LEFT if pad_left else 0) | (LABEL_IDS64 if ids64 else 0)
    check(lib().swt_answer_positions(_at(spans), _at(word), _at(seq), int(side), _at(sample), rows, width, _at(ans), int(ans.shape[0]), _at(length),
                                     int(ignore), flags, _at(out["start"]), _at(out["end"]), _at(out["has"]), _at(out["hit"]), _at(out["info"])))
    return out


BEST_TEXT = (("score", np.float32), ("null_score", np.float32), ("row", np.int32), ("start_col", np.int32), ("end_col", np.int32),
             ("char_start", np.uint32), ("char_end", np.uint32))
BEST_ROW = (("row_score", np.float32), ("row_start", np.int32), ("row_end", np.int32))


def answer_best(start_logit, end_logit, spans, n_samples, word=None, seq=None, side=0, sample=None, max_len=30, length=None, cls=False,
                pad_left=False, per_row=True, info=True):
    """The best span per row and per text from start and end logits (swt_answer_best).  The logits are float32 [rows, width].
    -> dict: per text score, null_score float32, row, start_col, end_col int32, char_start, char_end uint32 [n_samples]; per row
    row_score, row_start, row_end (or None); info uint64[2] (or None)"""
    for name, a in (("start_logit", start_logit), ("end_logit", end_logit)):
        if not isinstance(a, np.ndarray) or a.dtype != np.float32 or a.ndim != 2 or not a.flags.c_contiguous:
            raise TypeError("%s: a 2-D C-contiguous array of float32" % name)
    if end_logit.shape != start_logit.shape:
        raise ValueError("end_logit has the shape of start_logit")
    rows, width, word, seq, sample, spans, length = _label_rows(start_logit, word, seq, sample, spans, length)
    out = {name: np.zeros(int(n_samples), dtype=t) for name, t in BEST_TEXT}
    out.update((name, np.zeros(rows, dtype=t) if per_row else None) for name, t in BEST_ROW)
    out["info"] = np.zeros(BEST_COUNTS, dtype=np.uint64) if info else None
    flags = (ANSWER_CLS if cls else 0) | (ANSWER_PAD_LEFT if pad_left else 0)
    check(lib().swt_answer_best(_at(start_logit), _at(end_logit), _at(spans), _at(word), _at(seq), int(side), _at(sample), rows, width,
                                int(n_samples), int(max_len), _at(length), flags, *[_at(out[name]) for name, _ in BEST_TEXT + BEST_ROW],
                                _at(out["info"])))
    return out


TAG_FIRST, TAG_MEAN, TAG_MAX = 0, 1, 2  # the strategies of swt_word_predict
TAG_STRATEGIES = {"first": TAG_FIRST, "mean": TAG_MEAN, "max": TAG_MAX}
PLAN_COUNTS, PREDICT_COUNTS, ENTITY_COUNTS = 2, 4, 2  # the entries of info of the three calls
WORD_OUT = (("label", np.int32), ("score", np.float32), ("row", np.int32), ("col", np.int32), ("n_tokens", np.int32),
            ("char_start", np.uint32), ("char_end", np.uint32))
ENTITY_OUT = (("text_index", np.int32), ("type", np.int32), ("first_word", np.int32), ("last_word", np.int32), ("char_start", np.uint32),
              ("char_end", np.uint32), ("score", np.float32))


def tag_capacity():
    """-> (cols_per_step, text_rows, scan_words): the columns of a row one step of the tag kernels covers, the rows of one
    workgroup of the reduction over a text's rows, the words of one group of the entity scan (csrc/swt_tags.hip)"""
    a, b, c = C.c_uint32(), C.c_uint32(), C.c_uint32()
    check(lib().swt_tag_capacity(C.byref(a), C.byref(b), C.byref(c)))
    return a.value, b.value, c.value


def word_plan(word, n_samples, seq=None, side=0, sample=None):
    """How many words each text has (swt_word_plan).  word [rows, width] -> (word_off uint64[n_samples + 1], info uint64[2])"""
    if not isinstance(word, np.ndarray) or word.ndim != 2:
        raise TypeError("word: a 2-D array")
    rows, width, word, seq, sample, _, _ = _label_rows(word, word, seq, sample)
    word_off, info = np.zeros(int(n_samples) + 1, dtype=np.uint64), np.zeros(PLAN_COUNTS, dtype=np.uint64)
    check(lib().swt_word_plan(_at(word), _at(seq), int(side), _at(sample), rows, width, int(n_samples), _at(word_off), _at(info)))
    return word_off, info


def word_predict(logits, word, spans, word_off, seq=None, side=0, sample=None, strategy=TAG_FIRST, n_words=None, word_logits=False,
                 info=True):
    """One label and score per word from logits float32 [rows, width, n_labels] (swt_word_predict).  n_words: the capacity of the
    per-word arrays, word_off[-1] by default -> dict: label, score, row, col, n_tokens, char_start, char_end [n_words], logits
    [n_words, n_labels] (or None), info uint64[4] (or None)"""
    if not isinstance(logits, np.ndarray) or logits.dtype != np.float32 or logits.ndim != 3 or not logits.flags.c_contiguous:
        raise TypeError("logits: a 3-D C-contiguous array of float32")
    rows, width, word, seq, sample, spans, _ = _label_rows(logits, word, seq, sample, spans)
    word_off = np.ascontiguousarray(word_off, dtype=np.uint64)
    if word_off.size < 1:
        raise ValueError("word_off holds n_samples + 1 entries")
    n_words = int(word_off[-1]) if n_words is None else int(n_words)
    n_labels = int(logits.shape[2])
    out = {name: np.zeros(n_words, dtype=t) for name, t in WORD_OUT}
    out["logits"] = np.zeros((n_words, n_labels), dtype=np.float32) if word_logits else None
    out["info"] = np.zeros(PREDICT_COUNTS, dtype=np.uint64) if info else None
    check(lib().swt_word_predict(_at(logits), _at(word), _at(seq), int(side), _at(sample), _at(spans), rows, width, n_labels, _at(word_off),
                                 int(word_off.size) - 1, n_words, int(strategy), *[_at(out[name]) for name, _ in WORD_OUT], _at(out["logits"]),
                                 _at(out["info"])))
    return out


def entity_spans(label, score, char_start, char_end, word_off, etype, begins, info=True):
    """The BIO grouping of the words of word_predict (swt_entity_spans) -> dict: text_index, type, first_word, last_word,
    char_start, char_end, score [n_words] (the records at or beyond the count are "nothing"), info uint64[2] (or None)"""
    label, score = np.ascontiguousarray(label, dtype=np.int32), np.ascontiguousarray(score, dtype=np.float32)
    char_start, char_end = _as_u32(char_start), _as_u32(char_end)
    word_off, etype = np.ascontiguousarray(word_off, dtype=np.uint64), np.ascontiguousarray(etype, dtype=np.int32)
    begins = np.ascontiguousarray(begins, dtype=np.uint8)
    n_words = int(label.size)
    if not (score.shape == char_start.shape == char_end.shape == label.shape == (n_words,)) or begins.shape != etype.shape or word_off.size < 1:
        raise ValueError("label, score, char_start and char_end hold one entry per word, etype and begins one per label")
    out = {name: np.zeros(n_words, dtype=t) for name, t in ENTITY_OUT}
    out["info"] = np.zeros(ENTITY_COUNTS, dtype=np.uint64) if info else None
    check(lib().swt_entity_spans(_at(label), _at(score), _at(char_start), _at(char_end), _at(word_off), int(word_off.size) - 1, n_words,
                                 _at(etype), _at(begins), int(etype.size), *[_at(out[name]) for name, _ in ENTITY_OUT], _at(out["info"])))
    return out


FILL_EQUAL, FILL_NOT_EQUAL, FILL_IDS64 = 0, 1, 4  # the modes of swt_mlm_positions, the flag of both calls
POSITION_COUNTS, FILL_COUNTS = 2, 5  # the entries of info of the two calls
FILL_OUT = (("lse", np.float32, False), ("top_id", np.int32, True), ("top_logit", np.float32, True), ("label_id", np.int32, False),
            ("label_logit", np.float32, False), ("label_rank", np.int32, False))  # name, type, [n, k] instead of [n]


def fill_capacity():
    """-> (floats_per_step, positions_per_workgroup, k_max, scan_cells): the floats of a row one step of a wavefront covers, the
    positions of one workgroup of swt_mlm_predict, the greatest k, the cells of one scan group of swt_mlm_positions
    (csrc/swt_fill.hip)"""
    a, b, c, d = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
    check(lib().swt_fill_capacity(C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
    return a.value, b.value, c.value, d.value


def _fill_ids(name, a):
    if not isinstance(a, np.ndarray) or a.dtype not in (np.int32, np.int64) or a.ndim != 2 or not a.flags.c_contiguous:
        raise TypeError("%s: a 2-D C-contiguous array of int32 or int64" % name)
    return int(a.shape[0]), int(a.shape[1]), FILL_IDS64 if a.dtype == np.int64 else 0


def mlm_positions(ids, value, not_equal=False):
    """The flat indices of the cells of ids [rows, width] that equal `value` (or do not), ascending (swt_mlm_positions).
    -> (pos uint64[rows * width], UINT64_MAX from the count on; info uint64[2]: the count, the cells looked at)"""
    rows, width, flags = _fill_ids("ids", ids)
    pos, info = np.zeros(rows * width, dtype=np.uint64), np.zeros(POSITION_COUNTS, dtype=np.uint64)
    check(lib().swt_mlm_positions(_at(ids), rows, width, int(value), FILL_NOT_EQUAL if not_equal else FILL_EQUAL, flags, _at(pos), _at(info)))
    return pos, info


def mlm_predict(logits, pos, labels=None, k=0, lse=True, info=True):
    """The scores of the rows logits[pos[p]] of float32 logits [rows, width, V] (swt_mlm_predict).  -> dict: lse float32[n] (or
    None), top_id int32, top_logit float32 [n, k] (None with k == 0), label_id, label_logit, label_rank [n] (None without labels),
    info uint64[5] (or None)"""
    if not isinstance(logits, np.ndarray) or logits.dtype != np.float32 or logits.ndim != 3 or not logits.flags.c_contiguous:
        raise TypeError("logits: a 3-D C-contiguous array of float32")
    rows, width, n_vocab = (int(x) for x in logits.shape)
    flags = 0
    if labels is not None:
        lr, lw, flags = _fill_ids("labels", labels)
        if (lr, lw) != (rows, width):
            raise ValueError("labels has the shape %s, the logits want %s" % (labels.shape, (rows, width)))
    pos = np.ascontiguousarray(pos, dtype=np.uint64)
    if pos.ndim != 1:
        raise ValueError("pos: a 1-D array of flat cell indices")
    n, k = int(pos.size), int(k)
    wanted = {"lse": lse, "top_id": k > 0, "top_logit": k > 0, "label_id": labels is not None, "label_logit": labels is not None,
              "label_rank": labels is not None}
    out = {name: np.zeros((n, k) if per_k else n, dtype=t) if wanted[name] else None for name, t, per_k in FILL_OUT}
    out["info"] = np.zeros(FILL_COUNTS, dtype=np.uint64) if info else None
    check(lib().swt_mlm_predict(_at(logits), rows, width, n_vocab, _at(pos), n, _at(labels), flags, k,
                                *[_at(out[name]) for name, _, _ in FILL_OUT], _at(out["info"])))
    return out


ADDED_COUNTS = 3  # the entries of info of swt_added_find: matches, texts with a match, bytes blanked


def added_capacity():
    """-> (step_bytes, halo_bytes, tile_bytes, max_patterns, max_pattern_bytes): the bytes of one step of a wavefront's walk
    through a text, the halo staged behind a step, the bytes of a tile, the limits of a handle (csrc/swt_added.hip)"""
    v = [C.c_uint32() for _ in range(5)]
    check(lib().swt_added_capacity(*[C.byref(x) for x in v]))
    return tuple(x.value for x in v)


class AddedPatterns:
    """The patterns of the added tokens (swt_added): `patterns` are bytes objects, lowercased UTF-8.  Needs no device until the
    first find."""

    def __init__(self, patterns):
        self.n = len(patterns)
        blob = np.frombuffer(b"".join(patterns) + b"\0", dtype=np.uint8)
        off = np.zeros(self.n + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(p) for p in patterns], dtype=np.uint64)
        h = C.c_void_p()
        check(lib().swt_added_create(ptr(blob, u8p), ptr(off, u64p), self.n, C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.swt_added_destroy(self._h)
        self._h = None

    __del__ = close

    def find(self, text_u8, sent_off):
        """host buffers in -> (blanked text uint8, m_off uint64[n + 1], m_pat uint32[m], m_span uint32[m, 2], info uint64[3])"""
        n_sent, n_bytes = int(sent_off.size - 1), int(sent_off[-1]) if sent_off.size else 0
        text_u8, sent_off = np.ascontiguousarray(text_u8, dtype=np.uint8), np.ascontiguousarray(sent_off, dtype=np.uint64)
        blank, m_off = np.zeros(max(n_bytes, 1), dtype=np.uint8), np.zeros(n_sent + 1, dtype=np.uint64)
        m_pat, m_span = np.zeros(max(n_bytes, 1), dtype=np.uint32), np.zeros((max(n_bytes, 1), 2), dtype=np.uint32)
        info = np.zeros(ADDED_COUNTS, dtype=np.uint64)
        check(lib().swt_added_find(self._h, ptr(text_u8, u8p), ptr(sent_off, u64p), n_sent, ptr(blank, u8p), ptr(m_off, u64p), ptr(m_pat, u32p),
                                   ptr(m_span, u32p), n_bytes, ptr(info, u64p)))
        m = int(info[0])
        return blank[:n_bytes], m_off, m_pat[:m], m_span[:m], info

    def find_dev(self, d_text, n_bytes, d_off, n_sent, d_out_text, d_m_off, d_m_pat, d_m_span, d_info, stream=0):
        """device pointers (ints) in; enqueues on `stream` and returns"""
        check(lib().swt_added_find_dev(self._h, d_text, n_bytes, d_off, n_sent, d_out_text, d_m_off, d_m_pat, d_m_span, d_info, stream))


def added_splice(ids, tok_off, spans, word, m_off, m_pat, m_span, added_base):
    """The matches of AddedPatterns.find into the streams of a span call over the blanked text (swt_added_splice)
    -> (ids uint32, tok_off uint64[n + 1], spans uint32[n, 2], word uint32[n])"""
    ids, word, m_pat = (np.ascontiguousarray(a, dtype=np.uint32) for a in (ids, word, m_pat))
    spans, m_span = (np.ascontiguousarray(a, dtype=np.uint32).reshape(-1, 2) for a in (spans, m_span))
    tok_off, m_off = np.ascontiguousarray(tok_off, dtype=np.uint64), np.ascontiguousarray(m_off, dtype=np.uint64)
    n_sent = int(tok_off.size - 1)
    n = int(ids.size + m_pat.size)
    out_ids, out_off = np.zeros(max(n, 1), dtype=np.uint32), np.zeros(n_sent + 1, dtype=np.uint64)
    out_spans, out_word = np.zeros((max(n, 1), 2), dtype=np.uint32), np.zeros(max(n, 1), dtype=np.uint32)
    check(lib().swt_added_splice(ptr(ids, u32p), ptr(tok_off, u64p), ptr(spans, u32p), ptr(word, u32p), n_sent, ptr(m_off, u64p),
                                 ptr(m_pat, u32p), ptr(m_span, u32p), int(added_base), ptr(out_ids, u32p), ptr(out_off, u64p),
                                 ptr(out_spans, u32p), ptr(out_word, u32p)))
    return out_ids[:n], out_off, out_spans[:n], out_word[:n]


def bpe_length_table(strings):
    """The length table of a BPE id stream: code points of every interned symbol string (len_base = SYM_BASE, flagged = 1)."""
    return np.fromiter(map(len, strings), dtype=np.uint32, count=len(strings))


def wp_length_table(tokens):
    """The length table of a NaiveWP id stream over `tokens` = sorted(vocab): code points after the '##' with SPAN_LEN_CONT on the
    '##' tokens, then SPAN_WHOLE_WORD for n_vocab ("['UNK']") and n_vocab + 1 ("[UNK]") (len_base = 0, flagged = 0)."""
    out = np.zeros(len(tokens) + 2, dtype=np.uint32)
    for i, tok in enumerate(tokens):
        out[i] = (len(tok) - 2) | SPAN_LEN_CONT if tok.startswith("##") else len(tok)
    return out


def _encode_out(n_ids, n_sent, status):
    """the outputs every host encode fills: room for n_ids ids, the offsets, the statuses (or None) and the id count"""
    return (np.empty(max(n_ids, 1), dtype=np.uint32), np.zeros(n_sent + 1, dtype=np.uint64),
            np.zeros(max(n_sent, 1), dtype=np.uint8) if status else None, C.c_uint64())


def _encode_host(entry, handle, text_u8, sent_off, status=False, flags=None, spans=None, draw=()):
    """One host-buffer encode of include/swt.h: lowercased packed text and its offsets in, arrays trimmed to the id count out
    -> (ids uint32, offsets uint64[n+1]), then status uint8[n] for an entry that has per-sentence statuses, then (spans
    uint32[n, 2], word uint32[n]) for one that takes a span flag word (`spans`).  flags: the trailing flag word of the BPE entries;
    draw: (drop_below, seed, epoch) behind it, for the dropout entry."""
    n_sent = int(sent_off.size - 1)
    out, out_off, st, nt = _encode_out(int(sent_off[-1]), n_sent, status)
    args = [handle, ptr(text_u8, u8p), ptr(sent_off, u64p), n_sent, ptr(out, u32p), out.size, ptr(out_off, u64p)]
    args += [ptr(st, u8p), C.byref(nt)] if status else [C.byref(nt)]
    if flags is not None:
        args.append(flags)
    args += draw
    if spans is not None:
        sp, word = np.zeros((out.size, 2), dtype=np.uint32), np.zeros(out.size, dtype=np.uint32)
        args += [spans, ptr(sp, u32p), ptr(word, u32p)]
    check(getattr(lib(), entry)(*args))
    n = nt.value
    return (out[:n], out_off) + ((st[:n_sent],) if status else ()) + ((sp[:n], word[:n]) if spans is not None else ())


def _encode_joined(entry, handle, joined, n_sent, status=False, flags=None):
    """The same for the `_joined` entries: join_texts' bytes in (not lowercased), the prepared text staying on the device;
    None when a sentence needs the host's str.lower() (the entry leaves UINT64_MAX for the count)."""
    out, out_off, st, nt = _encode_out(int(joined.size), n_sent, status)
    need = np.zeros(max(n_sent, 1), dtype=np.uint8)
    args = [handle, ptr(joined, u8p), int(joined.size), n_sent, ptr(out, u32p), out.size, ptr(out_off, u64p)]
    args += [ptr(st, u8p), C.byref(nt), ptr(need, u8p)] if status else [C.byref(nt), ptr(need, u8p)]
    if flags is not None:
        args.append(flags)
    check(getattr(lib(), entry)(*args))
    if nt.value == 0xFFFFFFFFFFFFFFFF:
        return None
    return (out[:nt.value], out_off) + ((st[:n_sent],) if status else ())


class BpeTable:
    """Device merge-rank table (swt_bpe_table)."""

    def __init__(self, left, right, merged):
        left = np.ascontiguousarray(left, dtype=np.uint32)
        right = np.ascontiguousarray(right, dtype=np.uint32)
        merged = np.ascontiguousarray(merged, dtype=np.uint32)
        self.n_merges = int(left.size)
        h = C.c_void_p()
        check(lib().swt_bpe_table_create(ptr(left, u32p), ptr(right, u32p), ptr(merged, u32p), self.n_merges, C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.swt_bpe_table_destroy(self._h)
        self._h = None

    __del__ = close

    def set_option(self, option, value):
        check(lib().swt_bpe_table_set_option(self._h, option, value))

    def order_equivalent(self):
        """True when NaiveBPE's list order and FastBPE's lowest rank first cannot differ on this table (no pair listed twice,
        every pair above the merges that produce its symbols): encode_naive* then run the FastBPE kernels"""
        fn = lib().swt_debug_bpe_table_info
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int]
        return fn(self._h, 5) == 1

    def encode(self, text_u8, sent_off, flags=0, _entry="swt_bpe_encode"):
        """host buffers in -> (ids uint32, offsets uint64[n+1])"""
        return _encode_host(_entry, self._h, text_u8, sent_off, flags=flags)

    def encode_joined(self, joined, n_sent, flags=0, _entry="swt_bpe_encode_joined"):
        """join_texts' bytes in (not lowercased) -> (ids, offsets), the prepared text staying on the device; None when a sentence
        needs the host's str.lower() (the caller goes pack_and_lower -> encode)"""
        return _encode_joined(_entry, self._h, joined, n_sent, flags=flags)

    def encode_dev(self, d_text, n_bytes, d_off, n_sent, d_out, d_out_off, d_ntok, flags=0, stream=0):
        """device pointers (ints) in; enqueues on `stream` and returns"""
        check(lib().swt_bpe_encode_dev(self._h, d_text, n_bytes, d_off, n_sent, d_out, d_out_off, d_ntok, flags, stream))

    # BPE-dropout (swt_bpe_encode_dropout, include/swt.h): draw = (drop_below in [0, 2^32], seed, epoch)
    def encode_dropout(self, text_u8, sent_off, draw, flags=0):
        return _encode_host("swt_bpe_encode_dropout", self._h, text_u8, sent_off, flags=flags, draw=list(draw))

    def encode_dropout_dev(self, d_text, n_bytes, d_off, n_sent, d_out, d_out_off, d_ntok, draw, flags=0, stream=0):
        check(lib().swt_bpe_encode_dropout_dev(self._h, d_text, n_bytes, d_off, n_sent, d_out, d_out_off, d_ntok, flags, *draw, stream))

    # the merges in LIST order (NaiveBPE.encode_word, bpe.py:114-134): same arguments and results as the three above
    def encode_naive(self, text_u8, sent_off, flags=0):
        return self.encode(text_u8, sent_off, flags, _entry="swt_bpe_encode_naive")

    def encode_naive_joined(self, joined, n_sent, flags=0):
        return self.encode_joined(joined, n_sent, flags, _entry="swt_bpe_encode_naive_joined")

    def encode_naive_dev(self, d_text, n_bytes, d_off, n_sent, d_out, d_out_off, d_ntok, flags=0, stream=0):
        check(lib().swt_bpe_encode_naive_dev(self._h, d_text, n_bytes, d_off, n_sent, d_out, d_out_off, d_ntok, flags, stream))


class WpTrie:
    """Flattened failure-link trie (swt_wp_trie)."""

    def __init__(self, vocab_list):
        self.n_vocab = len(vocab_list)
        blob, off = pack_utf32(list(vocab_list))
        h = C.c_void_p()
        check(lib().swt_wp_trie_create(ptr(blob, u32p) if blob.size else None, ptr(off, u64p), self.n_vocab, C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.swt_wp_trie_destroy(self._h)
        self._h = None

    __del__ = close

    def set_option(self, option, value):
        check(lib().swt_wp_trie_set_option(self._h, option, value))

    def stats(self):
        a, b, c = C.c_uint32(), C.c_uint32(), C.c_uint32()
        check(lib().swt_wp_trie_stats(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return {"nodes": a.value, "edges": b.value, "pops": c.value}

    def corner(self):
        """ids of NaiveWP.encode_word("##"), or None when the reference never returns from it"""
        buf = np.zeros(64, dtype=np.uint32)
        n = lib().swt_wp_trie_corner(self._h, ptr(buf, u32p), buf.size)
        if n > buf.size:
            buf = np.zeros(n, dtype=np.uint32)
            n = lib().swt_wp_trie_corner(self._h, ptr(buf, u32p), buf.size)
        return None if n < 0 else buf[:n].copy()

    def node(self, path):
        """(node_id, link, is_end, pops) of the node spelled by `path`, or None"""
        a, _ = pack_utf32([path])
        nid, link, end, npops = C.c_uint32(), C.c_int32(), C.c_uint8(), C.c_uint32()
        pops = np.zeros(256, dtype=np.uint32)
        rc = lib().swt_wp_trie_node(self._h, ptr(a, u32p) if a.size else None, a.size, C.byref(nid), C.byref(link),
                                    C.byref(end), ptr(pops, u32p), pops.size, C.byref(npops))
        if rc == ERR_INVALID:
            return None
        check(rc)
        return nid.value, link.value, bool(end.value), pops[:npops.value].copy()

    def node_path(self, node_id):
        buf = np.zeros(512, dtype=np.uint32)
        n = C.c_uint64()
        check(lib().swt_wp_trie_node_path(self._h, node_id, ptr(buf, u32p), buf.size, C.byref(n)))
        return bytes(buf[:n.value]).decode("utf-32-le", "surrogatepass")

    def encode(self, text_u8, sent_off):
        return _encode_host("swt_wp_encode", self._h, text_u8, sent_off, status=True)

    def encode_joined(self, joined, n_sent):
        """join_texts' bytes in (not lowercased) -> (ids, offsets, status), or None when a sentence needs the host's str.lower()"""
        return _encode_joined("swt_wp_encode_joined", self._h, joined, n_sent, status=True)

    def encode_dev(self, d_text, n_bytes, d_off, n_sent, d_out, d_out_off, d_status, d_ntok, stream=0):
        check(lib().swt_wp_encode_dev(self._h, d_text, n_bytes, d_off, n_sent, d_out, d_out_off, d_status, d_ntok, stream))

    def encode_spans(self, text_u8, sent_off, codepoints=True):
        """encode() with, per token, where it came from (swt_wp_encode_spans) -> (ids, offsets, status, spans uint32[n, 2] = start
        and end inside the sentence in code points or bytes, word uint32[n] = index of the token's segment among those of its
        sentence that emit a token)"""
        return _encode_host("swt_wp_encode_spans", self._h, text_u8, sent_off, status=True, spans=SPAN_CODEPOINTS if codepoints else 0)

    def encode_spans_dev(self, d_text, n_bytes, d_off, n_sent, d_out, d_out_off, d_status, d_ntok, d_spans, d_word, codepoints=True,
                         stream=0):
        check(lib().swt_wp_encode_spans_dev(self._h, d_text, n_bytes, d_off, n_sent, d_out, d_out_off, d_status, d_ntok,
                                            SPAN_CODEPOINTS if codepoints else 0, d_spans, d_word, stream))

    @staticmethod
    def encode_spans_capacity():
        """-> (block, chunk, tile, direct_bytes, direct_sents): the sizes at which the spans call changes form (include/swt.h)"""
        v = [C.c_uint32() for _ in range(5)]
        check(lib().swt_wp_encode_spans_capacity(*[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def encode_naive(self, text_u8, sent_off):
        """NaiveWP.tokenize over lowercased packed text -> (ids, offsets, status)"""
        return _encode_host("swt_wp_encode_naive", self._h, text_u8, sent_off, status=True)

    def encode_naive_joined(self, joined, n_sent):
        """join_texts' bytes in (not lowercased) -> (ids, offsets, status), or None when a sentence needs the host's str.lower()"""
        return _encode_joined("swt_wp_encode_naive_joined", self._h, joined, n_sent, status=True)

    def encode_naive_dev(self, d_text, n_bytes, d_off, n_sent, d_out, d_out_off, d_status, d_ntok, stream=0):
        check(lib().swt_wp_encode_naive_dev(self._h, d_text, n_bytes, d_off, n_sent, d_out, d_out_off, d_status, d_ntok, stream))

    # MaxMatch-Dropout (swt_wp_encode_naive_dropout, include/swt.h): draw = (drop_below in [0, 2^32], seed, epoch)
    def encode_naive_dropout(self, text_u8, sent_off, draw):
        return _encode_host("swt_wp_encode_naive_dropout", self._h, text_u8, sent_off, status=True, draw=list(draw))

    def encode_naive_dropout_dev(self, d_text, n_bytes, d_off, n_sent, d_out, d_out_off, d_status, d_ntok, draw, stream=0):
        check(lib().swt_wp_encode_naive_dropout_dev(self._h, d_text, n_bytes, d_off, n_sent, d_out, d_out_off, d_status, d_ntok, *draw,
                                                    stream))


class BpeTrainer:
    """Device BPE trainer (swt_bpe_trainer): histogram + argmax + merge-apply."""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def from_text(cls, text_u8, sent_off):
        h = C.c_void_p()
        n_sent = int(sent_off.size - 1)
        check(lib().swt_bpe_train_create_text(ptr(text_u8, u8p), ptr(sent_off, u64p), n_sent, C.byref(h)))
        return cls(h)

    @classmethod
    def from_texts(cls, texts, joined=None, wordpiece=False):
        """list[str] -> trainer, the prepared text never leaving the device (swt_bpe_train_create_joined); None when the texts do
        not lend themselves to it (few of them, a U+0000 inside, a code point only the host lowercases): the caller then goes
        pack_and_lower -> from_text.  joined: join_texts(texts), if the caller has it already."""
        n = len(texts)
        if n <= 64 or not device_lower_ok():
            return None
        joined, n_nul = joined if joined is not None else join_texts(texts, "Corpus must be a list of strings.")
        if joined.size + 1 == n or n_nul:
            return None
        need = np.zeros(n, dtype=np.uint8)
        h = C.c_void_p()
        create = lib().swt_wp_train_create_joined if wordpiece else lib().swt_bpe_train_create_joined
        check(create(ptr(joined, u8p), int(joined.size), n, ptr(need, u8p), C.byref(h)))
        return cls(h) if h.value else None

    @classmethod
    def from_text_wordpiece(cls, text_u8, sent_off):
        """NaiveWP.train's state (wordpiece.py:44-63): '##' symbols, likelihood score; `count` outputs = score bit patterns"""
        h = C.c_void_p()
        n_sent = int(sent_off.size - 1)
        check(lib().swt_wp_train_create_text(ptr(text_u8, u8p), ptr(sent_off, u64p), n_sent, C.byref(h)))
        return cls(h)

    @classmethod
    def from_words(cls, syms, word_off, freq):
        syms = np.ascontiguousarray(syms, dtype=np.uint32)
        word_off = np.ascontiguousarray(word_off, dtype=np.uint64)
        freq = np.ascontiguousarray(freq, dtype=np.uint32)
        h = C.c_void_p()
        check(lib().swt_bpe_train_create_words(ptr(syms, u32p), ptr(word_off, u64p), ptr(freq, u32p), int(word_off.size - 1),
                                               C.byref(h)))
        return cls(h)

    def close(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.swt_bpe_train_destroy(self._h)
        self._h = None

    __del__ = close

    def set_pos_base(self, base):
        check(lib().swt_bpe_train_set_pos_base(self._h, base))

    def info(self):
        a, b, c, d = C.c_uint64(), C.c_uint64(), C.c_uint32(), C.c_uint64()
        check(lib().swt_bpe_train_info(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return {"n_words": a.value, "n_symbols": b.value, "n_base_symbols": c.value, "n_pairs": d.value}

    def base_symbols(self):
        n = self.info()["n_base_symbols"]
        out = np.zeros(max(n, 1), dtype=np.uint32)
        check(lib().swt_bpe_train_base_symbols(self._h, ptr(out, u32p), out.size))
        return out[:n]

    def best(self):
        """-> (left, right, count, n_tied, first_pos)"""
        l, r = C.c_uint32(), C.c_uint32()
        cnt, tied, pos = C.c_uint64(), C.c_uint64(), C.c_uint64()
        check(lib().swt_bpe_train_best(self._h, C.byref(l), C.byref(r), C.byref(cnt), C.byref(tied), C.byref(pos)))
        return l.value, r.value, cnt.value, tied.value, pos.value

    def apply(self, left, right, merged):
        check(lib().swt_bpe_train_apply(self._h, left, right, merged))

    def run(self, max_steps, first_merged):
        """device-driven steps -> (left uint32[n], right uint32[n], count uint64[n]); n < max_steps: no pair was left"""
        left = np.zeros(max(max_steps, 1), dtype=np.uint32)
        right = np.zeros(max(max_steps, 1), dtype=np.uint32)
        count = np.zeros(max(max_steps, 1), dtype=np.uint64)
        n = C.c_uint32()
        check(lib().swt_bpe_train_run(self._h, max_steps, first_merged, ptr(left, u32p), ptr(right, u32p), ptr(count, u64p),
                                      C.byref(n)))
        return left[:n.value], right[:n.value], count[:n.value]

    def export(self):
        inf = self.info()
        syms = np.zeros(max(inf["n_symbols"], 1), dtype=np.uint32)
        woff = np.zeros(inf["n_words"] + 1, dtype=np.uint64)
        freq = np.zeros(max(inf["n_words"], 1), dtype=np.uint32)
        check(lib().swt_bpe_train_export(self._h, ptr(syms, u32p), syms.size, ptr(woff, u64p), ptr(freq, u32p)))
        return syms[:int(woff[-1])], woff, freq[:inf["n_words"]]

    def histogram(self):
        cap = max(self.info()["n_pairs"], 1) + 16
        keys = np.zeros(cap, dtype=np.uint64)
        cnts = np.zeros(cap, dtype=np.uint64)
        n = C.c_uint64()
        check(lib().swt_bpe_train_histogram(self._h, ptr(keys, u64p), ptr(cnts, u64p), cap, C.byref(n)))
        return keys[:n.value], cnts[:n.value]

    def step_trace(self):
        """uint64[n_merges, 4]: winning count, pairs tied at it, candidate list length, live symbols before the merge"""
        n = C.c_uint64()
        check(lib().swt_bpe_train_trace(self._h, None, 0, C.byref(n)))
        rows = np.zeros((max(n.value, 1), 4), dtype=np.uint64)
        check(lib().swt_bpe_train_trace(self._h, ptr(rows, u64p), n.value, C.byref(n)))
        return rows[:n.value]

    def stats(self):
        out = np.zeros(11, dtype=np.uint64)
        check(lib().swt_bpe_train_stats(self._h, ptr(out, u64p), 11))
        names = ("replans", "theta", "candidates", "index_entries", "table_slots", "flags", "steps", "keys", "entries_scanned", "tie_words",
                 "squeezes")
        return dict(zip(names, map(int, out)))


class Dist:
    """Communicator of corpus-sharded training (swt_dist): RCCL between processes (one per GPU), or a loop-back whose ranks
    are all trainers of this process (one-GPU tests)."""

    def __init__(self, handle, rank, world, local):
        self._h, self.rank, self.world, self.local = handle, rank, world, local

    @staticmethod
    def unique_id():
        """128 bytes made by rank 0 (ncclGetUniqueId); hand them to every rank"""
        buf = np.zeros(128, dtype=np.uint8)
        check(lib().swt_dist_unique_id(ptr(buf, u8p)))
        return buf

    @classmethod
    def rccl(cls, rank, world, unique_id):
        uid = np.ascontiguousarray(unique_id, dtype=np.uint8)
        h = C.c_void_p()
        check(lib().swt_dist_init(rank, world, ptr(uid, u8p), C.byref(h)))
        return cls(h, rank, world, False)

    @classmethod
    def loopback(cls, world):
        h = C.c_void_p()
        check(lib().swt_dist_init_local(world, C.byref(h)))
        return cls(h, 0, world, True)

    def close(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.swt_dist_destroy(self._h)
        self._h = None

    __del__ = close

    def _handles(self, trainers):
        arr = (C.c_void_p * len(trainers))(*[t._h for t in trainers])
        return C.cast(arr, vpp), arr

    def shard_begin(self, trainers):
        """-> the distinct initial symbols of the whole corpus (uint32, ascending)"""
        hp, keep = self._handles(trainers)
        out = np.zeros(0x110000 + 4096, dtype=np.uint32)
        n = C.c_uint32()
        check(lib().swt_bpe_train_shard_begin(hp, len(trainers), self._h, ptr(out, u32p), out.size, C.byref(n)))
        return out[:n.value].copy()

    def run(self, trainers, max_steps, first_merged):
        """-> (left, right, count) of the merges done (fewer than max_steps: no pair was left)"""
        hp, keep = self._handles(trainers)
        left = np.zeros(max(max_steps, 1), dtype=np.uint32)
        right = np.zeros(max(max_steps, 1), dtype=np.uint32)
        count = np.zeros(max(max_steps, 1), dtype=np.uint64)
        n = C.c_uint32()
        check(lib().swt_bpe_train_run_sharded(hp, len(trainers), self._h, max_steps, first_merged, ptr(left, u32p), ptr(right, u32p),
                                              ptr(count, u64p), C.byref(n)))
        return left[:n.value], right[:n.value], count[:n.value]
