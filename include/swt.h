/*
 * include/swt.h -- C ABI of libswt_hip.so: the MI355X (gfx950) subword-tokenizer hot path.
 *
 * The reference (phtryll/subword-tokenizers) is pure Python and has NO FFI/plugin boundary of its own; the
 * drop-in boundary is its Python class surface.  This header is the C ABI a
 * maintainer binds underneath those classes (ctypes stub in INTEGRATION.md).  Each entry point names
 * the reference lines whose inner loop it replaces; citations are relative to /root/reference.
 *
 * Conventions
 *   - every function returns an int status: 0 = SWT_OK, negative = error (swt_last_error() has text);
 *     nothing throws, aborts or falls back to a CPU path: if the HIP runtime or the device is missing
 *     the call fails with SWT_ERR_NO_DEVICE.
 *   - handles are opaque; buffers are caller-owned; sizes are in elements of the pointed-to type.
 *   - text is UTF-8 of the ALREADY LOWERCASED string (Python str.lower() stays with the caller:
 *     source/utils.py:27, source/wordpiece.py:248), sentences concatenated, with n_sent+1 byte offsets.
 *     Lone surrogates encoded "surrogatepass"-style are accepted and decoded as their code point.
 *   - `_dev` entry points take DEVICE pointers (e.g. torch tensors' data_ptr()) and a hipStream_t passed
 *     as void* (NULL = default stream); they enqueue work and return without synchronising.
 *   - a handle may be used by one host thread at a time.
 *
 * Token ids
 *   BPE:  symbol id = the code point for a one-code-point symbol, else 0x110000 + k, where k is the
 *         caller's interning index of the merged string (symbols are identified by their STRING,
 *         source/bpe.py:41,103,227-228).  Token id = symbol id | SWT_BPE_CONT for every token after the
 *         first of its word (the '##' prefix of source/bpe.py:240-241).
 *   WP:   index into the vocabulary list given to swt_wp_trie_create; n_vocab = "['UNK']"
 *         (source/wordpiece.py:257); n_vocab+1 = "[UNK]" (source/wordpiece.py:149); n_vocab+2 =
 *         SWT_WP corner marker, emitted when NaiveWP.encode_word("##") (source/wordpiece.py:260-261)
 *         yields more than one token -- the caller substitutes the list it got from swt_wp_trie_corner.
 */
#ifndef SWT_H
#define SWT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SWT_OK 0
#define SWT_ERR_NO_DEVICE (-1)    /* no HIP device / runtime */
#define SWT_ERR_INVALID (-2)      /* bad argument */
#define SWT_ERR_CAPACITY (-3)     /* caller buffer too small; the needed size is reported */
#define SWT_ERR_HIP (-4)          /* a HIP call failed */
#define SWT_ERR_UNSUPPORTED (-5)
#define SWT_ERR_STATE (-6)        /* call out of order, or an internal capacity check failed (the handle is unusable) */
#define SWT_ERR_NOMEM (-7)        /* host memory exhausted (std::bad_alloc / std::length_error inside the library) */
#define SWT_ERR_INTERNAL (-8)     /* any other C++ exception stopped at the ABI boundary */

#define SWT_SYM_BASE 0x110000u
#define SWT_BPE_CONT 0x80000000u

/* per-sentence status of the WordPiece encoder */
#define SWT_WP_OK 0
#define SWT_WP_NONTERMINATING 1   /* the reference loops forever on this input */
#define SWT_WP_INDEXERROR 2       /* the reference raises IndexError (source/wordpiece.py:285, i == len) */

const char *swt_last_error(void);
int swt_version(void);
/* The contract above, testable without a GPU: raises a C++ exception of the given kind inside the library (1 std::bad_alloc,
 * 2 std::length_error, 3 std::runtime_error, 4 a non-std object) and returns what the ABI's exception barrier made of it
 * (SWT_ERR_NOMEM, SWT_ERR_NOMEM, SWT_ERR_INTERNAL, SWT_ERR_INTERNAL; swt_last_error() names the exception).  0: SWT_OK. */
int swt_abi_selftest(int kind);
/* Selects the HIP device for this process (one process per GPU).  Fails loudly without a GPU. */
int swt_init(int device_ordinal);
int swt_device_count(void);
/* multiprocessor count / name of the selected device (for launch sizing and reports) */
int swt_device_info(int *n_cu, char *name, size_t name_cap);

/* Kernel timing for bench.py's roofline line (state of the CALLING THREAD, like the error text).  on = 1: every launch of a path's DOMINANT kernel (bpe_lane_kernel,
 * wp_encode_kernel, the training apply/argmax pair) is bracketed by two HIP events on the stream it is launched on;
 * on = 2: the bracket spans all kernels of one call instead (first launch .. last launch); 0 = off.
 * on = 3 (a diagnostic): the bracket is the first kernel of the word-level dedup's front half alone (wordref_kernel), and nothing
 * else is bracketed, so the number of brackets is the number of dedup pipelines that ran on this thread: one per FastBPE or
 * FastWP encode call that took the dedup path, none for a call that went the direct way.
 * swt_profile_read waits for the events, returns the summed elapsed milliseconds and the number of brackets since
 * the last read, and clears the list. */
int swt_profile_enable(int on);
int swt_profile_read(double *ms_total, uint64_t *n_launches);

/* str.lower() on the device for the code points it maps one-to-one at equal UTF-8 length (the
 * reference lowercases on the host: source/utils.py:27 via preprocessing, source/wordpiece.py:248).  The text is rewritten
 * in place; need_host[s] = 1 marks a sentence that holds one of the 26 code points the device leaves alone (a lowercase of
 * another UTF-8 length or of several code points, or U+03A3 whose lowercase depends on its neighbours): the caller
 * lowercases THAT sentence on the host.  swt_lower_of: the table itself (0xFFFFFFFF = host only), for tests. */
uint32_t swt_lower_of(uint32_t cp);
/* The Unicode database the lowercase and class tables were generated from ("13.0.0"): a host whose own str.lower() follows
 * another version must lowercase every batch itself (swt_*_encode on its own text), or small and large batches disagree. */
const char *swt_unidata_version(void);
int swt_utf8_lower(uint8_t *text, const uint64_t *sent_off, uint64_t n_sent, uint8_t *need_host);
/* The same for a host that only knows its sentences' lengths in CODE POINTS (Python: "".join(texts).encode() and len(str)
 * are cheap, every string's byte length is not): text = well-formed UTF-8 of all sentences joined, cp_off[n_sent + 1] =
 * running code-point counts.  Writes byte_off[n_sent + 1] (a code point starts at every byte that is not a continuation
 * byte), lowercases in place and flags as above. */
int swt_utf8_prepare(uint8_t *text, uint64_t n_bytes, const uint64_t *cp_off, uint64_t n_sent, uint64_t *byte_off, uint8_t *need_host);
/* And for a host that knows nothing but the strings (Python: "\0".join(texts).encode(), and one bytes.count to make sure the
 * texts hold no U+0000 of their own): joined = the sentences with ONE zero byte between neighbours (n_joined bytes, exactly
 * n_sent - 1 of them zero).  Writes the text without the separators (n_joined - (n_sent - 1) bytes, lowercased as above) to
 * text_out, byte_off[n_sent + 1] and the flags.  SWT_ERR_INVALID when the separators do not add up. */
int swt_utf8_prepare_joined(const uint8_t *joined, uint64_t n_joined, uint64_t n_sent, uint8_t *text_out, uint64_t *byte_off,
                            uint8_t *need_host);
int swt_utf8_lower_dev(uint8_t *d_text, uint64_t n_bytes, const uint64_t *d_sent_off, uint64_t n_sent, uint8_t *d_need_host,
                       void *stream);

/* Per-handle options of the two encoders (swt_bpe_table_set_option / swt_wp_trie_set_option).  Every choice gives the same
 * output; they pick the path, for tests and measurements.
 *   SWT_OPT_DEDUP             0 (default): batches above a size threshold encode each DISTINCT word once (word-level dedup);
 *                             1: never; 2: always
 *   SWT_OPT_DEDUP_TABLE_BITS  log2 of the dedup word table's slots, 4..24; 0 (default): sized from the batch.  A tiny table
 *                             makes words overflow into their own slots; results stay exact
 *   SWT_OPT_UNIQUE_TILE       (FastBPE) tile size of the pass over the unique words: 0 (default), 64, 128 or 256
 *   SWT_OPT_LANE_SPAN         (FastBPE) consecutive tiles one wavefront of the direct path takes: 0 (default: one) or 1..16.
 *                             A span above one keeps tiles of one size, whatever SWT_OPT_LANE_TAPER says
 *   SWT_OPT_LANE_TAPER        (FastBPE) tile sizes of the direct path, falling from 384 to 128 bytes towards the end of the text so
 *                             that the wavefronts started last are short: 0 (default): the library's choice (its own factor, and
 *                             tiles of one size for a text that does not fill the device's slots twice); 1: tiles of one size;
 *                             v = 2..64: a tile is the largest of 384, 256, 192, 128 bytes that is no more than the bytes still
 *                             to be handed out / (v / 8 x the wavefront slots of the device); v + 256: the same with 192 bytes
 *                             as the smallest size
 *   SWT_OPT_LANE_SLOTS        (FastBPE) the wavefront slots SWT_OPT_LANE_TAPER counts with: 0 (default): those of the device;
 *                             1..1048576: that many, so that a text of a few KiB walks through every tile size
 *   SWT_OPT_LANE_NARROW       (FastBPE) the direct path of a table below 32 k symbols keeps 16-bit symbol codes on chip and takes
 *                             512-byte tiles at the top instead of 384: 0 (default): for a text that fills the device's slots
 *                             with 384-byte tiles once, tapering from there up; the 512-byte tiles in the library's own
 *                             geometry only (a SWT_OPT_LANE_TAPER or SWT_OPT_LANE_SPAN that is set counts from 384); 1: never;
 *                             2: at every size (tiles of one size under that floor), and the tile sizes fall from 512 under a
 *                             set SWT_OPT_LANE_TAPER / SWT_OPT_LANE_SPAN too */
#define SWT_OPT_DEDUP 1
#define SWT_OPT_DEDUP_TABLE_BITS 2
#define SWT_OPT_UNIQUE_TILE 3
#define SWT_OPT_LANE_SPAN 4
#define SWT_OPT_LANE_TAPER 5
#define SWT_OPT_LANE_SLOTS 6
#define SWT_OPT_LANE_NARROW 7

/* Code-point classes compiled into the library (fixture data probed from the wheel/interpreter the
 * reference runs on; tools/gen_unicode_tables.py).  bit0 pre-tokenizer whitespace, bit1 pre-tokenizer
 * punctuation (source/utils.py:27), bit2 str.isspace, bit3 str.isalnum (source/wordpiece.py:285-288). */
#define SWT_CLS_BERT_WS 1u
#define SWT_CLS_BERT_PUNCT 2u
#define SWT_CLS_PY_SPACE 4u
#define SWT_CLS_PY_ALNUM 8u
unsigned swt_class_of(uint32_t code_point);

/* ------------------------------------------------------------------------------------------------
 * FastBPE encode: replaces FastBPE.load_resources' rank dict (source/bpe.py:251-257, :200) and the
 * per-sentence loop FastBPE.tokenize -> encode_word (source/bpe.py:245-249, 205-243) including the
 * pre-tokenizer split of SubwordTokenizer.preprocessing (source/utils.py:26-29).
 */
typedef struct swt_bpe_table swt_bpe_table;

/* merges in list order as symbol-id triples; for swt_bpe_encode* a later duplicate (left,right) overrides an earlier one
 * (dict semantics of source/bpe.py:257), for swt_bpe_encode_naive* every position counts (list semantics of
 * source/bpe.py:126-127). */
int swt_bpe_table_create(const uint32_t *left, const uint32_t *right, const uint32_t *merged,
                         uint32_t n_merges, swt_bpe_table **out);
void swt_bpe_table_destroy(swt_bpe_table *t);
int swt_bpe_table_set_option(swt_bpe_table *t, int option, int value);

/* Host-buffer form: copies in, encodes on the device, copies out.
 *   text[n_bytes], sent_off[n_sent+1] -> out_ids[<= out_cap], out_off[n_sent+1], *n_tokens
 * out_cap >= n_bytes is always sufficient (every token covers at least one byte). */
#define SWT_BPE_RAW_WORDS 1u   /* flags: every "sentence" is ONE word, no pre-tokenizer split -- this is
                                  FastBPE.encode_word(word) (source/bpe.py:205), batched */
#define SWT_BPE_NO_DEDUP 2u    /* flags: encode every word occurrence (by default batches of 1.75 MiB and more encode each
                                  DISTINCT word once and copy its tokens to every occurrence; same output either way) */
int swt_bpe_encode(swt_bpe_table *t, const uint8_t *text, const uint64_t *sent_off, uint64_t n_sent,
                   uint32_t *out_ids, uint64_t out_cap, uint64_t *out_off, uint64_t *n_tokens, uint32_t flags);

/* Host-buffer form for a caller that holds strings, not offsets (Python's FastBPE.tokenize over a list: bpe.py:245-249 per
 * text): joined = the sentences with ONE zero byte between neighbours, as for swt_utf8_prepare_joined, NOT yet lowercased.
 * The device finds the separators, lowercases (utils.py:27) and encodes; the prepared text never travels back to the host.
 * out_cap >= n_joined is always sufficient.  need_host[n_sent] as from swt_utf8_lower: when it flags a sentence nothing is
 * encoded, *n_tokens = UINT64_MAX (SWT_OK), and the caller lowercases on the host and uses swt_bpe_encode. */
int swt_bpe_encode_joined(swt_bpe_table *t, const uint8_t *joined, uint64_t n_joined, uint64_t n_sent, uint32_t *out_ids,
                          uint64_t out_cap, uint64_t *out_off, uint64_t *n_tokens, uint8_t *need_host, uint32_t flags);

/* Device-buffer form.  d_out_ids needs room for n_bytes ids (worst case); d_out_off[n_sent+1].
 * d_n_tokens (device, 1 element) receives the total. */
int swt_bpe_encode_dev(swt_bpe_table *t, const uint8_t *d_text, uint64_t n_bytes, const uint64_t *d_sent_off,
                       uint64_t n_sent, uint32_t *d_out_ids, uint64_t *d_out_off, uint64_t *d_n_tokens,
                       uint32_t flags, void *stream);

/* ------------------------------------------------------------------------------------------------
 * NaiveBPE encode over the same table: replaces NaiveBPE.tokenize (source/bpe.py:136-158) -- the pre-tokenizer split of
 * SubwordTokenizer.preprocessing (source/utils.py:26-29) and, per word, NaiveBPE.encode_word (source/bpe.py:114-134): every
 * merge of the list applied IN LIST ORDER to all left-to-right non-overlapping occurrences (source/bpe.py:126-127 over
 * _replace_pair, source/bpe.py:25-48), '##' = SWT_BPE_CONT on every token after the first of its word (source/bpe.py:130-132).
 * A pair listed twice is applied at both of its positions (list semantics, not the dict of source/bpe.py:257).  Arguments, token
 * ids, flags (SWT_BPE_RAW_WORDS = NaiveBPE.encode_word batched; SWT_BPE_NO_DEDUP), need_host / *n_tokens = UINT64_MAX and
 * capacities (out_cap >= n_bytes, >= n_joined for the joined form, is always sufficient) as the swt_bpe_encode trio.
 * swt_bpe_table_create decides whether list order can differ from FastBPE's lowest rank first: it cannot when no pair is listed
 * twice and every pair ranks above the merges that produce its symbols (any trained list).  Such a table runs the FastBPE
 * kernels unchanged; only the others take the ordered form of the kernel (one lane per word, csrc/swt_bpe_encode.hip). */
int swt_bpe_encode_naive(swt_bpe_table *t, const uint8_t *text, const uint64_t *sent_off, uint64_t n_sent,
                         uint32_t *out_ids, uint64_t out_cap, uint64_t *out_off, uint64_t *n_tokens, uint32_t flags);
int swt_bpe_encode_naive_joined(swt_bpe_table *t, const uint8_t *joined, uint64_t n_joined, uint64_t n_sent, uint32_t *out_ids,
                                uint64_t out_cap, uint64_t *out_off, uint64_t *n_tokens, uint8_t *need_host, uint32_t flags);
int swt_bpe_encode_naive_dev(swt_bpe_table *t, const uint8_t *d_text, uint64_t n_bytes, const uint64_t *d_sent_off,
                             uint64_t n_sent, uint32_t *d_out_ids, uint64_t *d_out_off, uint64_t *d_n_tokens,
                             uint32_t flags, void *stream);

/* ------------------------------------------------------------------------------------------------
 * BPE-dropout (Provilkov et al. 2020; not in the reference): swt_bpe_encode with every candidate merge skipped with a given
 * probability at every merge step, so that the same text comes out in another segmentation per (seed, epoch).  Arguments, ids,
 * flags and capacities as swt_bpe_encode / swt_bpe_encode_dev, plus the draw: drop_below in [0, 2^32] (from a probability p,
 * round(p * 2^32); above 2^32: SWT_ERR_INVALID), a 64-bit seed and a 32-bit epoch.  No floating point on the device.
 *
 * Pre-tokenisation is swt_bpe_encode's; a word of one symbol is that symbol.  A word of symbols s[0..n) (its code points) has
 * the key (i, b): i = the index of its sentence in this call's sent_off, b = the byte offset of the word's first byte from
 * sent_off[i] in the text the call is given (for Python's entry points pack_and_lower(texts)), both mod 2^32.  Then
 *     t = 0
 *     while n >= 2:
 *         live = the k in [0, n - 1) whose pair (s[k], s[k+1]) has a rank and is not dropped(t, k)
 *         if there is none: stop
 *         m = the smallest rank among the pairs at live
 *         left to right (source/bpe.py:221-235): at k, if k is live and its pair has rank m, emit the merged symbol and go on
 *         at k + 2, else emit s[k] and go on at k + 1
 *         s, n = what was emitted; t += 1
 * dropped(t, k): x = Philox4x32-10 (the function and constants of swt_mlm_mask) of the counter
 * (((t << 16) + (k >> 2)) mod 2^32, b, i, epoch) under the key (seed & 0xFFFFFFFF, seed >> 32); the pair is dropped iff
 * x[k & 3] < drop_below.  k indexes the word's sequence as it stands at the start of round t.
 * So: a sentence's ids depend on (seed, epoch, i) and its own bytes, not on tiles, chunks, the route of the call or the other
 * sentences; drop_below = 0 is swt_bpe_encode for any table; drop_below = 2^32 leaves every word as its code points; the loop
 * stops in the first round in which every ranked pair is dropped (the paper's rule).  Two occurrences of a word must be able to
 * differ, so the word-level dedup pipeline is never taken, whatever SWT_OPT_DEDUP says.  With SWT_BPE_RAW_WORDS every sentence
 * is one word and b = 0.  One lane per word through the literal loop (csrc/swt_bpe_encode.hip, dropout_word). */
int swt_bpe_encode_dropout(swt_bpe_table *t, const uint8_t *text, const uint64_t *sent_off, uint64_t n_sent,
                           uint32_t *out_ids, uint64_t out_cap, uint64_t *out_off, uint64_t *n_tokens, uint32_t flags,
                           uint64_t drop_below, uint64_t seed, uint32_t epoch);
int swt_bpe_encode_dropout_dev(swt_bpe_table *t, const uint8_t *d_text, uint64_t n_bytes, const uint64_t *d_sent_off,
                               uint64_t n_sent, uint32_t *d_out_ids, uint64_t *d_out_off, uint64_t *d_n_tokens,
                               uint32_t flags, uint64_t drop_below, uint64_t seed, uint32_t epoch, void *stream);

/* ------------------------------------------------------------------------------------------------
 * FastWP encode: replaces WPTrie_E2E (source/utils.py:66-139: insert + precompute, built on the host
 * and flattened into device arrays) and FastWP.tokenize/matchloop/iswdbndry/ispunc
 * (source/wordpiece.py:233-316).
 */
typedef struct swt_wp_trie swt_wp_trie;

/* vocabulary as UTF-32 code points + n_vocab+1 offsets; token id = index (first wins on duplicates) */
int swt_wp_trie_create(const uint32_t *vocab_cps, const uint64_t *vocab_off, uint32_t n_vocab, swt_wp_trie **out);
void swt_wp_trie_destroy(swt_wp_trie *t);
int swt_wp_trie_set_option(swt_wp_trie *t, int option, int value);
int swt_wp_trie_stats(const swt_wp_trie *t, uint32_t *n_nodes, uint32_t *n_edges, uint32_t *n_pops);
/* NaiveWP.encode_word("##") evaluated once at build: returns its length in ids (copied to out up to
 * cap), or -1 when the reference never returns from it. */
int64_t swt_wp_trie_corner(const swt_wp_trie *t, uint32_t *out, uint64_t cap);
/* Debug/parity view of one node of the flattened trie, addressed by its path string (with the '##'
 * prefix where the token has one): failure link as a node id, pops copied out.  Node ids: 0 root,
 * 1 root_p, 2.. in creation order.  Returns SWT_ERR_INVALID when the path does not exist. */
int swt_wp_trie_node(const swt_wp_trie *t, const uint32_t *path, uint64_t path_len, uint32_t *node_id,
                     int32_t *link, uint8_t *is_end, uint32_t *pops, uint32_t pops_cap, uint32_t *n_pops);
int swt_wp_trie_node_path(const swt_wp_trie *t, uint32_t node_id, uint32_t *out, uint64_t cap, uint64_t *len);

int swt_wp_encode(swt_wp_trie *t, const uint8_t *text, const uint64_t *sent_off, uint64_t n_sent,
                  uint32_t *out_ids, uint64_t out_cap, uint64_t *out_off, uint8_t *status, uint64_t *n_tokens);
/* From the sentences joined with ONE zero byte between neighbours, not yet lowercased (wordpiece.py:248 lower() happens on the
 * device): see swt_bpe_encode_joined, including the meaning of need_host and *n_tokens = UINT64_MAX. */
int swt_wp_encode_joined(swt_wp_trie *t, const uint8_t *joined, uint64_t n_joined, uint64_t n_sent, uint32_t *out_ids,
                         uint64_t out_cap, uint64_t *out_off, uint8_t *status, uint64_t *n_tokens, uint8_t *need_host);
int swt_wp_encode_dev(swt_wp_trie *t, const uint8_t *d_text, uint64_t n_bytes, const uint64_t *d_sent_off,
                      uint64_t n_sent, uint32_t *d_out_ids, uint64_t *d_out_off, uint8_t *d_status,
                      uint64_t *d_n_tokens, void *stream);

/* ------------------------------------------------------------------------------------------------
 * NaiveWP encode over the same trie: replaces NaiveWP.tokenize (source/wordpiece.py:160-179) -- the pre-tokenizer split of
 * SubwordTokenizer.preprocessing (source/utils.py:26-29) and, per word, the longest-prefix loop of NaiveWP.encode_word
 * (source/wordpiece.py:132-159: "##" in front of every remainder, "[UNK]" = n_vocab+1 for the whole word when no prefix
 * matches).  Arguments, ids and statuses as the swt_wp_encode trio; the only status besides SWT_WP_OK is
 * SWT_WP_NONTERMINATING (a word of the sentence keeps the reference looping; the sentence gets no tokens).  out_cap >= n_bytes
 * is always sufficient.  SWT_ERR_UNSUPPORTED for a vocabulary with a token of three or more leading '#' followed by
 * another character: only there can a word yield more tokens than it has bytes. */
int swt_wp_encode_naive(swt_wp_trie *t, const uint8_t *text, const uint64_t *sent_off, uint64_t n_sent,
                        uint32_t *out_ids, uint64_t out_cap, uint64_t *out_off, uint8_t *status, uint64_t *n_tokens);
int swt_wp_encode_naive_joined(swt_wp_trie *t, const uint8_t *joined, uint64_t n_joined, uint64_t n_sent, uint32_t *out_ids,
                               uint64_t out_cap, uint64_t *out_off, uint8_t *status, uint64_t *n_tokens, uint8_t *need_host);
int swt_wp_encode_naive_dev(swt_wp_trie *t, const uint8_t *d_text, uint64_t n_bytes, const uint64_t *d_sent_off,
                            uint64_t n_sent, uint32_t *d_out_ids, uint64_t *d_out_off, uint8_t *d_status,
                            uint64_t *d_n_tokens, void *stream);

/* ------------------------------------------------------------------------------------------------
 * MaxMatch-Dropout (Hiraoka, COLING 2022; not in the reference): swt_wp_encode_naive with a vocabulary match of the
 * longest-match search thrown away with a given probability, so that the search falls back to a shorter piece and the same text
 * comes out in another segmentation per (seed, epoch).  Arguments, ids, statuses, capacities (out_cap >= n_bytes) and refusals
 * (SWT_ERR_UNSUPPORTED for a '###x' vocabulary included) as swt_wp_encode_naive / _dev, plus the draw, exactly as
 * swt_bpe_encode_dropout carries it: drop_below in [0, 2^32] (from a probability p, round(p * 2^32); above 2^32:
 * SWT_ERR_INVALID), a 64-bit seed and a 32-bit epoch.  No floating point on the device.
 *
 * The split is swt_wp_encode_naive's.  A word is walked as NaiveWP.encode_word walks it (source/wordpiece.py:131-158): the state
 * is the string "#" * L + word[p:], L = 0 at the word's start.  In one step
 *     the candidates are the prefixes of the state that are vocabulary tokens;
 *     a candidate TAKES c code points when it reaches c code points beyond the L leading '#' (c = 0: it ends inside them);
 *     a candidate with c >= 2 is dropped iff x[c & 3] < drop_below, x = Philox4x32-10 (the function and constants of
 *       swt_mlm_mask) of the counter (c >> 2, a, i, epoch), all mod 2^32, under the key (seed & 0xFFFFFFFF, seed >> 32), where
 *       i = the index of the sentence in this call's sent_off and a = the byte offset from sent_off[i] of the word byte the state
 *       starts at (p), in the text the call is given (for Python's entry points pack_and_lower(texts));
 *     candidates with c <= 1 are never dropped;
 *     the step takes the longest candidate that is not dropped; when there is none the whole word is one "[UNK]" and the pieces
 *       stored so far are discarded (wordpiece.py:148-149); everything else is the plain walk.
 * So: a draw depends on (seed, epoch, i, a, c) and on nothing else -- not on L, the step, tiles, chunks, the route of the call or
 * the other sentences; one Philox call serves four consecutive c.  drop_below = 0 is swt_wp_encode_naive on any vocabulary;
 * drop_below = 2^32 leaves every word as its code points wherever each is a token in its position.  At a fixed p the step is the
 * plain step over a vocabulary with some tokens removed, never a '#'-only one, so the bound of sharp_depth + 2 steps at one p
 * still decides SWT_WP_NONTERMINATING -- and a sentence's status is that of the thinned walk, so IT CAN DEPEND ON THE DRAW: under
 * {"a", "##", "##bc"} the word "abc" is a ##bc when "##bc" survives and never returns when it is dropped (the plain step at
 * "##bc" then takes "##" for ever); under {"a", "##bc"} it is "[UNK]" instead.  The paper's rule to our reading, except that a
 * single code point is never dropped here, so that p = 1 gives the characters.  There is no joined form: a is
 * an offset in the text the call is given.  One lane per word (csrc/swt_wp.hip, naive_word with a WpDraw). */
int swt_wp_encode_naive_dropout(swt_wp_trie *t, const uint8_t *text, const uint64_t *sent_off, uint64_t n_sent,
                                uint32_t *out_ids, uint64_t out_cap, uint64_t *out_off, uint8_t *status, uint64_t *n_tokens,
                                uint64_t drop_below, uint64_t seed, uint32_t epoch);
int swt_wp_encode_naive_dropout_dev(swt_wp_trie *t, const uint8_t *d_text, uint64_t n_bytes, const uint64_t *d_sent_off,
                                    uint64_t n_sent, uint32_t *d_out_ids, uint64_t *d_out_off, uint8_t *d_status,
                                    uint64_t *d_n_tokens, uint64_t drop_below, uint64_t seed, uint32_t epoch, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Token-id histogram on the device: the Counter over token strings of the reference's
 * zipf_distribution (source/benchmarks.py:240-253), over ids -- a '##' token and the same token without the prefix are
 * different strings and different ids.  counts has 2 * id_cap entries: counts[id & 0x7FFFFFFF] for ids without SWT_BPE_CONT,
 * counts[id_cap + (id & 0x7FFFFFFF)] for ids with it; ids whose low 31 bits reach id_cap are tallied in *out_of_range.
 * FastWP ids carry no flag: only the first half is used.  The `_dev` form takes device pointers and zeroes the outputs itself.
 */
int swt_token_histogram(const uint32_t *ids, uint64_t n, uint32_t id_cap, uint64_t *counts, uint64_t *out_of_range);
int swt_token_histogram_dev(const uint32_t *d_ids, uint64_t n, uint32_t id_cap, uint64_t *d_counts, uint64_t *d_out_of_range,
                            void *stream);

/* ------------------------------------------------------------------------------------------------
 * Token-sequence equivalence of two tokenizers on the device: the counting of the reference's token_sequence_equivalence
 * (source/benchmarks.py:113-183, what `--benchmark --pretrained --compare` prints) over two id streams with the same rows
 * (CSR offsets off_a[n_rows+1], off_b[n_rows+1]) instead of two lists of token strings per sentence and per word.
 *
 * The reference compares tokens as STRINGS after `tok[2:] if tok.startswith("##") else tok` (source/benchmarks.py:144-145,
 * 164-165), so the two streams need a common id space: the caller interns the stripped strings of both tokenizers in one
 * table and hands over one uint32 map per stream.  The canonical id of a token `id` is, with s = id & 0x7FFFFFFF:
 *     s                                                              when s < map_base
 *     map[(s - map_base) + ((flagged && (id >> 31)) ? n_map : 0)]    otherwise
 * (a BPE stream: map_base = SWT_SYM_BASE, flagged = 1, 2 * n_map entries, the second half for ids with SWT_BPE_CONT; a
 * WordPiece stream: map_base = 0, flagged = 0, n_map entries).  A token with s - map_base >= n_map, or whose map entry is
 * 0xFFFFFFFF, has no canonical id: it is tallied in totals[4] and takes part in nothing.
 *
 * Per row, with t1 / t2 the row's canonical ids (source/benchmarks.py:148-156, 166):
 *     positions    min(len(t1), len(t2))
 *     pos_matches  #{i < positions : t1[i] == t2[i]}
 *     unordered    sum over tokens of min(count in t1, count in t2)    (the multiset intersection)
 *     has_common   1 when set(t1) & set(t2) is not empty, else 0
 * per_row[4 r .. 4 r + 4) receives these four (may be NULL); totals[0..4) their sums over the rows, each row multiplied by
 * weight[r] (NULL = 1; the word pass runs once per DISTINCT word with its number of occurrences); totals has 5 entries.
 * Rows of any length are counted exactly and on the device (csrc/swt_metrics.hip; swt_token_equivalence_capacity reports the
 * row sizes at which the kernels change form: the shorter side's length up to which one wavefront takes the row, and the
 * distinct tokens one pass of the workgroup kernel holds).  The `_dev` form takes device pointers, zeroes its outputs itself,
 * enqueues on the stream and does not synchronise.
 */
int swt_token_equivalence(const uint32_t *ids_a, const uint64_t *off_a, const uint32_t *map_a, uint32_t map_base_a, uint32_t n_map_a,
                          int flagged_a, const uint32_t *ids_b, const uint64_t *off_b, const uint32_t *map_b, uint32_t map_base_b,
                          uint32_t n_map_b, int flagged_b, uint64_t n_rows, const uint32_t *weight, uint64_t *totals, uint32_t *per_row);
int swt_token_equivalence_dev(const uint32_t *d_ids_a, const uint64_t *d_off_a, const uint32_t *d_map_a, uint32_t map_base_a,
                              uint32_t n_map_a, int flagged_a, const uint32_t *d_ids_b, const uint64_t *d_off_b, const uint32_t *d_map_b,
                              uint32_t map_base_b, uint32_t n_map_b, int flagged_b, uint64_t n_rows, const uint32_t *d_weight,
                              uint64_t *d_totals, uint32_t *d_per_row, void *stream);
int swt_token_equivalence_capacity(uint32_t *wave_cap, uint32_t *block_cap);

/* ------------------------------------------------------------------------------------------------
 * Token spans on the device: for every token of an id stream, where in its sentence it came from (offset_mapping) and the index
 * of its pre-tokenizer word (word_ids).  SubwordTokenizer.preprocessing (source/utils.py:15-29) returns (word, (start, end)) per
 * word; this carries the offsets on to the tokens of NaiveBPE, FastBPE and NaiveWP, whose tokens are grouped by word and tile
 * it: a token covers as many code points as its string has after the '##', NaiveWP's "[UNK]" its whole word
 * (source/wordpiece.py:132-159).  FastWP is NOT covered here: its segments end where the trie walk ends, not at character
 * classes.  Its spans come out of the walk itself: swt_wp_encode_spans below.
 *
 * In: the lowercased text with sent_off[n_sent+1]; ids with tok_off[n_sent+1] (the CSR the encoders return; spans, word and the
 * ids are indexed by the same token slots tok_off[0] .. tok_off[n_sent]); a length table in the (base, n, flagged) convention of
 * swt_token_equivalence.  With s = id & 0x7FFFFFFF the token covers
 *     1 code point                       when s < len_base
 *     len[s - len_base] & 0xFFFFFF       otherwise; 0 = its whole word (the unknown token); s - len_base >= n_len: no length
 * and it continues its word when flagged ? bit 31 of the id (SWT_BPE_CONT) : bit 31 of its entry (ids below len_base: never).
 * (BPE: len_base = SWT_SYM_BASE, flagged = 1.  NaiveWP: len_base = 0, flagged = 0, n_vocab + 2 entries, the last two 0.)
 *
 * The text is split by the preprocessing rule over the library's class table: SWT_CLS_BERT_WS code points are dropped, every
 * SWT_CLS_BERT_PUNCT code point is a word, anything else forms runs.  Generalised UTF-8: surrogates pass through; a lead byte
 * takes the continuation bytes that follow it, up to its length and the end of its sentence; a continuation byte no lead takes
 * is one code point.  The k-th word of a sentence belongs to its k-th token group; a group starts at a token that is not a
 * continuation.
 *
 * Out: spans[2 t], spans[2 t + 1] = start and end of token t relative to its sentence's first byte, in bytes, or in code
 * points with SWT_SPAN_CODEPOINTS; word[t] (may be NULL) = index of its word in the sentence; status[s] = SWT_SPAN_OK, or
 * SWT_SPAN_MISMATCH when the ids of sentence s do not tile its text: another number of groups than words, a group whose lengths
 * do not add up to its word, a whole-word token with company in its group, a first token that continues, an id without a
 * length (or, in the `_dev` form, offsets of the sentence that decrease or pass n_bytes).  Such a sentence gets (0, 0) for
 * every span and 0 for every word index; it causes no access outside the arrays and leaves its neighbours alone, so the call
 * is safe with ids made by another table or from another text.
 *
 * swt_token_spans: host buffers; SWT_ERR_INVALID for a NULL required pointer, decreasing offsets or a sentence of 2^32 bytes or
 * more.  The `_dev` form takes device pointers (offsets that do not decrease), writes every entry of its outputs itself,
 * enqueues on the stream and does not synchronise; its scratch is one grow-only workspace of the process (12 bytes per text
 * byte), so two calls must not run at the same time on different streams.  swt_token_spans_capacity: the byte sizes at which
 * the kernel changes form (csrc/swt_spans.hip) -- block: what one wavefront classifies per step (bytes, and tokens), counted from
 * the sentence's first; chunk: what it stages at a time, likewise; tile: the window of text whose sentence starts one workgroup
 * owns. */
#define SWT_SPAN_CODEPOINTS 1u
#define SWT_SPAN_OK 0
#define SWT_SPAN_MISMATCH 1
int swt_token_spans(const uint8_t *text, const uint64_t *sent_off, uint64_t n_sent, const uint32_t *ids, const uint64_t *tok_off,
                    const uint32_t *len, uint32_t len_base, uint32_t n_len, int flagged, uint32_t flags, uint32_t *spans, uint32_t *word,
                    uint8_t *status);
int swt_token_spans_dev(const uint8_t *d_text, uint64_t n_bytes, const uint64_t *d_sent_off, uint64_t n_sent, const uint32_t *d_ids,
                        const uint64_t *d_tok_off, const uint32_t *d_len, uint32_t len_base, uint32_t n_len, int flagged, uint32_t flags,
                        uint32_t *d_spans, uint32_t *d_word, uint8_t *d_status, void *stream);
int swt_token_spans_capacity(uint32_t *block, uint32_t *chunk, uint32_t *tile);

/* ------------------------------------------------------------------------------------------------
 * FastWP with token spans: FastWP.tokenize (source/wordpiece.py:233-270) where every token comes with the characters it covers
 * and the index of its segment.  Each pass of the loop at wordpiece.py:251 is one segment starting at i0; matchloop leaves it
 * at i1.  The tokens of a valid segment cover a prefix of s[i0:i1] one after the other: the first covers len(token) code points
 * (a literal "##ing" in the text covers five), every later one -- it begins with "##" -- len(token) - 2.  The prefix may be
 * shorter than the segment: source/utils.py:136-137 redirects the failure link of every non-alphanumeric node and drops the
 * path of the old link target, and nothing covers those characters.  The "['UNK']" of an invalid segment (wordpiece.py:255-257)
 * covers (i0, b), b the first iswdbndry position at or after i1 (the sentence's length at most).  The one id of the "##" corner
 * (wordpiece.py:260-261) covers (i0, i0 + 2).  The word index numbers the segments of a sentence that emit at least one token.
 * A span never passes its sentence's end (a vocabulary token that holds a space could cover the appended one).
 *
 * Arguments, ids, offsets and statuses are exactly those of swt_wp_encode / swt_wp_encode_dev, bit for bit.  spans[2 t],
 * spans[2 t + 1] = start and end of token t relative to its sentence's first byte, in bytes, or in code points with
 * SWT_SPAN_CODEPOINTS (the unit is a lead byte with the continuation bytes that ride with it); word[t] (may be NULL) its word
 * index; both are indexed by the token slots of out_ids.  spans needs two words and word one for every id out_ids has room for
 * (out_cap in the host form, n_bytes in the `_dev` form); any 4-byte alignment will do.  A sentence whose status is not
 * SWT_WP_OK has no tokens and no spans.  SWT_ERR_INVALID for NULL spans or an unknown flag.
 *
 * The span form of the kernel is a second instantiation (csrc/swt_wp.hip); the length of every vocabulary token is kept by the
 * trie handle and uploaded by the first call, and the handle's grow-only workspace takes 12 more bytes per text byte.  The
 * word-level dedup pipeline is never taken, whatever SWT_OPT_DEDUP says: a unique chunk has no position.
 * swt_wp_encode_spans_capacity: the sizes at which the call changes form -- block: bytes classified per step; chunk: bytes
 * staged at a time (a longer sentence is walked by one lane); tile: the window of sentence starts of one workgroup;
 * direct_bytes, direct_sents: up to here one workgroup and one launch do the whole call. */
int swt_wp_encode_spans(swt_wp_trie *t, const uint8_t *text, const uint64_t *sent_off, uint64_t n_sent, uint32_t *out_ids,
                        uint64_t out_cap, uint64_t *out_off, uint8_t *status, uint64_t *n_tokens, uint32_t flags, uint32_t *spans,
                        uint32_t *word);
int swt_wp_encode_spans_dev(swt_wp_trie *t, const uint8_t *d_text, uint64_t n_bytes, const uint64_t *d_sent_off, uint64_t n_sent,
                            uint32_t *d_out_ids, uint64_t *d_out_off, uint8_t *d_status, uint64_t *d_n_tokens, uint32_t flags,
                            uint32_t *d_spans, uint32_t *d_word, void *stream);
int swt_wp_encode_spans_capacity(uint32_t *block, uint32_t *chunk, uint32_t *tile, uint32_t *direct_bytes, uint32_t *direct_sents);

/* ------------------------------------------------------------------------------------------------
 * BPE training: replaces the merge loop of NaiveBPE.train (source/bpe.py:88-111; FastBPE.train
 * inherits it, source/bpe.py:198-200) and its word dedup (source/bpe.py:73-81).
 *
 * The caller keeps the string set and the stop test (`len(vocab) < max_vocab`, source/bpe.py:88,103):
 *   swt_bpe_train_create*  ->  loop { swt_bpe_train_best; intern(left+right); swt_bpe_train_apply }.
 * Device state: the unique-word symbol stream (uint32; a merge leaves a hole, addresses are stable), word offsets and
 * frequencies, the pair histogram (hash table of 64-bit pair keys with 64-bit counts) which is built once and then updated
 * incrementally by every merge -- the same counts the reference recomputes from scratch each round -- an inverted index
 * pair -> words so that a merge visits only the words that hold it, and the list of high-count candidates the argmax scans.
 * All of a trainer's work is enqueued on one stream (the legacy default stream).
 */
typedef struct swt_bpe_trainer swt_bpe_trainer;

/* From lowercased UTF-8 text: pre-tokenize, dedup words in first-occurrence order, symbolise
 * (source/bpe.py:70-81).  n_base_symbols = number of distinct code points (the initial len(vocab)). */
int swt_bpe_train_create_text(const uint8_t *text, const uint64_t *sent_off, uint64_t n_sent,
                              swt_bpe_trainer **out);
/* The same from the sentences joined with ONE zero byte between neighbours (exactly n_sent - 1 zero bytes: the input of
 * swt_utf8_prepare_joined, which also says what "lowercased" means here): the device finds the separators, lowercases and
 * takes the census without the prepared text travelling to the host and back.  need_host[n_sent] comes back as from
 * swt_utf8_lower; when it flags a sentence, *out stays NULL (SWT_OK) and the caller lowercases on the host and uses
 * swt_bpe_train_create_text. */
int swt_bpe_train_create_joined(const uint8_t *joined, uint64_t n_joined, uint64_t n_sent, uint8_t *need_host, swt_bpe_trainer **out);
/* NaiveWP.train's state instead (source/wordpiece.py:44-63): the same split and word dedup, symbols
 * = the word's first code point c and SWT_WP_CONT + c ("##c") for the others, plus exact symbol frequencies.  The handle
 * works with every swt_bpe_train_* call below; the step maximises the likelihood score freq / (f_left * f_right)
 * (source/wordpiece.py:84-92: Python's int / int, the correctly rounded quotient; first maximum in first-occurrence
 * order) and the `count` outputs carry that score's IEEE-754 bit pattern.  Merged symbols start at SWT_WP_MERGED_BASE;
 * the caller names them left + right[2:] (source/wordpiece.py:95). */
#define SWT_WP_CONT 0x110000u
#define SWT_WP_MERGED_BASE 0x220000u
int swt_wp_train_create_text(const uint8_t *text, const uint64_t *sent_off, uint64_t n_sent,
                             swt_bpe_trainer **out);
/* ... and from the joined texts, as swt_bpe_train_create_joined (NULL handle + SWT_OK: a sentence needs the host's lower()). */
int swt_wp_train_create_joined(const uint8_t *joined, uint64_t n_joined, uint64_t n_sent, uint8_t *need_host, swt_bpe_trainer **out);
/* From an already deduplicated word list (symbol ids, CSR offsets, frequencies). */
int swt_bpe_train_create_words(const uint32_t *syms, const uint64_t *word_off, const uint32_t *freq,
                               uint64_t n_words, swt_bpe_trainer **out);
void swt_bpe_train_destroy(swt_bpe_trainer *t);
/* Rank-sharded training: pos_base orders this shard's words after those of lower ranks in the
 * first-occurrence tie-break (source/bpe.py:102).  Default 0. */
int swt_bpe_train_set_pos_base(swt_bpe_trainer *t, uint64_t pos_base);
int swt_bpe_train_info(const swt_bpe_trainer *t, uint64_t *n_words, uint64_t *n_symbols, uint32_t *n_base_symbols,
                       uint64_t *n_pairs);
/* distinct code points of the corpus, ascending (the initial vocab, source/bpe.py:75) */
int swt_bpe_train_base_symbols(const swt_bpe_trainer *t, uint32_t *out, uint32_t cap);
/* Most frequent pair (source/bpe.py:90-102).  *count == 0 means no pair is left (source/bpe.py:98-99).
 * *n_tied = number of pairs holding the maximum.  When it is 1, (left,right) is that pair and *first_pos is
 * ~0.  When it is > 1 the tie is broken by the earliest (word, position) in THIS handle's stream:
 * (left,right) is the pair found there and *first_pos = pos_base + its stream position; if none of the tied
 * pairs occurs in this handle's stream, *first_pos = ~0 and left = right = 0xFFFFFFFF. */
int swt_bpe_train_best(swt_bpe_trainer *t, uint32_t *left, uint32_t *right, uint64_t *count, uint64_t *n_tied,
                       uint64_t *first_pos);
/* Replace every L->R non-overlapping occurrence of (left,right) by merged (source/bpe.py:25-48,
 * 108-111) and update the histogram. */
int swt_bpe_train_apply(swt_bpe_trainer *t, uint32_t left, uint32_t right, uint32_t merged);
/* Device-driven training: up to max_steps iterations of {best, apply} enqueued back to back with no host round trip
 * per merge.  Step i merges into symbol id first_merged + i -- valid while every merged STRING is new, which the caller
 * checks afterwards from (left, right) (symbols are identified by their string; on the never-observed collision the
 * caller replays with swt_bpe_train_apply).  Stops early when no pair is left; *n_done = merges performed. */
int swt_bpe_train_run(swt_bpe_trainer *t, uint32_t max_steps, uint32_t first_merged, uint32_t *left, uint32_t *right,
                      uint64_t *count, uint32_t *n_done);
/* Copies the current stream back (parity checks, corpus_as_symbols): syms[n_symbols], word_off[n_words+1],
 * freq[n_words] (freq may be NULL). */
int swt_bpe_train_export(swt_bpe_trainer *t, uint32_t *syms, uint64_t syms_cap, uint64_t *word_off, uint32_t *freq);
/* Copies the histogram back: up to cap (key = left<<32|right, count) entries with count > 0. */
int swt_bpe_train_histogram(swt_bpe_trainer *t, uint64_t *keys, uint64_t *counts, uint64_t cap, uint64_t *n);

/* Diagnostics of the trainer's machinery (tests, bench.py): out[0..n) = re-plans of the candidate threshold so far, the
 * threshold theta (0: full-table argmax), candidate list length, inverted-index log entries, pair-table slots, state flags
 * (bit 0: the index was abandoned for whole-stream applies), steps enqueued, distinct keys in the table, index entries the
 * apply launches have gone through, words the tie scans have covered (these two: bench.py's bytes-per-merge model), times
 * the stream was rewritten without its holes. */
int swt_bpe_train_stats(const swt_bpe_trainer *t, uint64_t *out, uint32_t n);

/* One row per merge performed by swt_bpe_train_run(_sharded) so far: rows[4 i ..] = the winning count (score bits for
 * WordPiece), the number of pairs that held that maximum (> 1: the first-occurrence tie-break ran), the candidate list
 * length, and the live symbols N_t before the merge (what the reference would have rescanned).
 * rows may be NULL to query *n_rows. */
int swt_bpe_train_trace(const swt_bpe_trainer *t, uint64_t *rows, uint64_t cap_rows, uint64_t *n_rows);

/* ------------------------------------------------------------------------------------------------
 * Corpus-sharded BPE training, one process per GPU over RCCL: the multi-GPU form of the merge loop of
 * source/bpe.py:88-111 (the reference itself has no parallelism).  Every rank builds a trainer from ITS contiguous range of
 * sentences (swt_bpe_train_create_text) and keeps the pair histogram of the whole corpus; per merge the runner issues ONE
 * fixed-size ncclAllGather of packed (pair, delta) records and ONE 16-byte all-gather for the first-occurrence tie-break
 * (source/bpe.py:102; ranks are ordered by their sentence ranges), enqueued on the training stream with no host round trip,
 * up to 256 merges per call into the device.
 *
 *   rank 0: swt_dist_unique_id(id) -> the caller hands the 128 bytes to every rank (torch.distributed, MPI, a file ...)
 *   every rank: swt_init(local device); swt_dist_init(rank, world, id, &comm);
 *               swt_bpe_train_create_text(shard) -> t;  swt_bpe_train_shard_begin(&t, 1, comm, base, cap, &n_base);
 *               loop { swt_bpe_train_run_sharded(&t, 1, comm, k, first_merged, left, right, count, &n_done); intern strings }
 * The outputs are identical on every rank.  swt_dist_init_local makes a loop-back communicator whose `world` ranks are all
 * trainers of the calling process (trainers[r] = rank r; device copies instead of RCCL): the same runner on one GPU. */
typedef struct swt_dist swt_dist;
int swt_dist_unique_id(uint8_t *out128);
int swt_dist_init(int rank, int world, const uint8_t *unique_id128, swt_dist **out);
int swt_dist_init_local(int world, swt_dist **out);
void swt_dist_destroy(swt_dist *d);
int swt_dist_info(const swt_dist *d, int *rank, int *world, int *is_local);
/* Enters sharded mode: gathers the distinct initial symbols of ALL shards (the initial vocab, source/bpe.py:75; written to
 * base_out[0..*n_base) ascending when base_out is not NULL) and reduces the local histograms into every replica. */
int swt_bpe_train_shard_begin(swt_bpe_trainer **trainers, uint32_t n_local, swt_dist *d, uint32_t *base_out, uint32_t base_cap,
                              uint32_t *n_base);
/* As swt_bpe_train_run, over all shards. */
int swt_bpe_train_run_sharded(swt_bpe_trainer **trainers, uint32_t n_local, swt_dist *d, uint32_t max_steps, uint32_t first_merged,
                              uint32_t *left, uint32_t *right, uint64_t *count, uint32_t *n_done);

/* ------------------------------------------------------------------------------------------------
 * Model-ready batches on the device: the CSR pair the encoders return (ids, tok_off[n_rows+1]) as dense, padded rows of a fixed
 * width with the attention mask -- what a model's embedding layer takes, and where the reference stops at lists of strings
 * (source/bpe.py:244, source/wordpiece.py:270).  A post-pass over the ids: nothing is encoded again, no text is needed.
 *
 * Per source row r: n = tok_off[r+1] - tok_off[r] tokens; cap = width - (cls present) - (sep present) tokens fit a row.
 *   truncation (default)   one output row per source row; its body is the first min(n, cap) tokens
 *   SWT_BATCH_WINDOWS      step = cap - stride; k = 1 when n <= cap, else 1 + ceil((n - cap) / step) rows; window w holds the
 *                          tokens [w step, min(n, w step + cap)) and is output row row_base[r] + w, row_base the exclusive sum
 *                          of k (swt_batch_plan).  A row without tokens gives one row of specials and padding
 * An output row is [cls?] body [sep?] and then pad_id up to width; with SWT_BATCH_PAD_LEFT the padding comes first.  The mask is
 * 1 on cls, body and sep and 0 on padding; out_len[row] counts its ones; out_sample[row] = r.
 * Dense ids: with s = id & 0x7FFFFFFF a token becomes map[s + ((flagged && id >> 31) ? n_map : 0)]; the map has n_map entries,
 * 2 n_map when flagged.  map == NULL (only with flagged == 0) is the identity on s, n_map still bounding it.  s >= n_map or the
 * entry 0xFFFFFFFF gives unk_id and counts in info[2], once per output slot written.  Payloads (each given together with its
 * output): spans (two words per token) and word (one), as the span calls write them, go to out_spans[row, col, 0..1] and
 * out_word[row, col]; specials and padding get (0, 0) and 0xFFFFFFFF.  out_ids is int32[rows, width], int64 with SWT_BATCH_IDS64.
 *
 * SWT_ERR_INVALID: cap < 1, stride >= cap, an unknown flag, pad_id / unk_id = SWT_BATCH_NONE (the plan calls look at these only
 * with SWT_BATCH_WINDOWS, so a caller can ask for the longest row before it picks a width); NULL out_ids or out_mask; flagged
 * without a map; SWT_BATCH_WINDOWS without row_base; 2^32 rows or more.  row_base may be NULL without SWT_BATCH_WINDOWS;
 * out_sample, out_len and info may always be NULL.  The spec is a host pointer in both forms.  The host forms check everything --
 * decreasing offsets and a row_base that is not the plan of the offsets included -- before anything touches the device, and
 * swt_batch_rows returns SWT_ERR_CAPACITY with info[0] = the rows needed when they exceed rows_cap.  The `_dev` forms take device
 * pointers (offsets that do not decrease; outputs aligned to their element type, to 16 bytes for the wide stores), enqueue on
 * the stream and do not synchronise; swt_batch_rows_dev writes every element of the rows < min(rows needed, rows_cap) of every
 * output given and nothing at or beyond rows_cap * width, whatever ids and row_base hold.  swt_batch_plan_dev scans in one
 * grow-only workspace of the process: two plans must not run at once on different streams.  swt_batch_capacity: the columns one
 * wavefront writes per step and the rows of one scan group of the plan (csrc/swt_batch.hip). */
#define SWT_BATCH_NONE 0xFFFFFFFFu
#define SWT_BATCH_WINDOWS 1u
#define SWT_BATCH_PAD_LEFT 2u
#define SWT_BATCH_IDS64 4u
typedef struct swt_batch_spec { uint32_t width, stride, flags, pad_id, unk_id, cls_id, sep_id; } swt_batch_spec;  /* cls/sep = NONE: absent */

/* row_base[n_rows+1] (exclusive sum of window counts; r itself without WINDOWS), info[0] = rows out, info[1] = longest source row in tokens */
int swt_batch_plan(const uint64_t *tok_off, uint64_t n_rows, const swt_batch_spec *spec, uint64_t *row_base, uint64_t *info);
int swt_batch_plan_dev(const uint64_t *d_tok_off, uint64_t n_rows, const swt_batch_spec *spec, uint64_t *d_row_base, uint64_t *d_info, void *stream);
/* info[0] rows written, info[1] source rows that lost tokens (only without WINDOWS), info[2] tokens sent to unk_id */
int swt_batch_rows(const uint32_t *ids, const uint64_t *tok_off, uint64_t n_rows, const uint32_t *map, uint32_t n_map, int flagged,
                   const uint32_t *spans, const uint32_t *word, const swt_batch_spec *spec, const uint64_t *row_base, uint64_t rows_cap,
                   void *out_ids, uint8_t *out_mask, uint32_t *out_spans, uint32_t *out_word, uint32_t *out_sample, uint32_t *out_len, uint64_t *info);
int swt_batch_rows_dev(const uint32_t *d_ids, const uint64_t *d_tok_off, uint64_t n_rows, const uint32_t *d_map, uint32_t n_map, int flagged,
                       const uint32_t *d_spans, const uint32_t *d_word, const swt_batch_spec *spec, const uint64_t *d_row_base, uint64_t rows_cap,
                       void *d_out_ids, uint8_t *d_out_mask, uint32_t *d_out_spans, uint32_t *d_out_word, uint32_t *d_out_sample, uint32_t *d_out_len,
                       uint64_t *d_info, void *stream);
int swt_batch_capacity(uint32_t *cols_per_step, uint32_t *scan_group);

/* ------------------------------------------------------------------------------------------------
 * Sentence-pair batches: rows [cls] A [sep] B [sep] for the two-segment tasks (question answering, NLI), with token types,
 * truncation that spares one side and windows that slide over one side while the other is repeated in every row -- what the
 * `tokenizers` wheel gives with the template "[CLS] $A [SEP] $B:1 [SEP]:1", enable_truncation(width, stride, strategy) and
 * enable_padding(length=width).  The same post-pass as above with the same spec; cls_id and sep_id are both ids or both
 * SWT_BATCH_NONE, and cap = width - 3 with them, width without.
 *
 * off_a[n_rows+1] and off_b[n_rows+1] index ONE stream ids / spans / word: pair r is the tokens [off_a[r], off_a[r+1]) and
 * [off_b[r], off_b[r+1]), na and nb of them.  One encoder call over texts + text_pairs gives tok_off[2 n_rows + 1]; off_a =
 * tok_off and off_b = tok_off + n_rows are the two arrays, with no second encode and no copy.  Any two arrays that do not
 * decrease will do.
 *   a pair that fits (na + nb <= cap)   one row, whatever the strategy and the stride
 *   SWT_PAIR_ONLY_SECOND   A whole, B in a budget of cap - na tokens: its first cap - na, or with SWT_BATCH_WINDOWS windows of
 *                          the budget that advance by budget - stride, counted and placed as the windows above; every window
 *                          row repeats A
 *   SWT_PAIR_ONLY_FIRST    the mirror image: B whole, A cut or windowed in cap - nb
 *   SWT_PAIR_LONGEST_FIRST with n1 <= n2 the two lengths (A is n1 on a tie): n2 = n1 if n1 > cap, else max(n1, cap - n1); if
 *                          n1 + n2 > cap then n1 = cap / 2, n2 = n1 + cap % 2; each side keeps its first n1 or n2 tokens.
 *                          Truncation only: with SWT_BATCH_WINDOWS the wheel emits the cross product of both sides' windows
 *                          in an order nobody relies on, which is out of scope here -- SWT_ERR_INVALID
 * A pair that does not fit and whose cut side has a budget below 1 -- or, with SWT_BATCH_WINDOWS, a budget <= stride -- is
 * REFUSED (the wheel raises "Sequence to truncate too short" / "`stride` must be strictly less than `max_len`"): status[r] =
 * SWT_PAIR_REFUSED, and the pair still gives exactly one row: pad_id everywhere, mask 0, length 0.  Only the two ONLY
 * strategies refuse.  The call succeeds; info[3] counts such pairs.
 *
 * Per column, besides the outputs of swt_batch_rows: out_type (the element type of out_ids: it indexes an embedding table) 0 on
 * cls, A and the first sep, 1 on B and the last sep, 0 on padding; out_special 1 on cls, sep and padding; out_seq 0 on A's
 * tokens, 1 on B's, -1 elsewhere.  Spans and word indices are each side's own, as the span calls wrote them: B's start again
 * at 0.  An empty A gives cls sep B sep, two empty sides cls sep sep with types 0 0 1.  Without cls and sep the row is A's
 * tokens and then B's.  Dense ids, unk_id and the padding side are those of swt_batch_rows.
 *
 * info[5]: [0] rows out, [1] the largest na + nb, [2] tokens sent to unk_id (once per slot written), [3] refused pairs, [4]
 * pairs that lost tokens (without SWT_BATCH_WINDOWS; a refused pair is not among them).  The plan fills [0], [1] and [3] and
 * zeroes the rest; with a zero width (and no SWT_BATCH_WINDOWS) it takes every pair as fitting, for a caller that wants [1]
 * before it picks a width.  The row call fills all five, [3] and [4] over the pairs whose rows lie below rows_cap.
 * row_base[n_rows+1] and status[n_rows] come from the plan.  The row call takes row_base as swt_batch_rows does (NULL only
 * without SWT_BATCH_WINDOWS).  status may be NULL: the kernel takes every pair's cut from its offsets, as it takes the window
 * counts; the host form checks a status it is given.  out_type, out_special, out_seq, out_sample, out_len, info and the payload
 * outputs may be NULL.
 *
 * SWT_ERR_INVALID: what swt_batch_rows refuses; cls_id without sep_id or the reverse; a strategy that is none of the three;
 * SWT_PAIR_LONGEST_FIRST with SWT_BATCH_WINDOWS; in the plan a NULL row_base, status or info.  The host forms check everything
 * -- decreasing offsets, a row_base or a status that is not the plan of these offsets -- before anything touches the device,
 * and swt_batch_pair_rows returns SWT_ERR_CAPACITY with info[0] = the rows needed when they exceed rows_cap.  The `_dev` forms
 * enqueue and do not synchronise; swt_batch_pair_rows_dev writes every element of the rows < min(rows needed, rows_cap) of
 * every output given and nothing at or beyond rows_cap * width, whatever ids, row_base and status hold.  The plan scans in the
 * workspace of swt_batch_plan_dev: no two plans of either kind at once on different streams.  swt_batch_pair_capacity: as
 * swt_batch_capacity, for the pair kernels (csrc/swt_batch.hip). */
#define SWT_PAIR_LONGEST_FIRST 0u
#define SWT_PAIR_ONLY_FIRST 1u
#define SWT_PAIR_ONLY_SECOND 2u
#define SWT_PAIR_OK 0
#define SWT_PAIR_REFUSED 1
int swt_batch_pair_plan(const uint64_t *off_a, const uint64_t *off_b, uint64_t n_rows, const swt_batch_spec *spec, uint32_t strategy,
                        uint64_t *row_base, uint8_t *status, uint64_t *info);
int swt_batch_pair_plan_dev(const uint64_t *d_off_a, const uint64_t *d_off_b, uint64_t n_rows, const swt_batch_spec *spec, uint32_t strategy,
                            uint64_t *d_row_base, uint8_t *d_status, uint64_t *d_info, void *stream);
int swt_batch_pair_rows(const uint32_t *ids, const uint64_t *off_a, const uint64_t *off_b, uint64_t n_rows, const uint32_t *map, uint32_t n_map,
                        int flagged, const uint32_t *spans, const uint32_t *word, const swt_batch_spec *spec, uint32_t strategy,
                        const uint64_t *row_base, const uint8_t *status, uint64_t rows_cap, void *out_ids, uint8_t *out_mask, void *out_type,
                        uint8_t *out_special, int8_t *out_seq, uint32_t *out_spans, uint32_t *out_word, uint32_t *out_sample, uint32_t *out_len,
                        uint64_t *info);
int swt_batch_pair_rows_dev(const uint32_t *d_ids, const uint64_t *d_off_a, const uint64_t *d_off_b, uint64_t n_rows, const uint32_t *d_map,
                            uint32_t n_map, int flagged, const uint32_t *d_spans, const uint32_t *d_word, const swt_batch_spec *spec,
                            uint32_t strategy, const uint64_t *d_row_base, const uint8_t *d_status, uint64_t rows_cap, void *d_out_ids,
                            uint8_t *d_out_mask, void *d_out_type, uint8_t *d_out_special, int8_t *d_out_seq, uint32_t *d_out_spans,
                            uint32_t *d_out_word, uint32_t *d_out_sample, uint32_t *d_out_len, uint64_t *d_info, void *stream);
int swt_batch_pair_capacity(uint32_t *cols_per_step, uint32_t *scan_group);

/* ------------------------------------------------------------------------------------------------
 * Packed batches: several short source rows share one model row, so that a batch at pre-training widths is tokens and not
 * padding; the model gets the position of every column inside its sentence and a segment number per column to keep attention
 * inside a sentence.  The same post-pass over (ids, tok_off) as swt_batch_rows, with the same dense ids and the same spec: width,
 * pad_id, unk_id, cls_id, sep_id and SWT_BATCH_IDS64 are used; stride must be 0, SWT_BATCH_WINDOWS and SWT_BATCH_PAD_LEFT are
 * refused.  The reference has nothing of the sort; tests/pack_cases.py holds these semantics.
 *
 * A source row r gives a SEGMENT [cls?] body [sep?] of L(r) columns.  P is the exclusive sum of L, T = P[n_rows].
 *   SWT_PACK_WHOLE   no segment is split.  The body is the first min(n, cap) tokens, cap = width - (cls present) - (sep present),
 *                    so L(r) <= width.  Next-fit in source order: a packed row that starts at source row r holds the source rows
 *                    r .. next(r) - 1, next(r) the largest q <= n_rows with P[q] - P[r] <= width; the packed rows are the orbit of
 *                    0 under next.  Segments of no column (an empty text without specials) ride along in the row that is open.
 *                    n_rows >= 1 gives at least one packed row (T == 0: one row of padding).
 *   SWT_PACK_SPLIT   concatenate and cut: no truncation, L(r) = n + specials; the segments are one stream of T columns and packed
 *                    row b holds the stream positions [b width, min(T, (b + 1) width)); rows = ceil(T / width), the last one
 *                    padded.  With SWT_PACK_DROP_LAST (or-ed into the mode; SPLIT only) a last row that is not full is
 *                    dropped: rows = floor(T / width).
 * The plan: slot[n_rows+1], the flat output position row * width + col of every segment's first column (SPLIT: P[r]; WHOLE:
 * bin(r) width + P[r] - P[first row of the bin]), slot[n_rows] the end of the last segment; row_first[n_rows+1], whose first
 * `rows` entries are the source row that owns column 0 of each packed row (WHOLE: the packed row's first source row; SPLIT:
 * the r with P[r] <= b width < P[r+1]) and whose entries from row_first[rows] on are n_rows.  SPLIT can give more packed rows
 * than source rows: row_first then holds the owners of the first n_rows + 1 packed rows, and the row call, which finds a SPLIT
 * row's owner by a search in slot, does not read it.  info[4]: [0] rows out, [1] the longest source row in tokens, [2] 0, [3] T
 * (WHOLE: after truncation).
 *
 * The rows, [rows, width] each: out_ids (int32, int64 with SWT_BATCH_IDS64; padding pad_id) and out_mask (uint8; 0) are
 * required.  out_pos (uint32; may be NULL): the column's position inside its segment, stream position - P[r], 0 on the cls --
 * in SPLIT it carries on across a cut; padding 0.  out_seg (uint32; may be NULL): r - row_first[row]; padding 0xFFFFFFFF.
 * out_doc (uint32; may be NULL): r; padding 0xFFFFFFFF.  out_len[row] (may be NULL): the columns that are not padding.
 * info[3] (may be NULL): [0] rows written, [1] source rows that lost tokens (WHOLE only), [2] tokens sent to unk_id, once per
 * column written.
 *
 * SWT_ERR_INVALID: cap < 1, a stride, SWT_BATCH_WINDOWS, SWT_BATCH_PAD_LEFT, an unknown flag, pad_id / unk_id =
 * SWT_BATCH_NONE, a mode that is not exactly one of WHOLE and SPLIT, SWT_PACK_DROP_LAST without SPLIT, NULL out_ids or out_mask,
 * NULL slot or row_first, flagged without a map, 2^32 source rows or more.  The host forms check everything -- decreasing offsets
 * and a slot / row_first that is not the plan of the offsets included -- before anything touches the device, and swt_pack_rows
 * returns SWT_ERR_CAPACITY with info[0] = the rows needed when they exceed rows_cap.  The `_dev` forms take device pointers
 * (offsets that do not decrease; outputs aligned to their element type, to 16 bytes for the wide stores), enqueue on the stream
 * and do not synchronise; swt_pack_rows_dev writes every element of the rows < min(rows, rows_cap) of every output given and
 * nothing at or beyond rows_cap * width, whatever ids, slot and row_first hold.  swt_pack_plan_dev scans in the workspace of
 * swt_batch_plan_dev and keeps its own beside it: no two plans of any kind at once on different streams.  swt_pack_capacity:
 * the columns one wavefront writes per step, the rows of one scan group, and the rows of one group of the orbit step of the
 * WHOLE plan (csrc/swt_pack.hip). */
#define SWT_PACK_WHOLE 1u
#define SWT_PACK_SPLIT 2u
#define SWT_PACK_DROP_LAST 4u
int swt_pack_plan(const uint64_t *tok_off, uint64_t n_rows, const swt_batch_spec *spec, uint32_t mode, uint64_t *slot, uint64_t *row_first,
                  uint64_t *info);
int swt_pack_plan_dev(const uint64_t *d_tok_off, uint64_t n_rows, const swt_batch_spec *spec, uint32_t mode, uint64_t *d_slot,
                      uint64_t *d_row_first, uint64_t *d_info, void *stream);
int swt_pack_rows(const uint32_t *ids, const uint64_t *tok_off, uint64_t n_rows, const uint32_t *map, uint32_t n_map, int flagged,
                  const swt_batch_spec *spec, uint32_t mode, const uint64_t *slot, const uint64_t *row_first, uint64_t rows_cap, void *out_ids,
                  uint8_t *out_mask, uint32_t *out_pos, uint32_t *out_seg, uint32_t *out_doc, uint32_t *out_len, uint64_t *info);
int swt_pack_rows_dev(const uint32_t *d_ids, const uint64_t *d_tok_off, uint64_t n_rows, const uint32_t *d_map, uint32_t n_map, int flagged,
                      const swt_batch_spec *spec, uint32_t mode, const uint64_t *d_slot, const uint64_t *d_row_first, uint64_t rows_cap,
                      void *d_out_ids, uint8_t *d_out_mask, uint32_t *d_out_pos, uint32_t *d_out_seg, uint32_t *d_out_doc,
                      uint32_t *d_out_len, uint64_t *d_info, void *stream);
int swt_pack_capacity(uint32_t *cols_per_step, uint32_t *scan_group, uint32_t *orbit_group);

/* ------------------------------------------------------------------------------------------------
 * Masked-LM batches: over finished rows ids[rows, width] of dense ids (int32, int64 with SWT_MLM_IDS64; C-contiguous; any
 * input_ids of the batch calls above), the columns the masked-LM objective selects, what stands in their place, and the labels.
 * The reference has nothing of the sort; tests/mlm_cases.py holds these semantics, and the kernel equals it bit for bit.
 *
 * The class of a column comes from cls_tab[n_class] (uint8) at its id: 0 starts a word, 1 continues one ('##' and more), 2 is
 * never masked ([PAD], [UNK], [CLS], [SEP], [MASK]); an id that is negative or >= n_class is class 2, as is any other value of the
 * table.  Nothing but the id decides: there is no attention mask, padding is [PAD].  A column of class 0 or 1 is ELIGIBLE.  It is
 * a HEAD when its class is 0, or when its class is 1 and the column to its left in the row is class 2 or does not exist (a word
 * cut by truncation, a window or a split row); head(c) = the largest head column <= c.  Without SWT_MLM_WHOLE_WORD every
 * eligible column is its own head.
 *
 * A draw is Philox4x32-10 (Random123: multipliers D2511F53 CD9E8D57, Weyl constants 9E3779B9 BB67AE85) of the counter (column,
 * row, epoch, 0) under the key (seed's low word, seed's high word); x0 .. x3 its four output words.  The thresholds
 * select_below, mask_below <= random_below are integers in [0, 2^32]: there is no floating point on the device.
 *   an eligible column c is SELECTED iff x0 of the draw at (head(c), row) < select_below: a word is selected whole;
 *   a selected column, by x1 and x2 of its OWN draw: x1 < mask_below -> mask_id; else x1 < random_below ->
 *   rand_ids[(x2 * n_rand) >> 32]; else its id stays.
 * out_ids: the id of every column not replaced, else the replacement.  out_labels: the id before replacement on selected columns,
 * -100 elsewhere.  out_selected (uint8; may be NULL): 1 on selected columns.  info[5] (may be NULL): eligible columns, selected,
 * replaced by mask_id, replaced by a random id, selected and kept.  The result is a function of (seed, epoch, row, column) and the
 * row's content alone -- not of the launch, of the other rows of the call or of the integer width; a new epoch masks the same
 * rows anew.  rand_ids may be NULL when mask_below == random_below: nothing is replaced by a random id.
 *
 * SWT_ERR_INVALID, swt_last_error naming the argument: NULL ids, out_ids, out_labels, cls_tab or spec; width == 0 with rows > 0;
 * 2^32 rows or more; 2^31 columns or more; an unknown flag; a threshold above 2^32 or mask_below > random_below; n_class == 0;
 * rand_ids NULL or n_rand == 0 where a random replacement can be drawn; an output that overlaps ids (a lane reads its
 * neighbours' classes: not in place).  rows == 0 succeeds and zeroes info.  The spec is a host pointer in both forms.  The host
 * form checks everything before anything touches the device.  The `_dev` form takes device pointers (aligned to their element
 * type, to 16 bytes for the wide loads and stores), enqueues on the stream and does not synchronise; it writes every element of
 * every output given and nothing outside rows * width, whatever ids holds, and fills d_info[0..4] (zeroes for no row).  With
 * d_info it keeps the workgroups' counts between its two launches in a workspace of the process: no two such calls at once on
 * different streams.
 * swt_mlm_capacity: the columns of a row one step covers, and the most rows that share a wavefront (csrc/swt_mlm.hip). */
#define SWT_MLM_WHOLE_WORD 1u
#define SWT_MLM_IDS64 4u /* the value of SWT_BATCH_IDS64 */
typedef struct swt_mlm_spec {
  uint64_t seed, select_below, mask_below, random_below;
  uint32_t epoch, flags, mask_id, n_class;
} swt_mlm_spec;
int swt_mlm_mask(const void *ids, uint64_t rows, uint32_t width, const uint8_t *cls_tab, const uint32_t *rand_ids, uint32_t n_rand,
                 const swt_mlm_spec *spec, void *out_ids, void *out_labels, uint8_t *out_selected, uint64_t *info);
int swt_mlm_mask_dev(const void *d_ids, uint64_t rows, uint32_t width, const uint8_t *d_cls_tab, const uint32_t *d_rand_ids, uint32_t n_rand,
                     const swt_mlm_spec *spec, void *d_out_ids, void *d_out_labels, uint8_t *d_out_selected, uint64_t *d_info, void *stream);
int swt_mlm_capacity(uint32_t *cols_per_step, uint32_t *rows_per_wave_max);

/* ------------------------------------------------------------------------------------------------
 * Decoding: finished rows ids[rows, width] of dense ids (int32, int64 with SWT_DECODE_IDS64; C-contiguous; any input_ids of the
 * batch calls above, a model's output) back to text, as the reference's recover_sentence (utils.py:141-154) spells the rows'
 * tokens.  tests/decode_cases.py holds these semantics, tests/golden/recover_sentence.json pins them to the reference's strings,
 * and the kernel equals the model byte for byte.
 *
 * The vocabulary is tok_bytes (the UTF-8 of all tokens in dense-id order), tok_off[n_tok + 1] (uint32) and tok_flags[n_tok]
 * (uint8), the vocabulary's bytes tok_off[n_tok] below 2^23 (a step's bytes are summed in 32 bits).  The bits of tok_flags:
 * GLUE 1 ('##' and at least one more code point), NO_SPACE_BEFORE 2 (the first code point is one of . , ) ] \ U+2019 - ' /),
 * NO_SPACE_AFTER 4 (the last is one of ( [ \ U+2019 - ' /), SPECIAL 8 ([PAD], [CLS], [SEP], [MASK]; not [UNK], which stands for a
 * word of the text), BAD 16 (empty, or holding a code point Python's \s matches: the reference's regular expressions would act
 * inside such a token, and its spelling is not guessed).
 *
 * A column is KEPT when mask (uint8[rows, width], as out_mask of swt_batch_rows; may be NULL) is nonzero there and, with
 * SWT_DECODE_SKIP_SPECIAL, its token is not SPECIAL.  Nothing is looked up for a column whose mask is zero.  A kept column whose
 * id is negative or >= n_tok sets bit 0 of status[row], one whose token is BAD sets bit 1; such a column WRITES nothing and is
 * no neighbour of the columns that do.  Of the writing columns of a row, in order: the first writes its token as it is (a
 * leading '##' stays); a GLUE token after another writes its bytes without the first two and no space; otherwise a token that is
 * NO_SPACE_BEFORE, or follows one that is NO_SPACE_AFTER, writes its bytes; every other writes one space (0x20) and its bytes.
 * There is no terminator.
 *
 * swt_decode_plan: text_off[rows + 1] (uint64), the exclusive sum of the rows' byte lengths; status[rows] (uint8);
 * info[3]: total bytes, rows with a nonzero status, kept columns (those that set a status bit among them).
 * swt_decode_rows: row r's bytes to out_text[text_off[r] .. text_off[r + 1]); SWT_ERR_CAPACITY when text_cap is below the total.
 *
 * SWT_ERR_INVALID, swt_last_error naming the argument: a NULL pointer other than mask; width == 0 with rows > 0; 2^32 rows or
 * more; 2^31 columns or more; an unknown flag; n_tok == 0; in the host forms a tok_off that decreases or ends at 2^23 or more,
 * and for swt_decode_rows a text_off that is not the plan of these ids.
 * rows == 0 succeeds: text_off[0] = 0, info zeroed, nothing written by swt_decode_rows.  The host forms check everything before
 * anything touches the device.  The `_dev` forms take device pointers aligned to their element type, enqueue on the stream and do
 * not synchronise.  swt_decode_rows_dev recomputes every length from ids: it writes nothing at or beyond text_cap and nothing
 * outside [text_off[r], text_off[r + 1]) for row r, whatever ids and text_off hold.  swt_decode_plan_dev scans in the workspace of
 * swt_batch_plan_dev and keeps its workgroups' counts beside it: no two plans of any kind at once on different streams.
 * swt_decode_capacity: the columns of a row one step covers, and the rows of one scan group (csrc/swt_decode.hip). */
#define SWT_DECODE_SKIP_SPECIAL 1u
#define SWT_DECODE_IDS64 4u /* the value of SWT_BATCH_IDS64 */
#define SWT_TOK_GLUE 1u
#define SWT_TOK_NO_SPACE_BEFORE 2u
#define SWT_TOK_NO_SPACE_AFTER 4u
#define SWT_TOK_SPECIAL 8u
#define SWT_TOK_BAD 16u
int swt_decode_plan(const void *ids, const uint8_t *mask, uint64_t rows, uint32_t width, const uint32_t *tok_off, const uint8_t *tok_flags,
                    uint32_t n_tok, uint32_t flags, uint64_t *text_off, uint8_t *status, uint64_t *info);
int swt_decode_plan_dev(const void *d_ids, const uint8_t *d_mask, uint64_t rows, uint32_t width, const uint32_t *d_tok_off,
                        const uint8_t *d_tok_flags, uint32_t n_tok, uint32_t flags, uint64_t *d_text_off, uint8_t *d_status, uint64_t *d_info,
                        void *stream);
int swt_decode_rows(const void *ids, const uint8_t *mask, uint64_t rows, uint32_t width, const uint8_t *tok_bytes, const uint32_t *tok_off,
                    const uint8_t *tok_flags, uint32_t n_tok, uint32_t flags, const uint64_t *text_off, uint8_t *out_text, uint64_t text_cap);
int swt_decode_rows_dev(const void *d_ids, const uint8_t *d_mask, uint64_t rows, uint32_t width, const uint8_t *d_tok_bytes,
                        const uint32_t *d_tok_off, const uint8_t *d_tok_flags, uint32_t n_tok, uint32_t flags, const uint64_t *d_text_off,
                        uint8_t *d_out_text, uint64_t text_cap, void *stream);
int swt_decode_capacity(uint32_t *cols_per_step, uint32_t *scan_group);

/* ------------------------------------------------------------------------------------------------
 * Fine-tuning labels: over the finished rows of the batch calls above -- word[rows, width] (out_word), seq[rows, width] (int8,
 * the pair rows' out_seq), spans[rows, width, 2] (out_spans), sample[rows] (out_sample) and len[rows] (out_len) -- the labels of
 * token classification and of extractive question answering, and the best answer span from a model's logits.  The reference has
 * nothing of the sort; tests/label_cases.py holds these semantics and the kernels equal it element by element.
 *
 * A TOKEN COLUMN of row r is a column c that holds a token of the side in question: seq[r, c] == side (0 or 1) when seq is given,
 * word[r, c] != 0xFFFFFFFF when seq is NULL (single-sentence rows).  sample[r] names the row's text; NULL: row r is text r.  A row
 * with sample[r] >= n_samples gets the "nothing" result of the call and is counted in info where info has a place for it.
 * Labels and positions are int32, int64 with SWT_LABEL_IDS64.
 *
 * 1. swt_label_words: the labels lab[lab_off[s] .. lab_off[s + 1]) (int32; lab_off uint64[n_samples + 1], non-decreasing, ending
 * at or below n_lab) of the words of text s onto its rows.  For column c of row r, s = sample[r], k = word[r, c]:
 *   no token column, or a row of no text: ignore;
 *   k >= lab_off[s + 1] - lab_off[s]: ignore, the column counts in info[2] and out_status[r] (uint8[rows], may be NULL) is 1,
 *     else 0;
 *   c is the FIRST column of its word in this row -- c == 0, or column c - 1 is no token column, or word[r, c - 1] != k:
 *     l = lab[lab_off[s] + k].  A word cut by a window's edge is labelled again in the next window, as the usual recipe does
 *     and as the masked-LM rule treats a cut word;
 *   any other column of the word: ignore; with SWT_LABEL_ALL_TOKENS l, and where inside (int32[n_inside], may be NULL) is given
 *     and 0 <= l < n_inside, inside[l] -- the B-x to I-x map of BIO tagging.
 * info[4] (may be NULL): columns given a label, token columns left at ignore as non-first, token columns whose word has no
 * label, rows of no text (their columns are in none of the first three).
 *
 * 2. swt_answer_positions: the answer's characters ans[s] = (a, e) (uint32[n_samples, 2], in the unit of spans; a == 0xFFFFFFFF
 * or a >= e: the text has no answer) as start and end columns.  C: the token columns of the row in order, c0 the first, c1 the
 * last.  The row HOLDS the answer iff C is not empty, the text has an answer, spans[c0].start <= a and spans[c1].end >= e; then
 * start = max{c in C: spans[c].start <= a}, end = min{c in C: spans[c].end >= e} and out_has[r] = 1.  Otherwise both positions
 * are the NOTHING COLUMN and out_has[r] = 0: with SWT_ANSWER_CLS the [CLS] column -- 0, or with SWT_ANSWER_PAD_LEFT (which needs
 * len) width - len[r], 0 where len[r] is 0 or above the width -- and `ignore` without.  This is the recipe of the usual QA preprocessing with its
 * two scans confined to C; the recipe's first loop runs on into [SEP] and the padding, whose offsets are (0, 0), when the answer
 * starts in the window's last token: that quirk is not reproduced.  out_has (uint8[rows]) and out_hit (uint8[n_samples]; zeroed
 * by the call, 1 where some row holds the text's answer) may be NULL.  info[3] (may be NULL): rows that hold their answer, rows
 * of a text that do not, rows of no text.
 *
 * 3. swt_answer_best: from start_logit and end_logit (float32[rows, width]) the best span of every row and of every text.  The
 * candidates of a row are the pairs of token columns (i, j), i <= j < i + max_len (max_len >= 1; a larger value acts as width);
 * the score is the float32 sum start_logit[i] + end_logit[j], one IEEE addition; a candidate whose score is a NaN is none.  The
 * order: higher score, then smaller i, then smaller j -- total, so that the result does not depend on how it is reduced.  A
 * row's result (out_row_score, out_row_start, out_row_end; each may be NULL) is its first candidate, (-inf, -1, -1) without one;
 * a candidate at -inf is one.  `sample` must not decrease: a text's rows are contiguous, as the window plans emit them (the host
 * form checks; the `_dev` form then leaves which run of such a text is reported undefined, and writes nothing out of place).
 * Per text (all required when n_samples > 0): the first of its rows' results in the order (higher score, smaller row) as
 * out_score, out_row, out_start_col, out_end_col, out_char_start = spans[row, start_col].start, out_char_end =
 * spans[row, end_col].end; (-inf, -1, -1, -1, 0, 0) for a text with no row or no candidate.  out_null_score: with SWT_ANSWER_CLS
 * the least start_logit[cls] + end_logit[cls] over the text's rows that is no NaN (the [CLS] column as in 2.), +inf without such
 * a row or without the flag.  info[2] (may be NULL): rows with a candidate, texts with one.  Fewer than 2^31 rows.
 *
 * SWT_ERR_INVALID, swt_last_error naming the argument: a NULL array that is not optional (word may be NULL in 2. and 3. when seq
 * is given); width == 0 with rows > 0; 2^32 rows or more; 2^31 columns or more; 2^32 texts or more; a side that is not 0 or 1
 * with seq; an unknown flag; an array that is not aligned to its element type; an output that shares a byte with another array;
 * max_len == 0; in the host forms a lab_off that decreases or runs past n_lab, and a sample that decreases in 3.
 * rows == 0 succeeds: info and out_hit zeroed, every text's "nothing" record written.  The host forms check everything before
 * anything touches the device and need none for rows == 0.  The `_dev` forms take device pointers (16-byte alignment lets them
 * take the wide loads and stores), enqueue on the stream and do not synchronise; they write every element of every output given
 * and nothing else.  With d_info (and swt_answer_best_dev always) they keep counts and rows' results between their launches in a
 * workspace of the process: no two such calls at once on different streams.
 * swt_label_capacity: the columns of a row one step covers, and the rows of one workgroup of the reduction over a text's rows
 * (csrc/swt_labels.hip). */
#define SWT_LABEL_ALL_TOKENS 1u
#define SWT_LABEL_IDS64 4u /* the value of SWT_BATCH_IDS64 */
#define SWT_ANSWER_CLS 1u
#define SWT_ANSWER_PAD_LEFT 2u
int swt_label_words(const uint32_t *word, const int8_t *seq, int32_t side, const uint32_t *sample, uint64_t rows, uint32_t width,
                    const uint64_t *lab_off, const int32_t *lab, uint64_t n_lab, uint64_t n_samples, const int32_t *inside, uint32_t n_inside,
                    int32_t ignore, uint32_t flags, void *out_labels, uint8_t *out_status, uint64_t *info);
int swt_label_words_dev(const uint32_t *d_word, const int8_t *d_seq, int32_t side, const uint32_t *d_sample, uint64_t rows, uint32_t width,
                        const uint64_t *d_lab_off, const int32_t *d_lab, uint64_t n_lab, uint64_t n_samples, const int32_t *d_inside,
                        uint32_t n_inside, int32_t ignore, uint32_t flags, void *d_out_labels, uint8_t *d_out_status, uint64_t *d_info,
                        void *stream);
int swt_answer_positions(const uint32_t *spans, const uint32_t *word, const int8_t *seq, int32_t side, const uint32_t *sample, uint64_t rows,
                         uint32_t width, const uint32_t *ans, uint64_t n_samples, const uint32_t *len, int32_t ignore, uint32_t flags,
                         void *out_start, void *out_end, uint8_t *out_has, uint8_t *out_hit, uint64_t *info);
int swt_answer_positions_dev(const uint32_t *d_spans, const uint32_t *d_word, const int8_t *d_seq, int32_t side, const uint32_t *d_sample,
                             uint64_t rows, uint32_t width, const uint32_t *d_ans, uint64_t n_samples, const uint32_t *d_len, int32_t ignore,
                             uint32_t flags, void *d_out_start, void *d_out_end, uint8_t *d_out_has, uint8_t *d_out_hit, uint64_t *d_info,
                             void *stream);
int swt_answer_best(const float *start_logit, const float *end_logit, const uint32_t *spans, const uint32_t *word, const int8_t *seq, int32_t side,
                    const uint32_t *sample, uint64_t rows, uint32_t width, uint64_t n_samples, uint32_t max_len, const uint32_t *len,
                    uint32_t flags, float *out_score, float *out_null_score, int32_t *out_row, int32_t *out_start_col, int32_t *out_end_col,
                    uint32_t *out_char_start, uint32_t *out_char_end, float *out_row_score, int32_t *out_row_start, int32_t *out_row_end,
                    uint64_t *info);
int swt_answer_best_dev(const float *d_start_logit, const float *d_end_logit, const uint32_t *d_spans, const uint32_t *d_word, const int8_t *d_seq,
                        int32_t side, const uint32_t *d_sample, uint64_t rows, uint32_t width, uint64_t n_samples, uint32_t max_len,
                        const uint32_t *d_len, uint32_t flags, float *d_out_score, float *d_out_null_score, int32_t *d_out_row,
                        int32_t *d_out_start_col, int32_t *d_out_end_col, uint32_t *d_out_char_start, uint32_t *d_out_char_end,
                        float *d_out_row_score, int32_t *d_out_row_start, int32_t *d_out_row_end, uint64_t *d_info, void *stream);
int swt_label_capacity(uint32_t *cols_per_step, uint32_t *scan_rows);

/* ------------------------------------------------------------------------------------------------
 * Token-classification inference: from a model's logits (float32[rows, width, n_labels], C-contiguous, n_labels >= 1, fewer
 * than 2^40 elements) over the same finished rows, one label and score per WORD of every text and the words' BIO grouping into
 * entities.  The conventions are those of the labels block above: token columns of `side`, sample (NULL: row r is text r; a row
 * with sample[r] >= n_samples is a row of no text), the argument checks, the `_dev` forms.  The reference has nothing of the
 * sort; tests/tag_cases.py holds these semantics.
 *
 * A RUN of row r is a maximal set of consecutive token columns with the same word id k: the first-column rule of
 * swt_label_words, continued to the right.  `sample` must not decrease (as in swt_answer_best; the host forms check, the `_dev`
 * forms then leave the affected texts' results undefined and write nothing out of place).
 *
 * 1. swt_word_plan: n_words[s] = 1 + the greatest word[r, c] over the token columns of the rows of text s, 0 for a text with no
 * token column; out_word_off (uint64[n_samples + 1]) is its exclusive prefix sum.  info[2] (required): out_word_off[n_samples],
 * rows of no text.  The plan half of a plan / rows pair, as swt_decode_plan: the caller reads the total back and sizes the
 * per-word arrays of 2. and 3. with it.
 *
 * 2. swt_word_predict: per word, at index w = word_off[s] + k of arrays of n_words elements (word_off as 1. made it, or any
 * other that does not decrease and ends at or below n_words), each of which may be NULL: out_label (int32), out_score (float32),
 * out_row, out_col, out_ncols (int32), out_char_start, out_char_end (uint32), out_logits (float32[n_words, n_labels]).
 *   WHICH RUN SPEAKS FOR A WORD.  The context of a run is min(token columns of the side left of its first column, token columns
 *   of the side right of its last column), both in its row -- the "max context" of the original BERT span code.  Among the runs
 *   of (s, k) over all rows of s the winner has the greater context, then the smaller row, then the smaller first column: a
 *   total order, so that the result does not depend on how it is reduced.  A word cut by a window's edge has context 0 there.
 *   A run of a row of no text, and a run with k >= word_off[s + 1] - word_off[s] or word_off[s] + k >= n_words, takes no part
 *   and counts in info[3].
 *   THE WORD'S VECTOR v[0, n_labels) from the winner's columns c_0 < ... < c_{n-1}, x = logits[row]:
 *     SWT_TAG_FIRST  v_l = x[c_0, l]
 *     SWT_TAG_MEAN   v_l = (((x[c_0, l] + x[c_1, l]) + ...) + x[c_{n-1}, l]) / float32(n): float32 IEEE additions in column
 *                    order, then one IEEE division -- the order is part of the contract
 *     SWT_TAG_MAX    v_l = the greatest x[c_i, l] that is no NaN, NaN if all are
 *   out_label: the smallest l whose v_l is no NaN and >= every entry that is no NaN; -1 if all are NaN.  Exact.
 *   out_score: with m = v[label], 1 / sum over l in order of expf(v_l - m), in float32: the softmax probability of the label.
 *   NaN and +-inf go through as IEEE has them: a NaN entry makes the score NaN while the label stands; label -1 has score NaN.
 *   out_row, out_col = c_0, out_ncols = n; out_char_start = spans[row, c_0].start, out_char_end = spans[row, c_{n-1}].end;
 *   out_logits = v.
 *   A WORD WITH NO RUN: label -1, score 0, row, col and ncols -1, characters (0, 0), out_logits all NaN.
 * info[4] (may be NULL): words with a run, words without, runs that lost to another row's run, runs that take no part.
 * Fewer than 2^31 rows; n_words * n_labels below 2^40; SWT_ERR_INVALID where bits(width) * 2 + bits(rows - 1) exceeds 64 (a
 * run's context, row and column make one 64-bit key): with fewer than 2^40 logits that needs a width of 2^21 columns or more.
 *
 * 3. swt_entity_spans: over the word arrays of 2. (label, score, char_start, char_end; n_words each) and the label scheme etype
 * (int32[n_labels]; -1: outside) and begins (uint8[n_labels]).  Word w of text s (word_off[s] <= w < word_off[s + 1]; a word at
 * or beyond word_off[n_samples] is of no text and of no entity) has the type t_w = etype[label_w], -1 for a label outside
 * [0, n_labels).  It HEADS an entity iff t_w >= 0 and it is the first word of its text, or t_{w-1} != t_w, or begins[label_w];
 * the entity runs through the following words of the text that have the same type and are no heads.  Records, n_words of each
 * (all required when n_words > 0), in the order of the heads: ent_text, ent_type, ent_first_word, ent_last_word (int32; the
 * words as indices in the text), ent_char_start of the head, ent_char_end of the last word (uint32), ent_score (float32): the
 * words' scores added in order from the first, float32 IEEE additions, divided by float32(count).  Every record at or beyond
 * the count is (-1, -1, -1, -1, 0, 0, 0.0).  info[2] (may be NULL): entities, words inside entities.
 *
 * SWT_ERR_INVALID also for: a NULL array that is not optional (seq, sample and the outputs of 2. are), the shapes the labels
 * block refuses, n_labels == 0, an unknown strategy, misalignment to the element type, an output sharing a byte with another
 * array; in the host forms a sample or word_off that decreases, and a word_off that ends beyond n_words.  rows == 0 (n_words
 * == 0 in 3.) succeeds without a device: the offsets and info zeroed, every word's "nothing" record written.  The `_dev` forms
 * enqueue on the stream, do not synchronise, write every element of every output given and nothing else; they keep keys,
 * flags and counts in a workspace of the process, and 1. and 3. scan in the workspace of the plans: no two such calls at once on
 * different streams.
 * swt_tag_capacity: the columns of a row one step covers, the rows of one workgroup of the reduction over a text's rows (also
 * the words of one workgroup of the per-word kernels), and the words of one group of the entity scan (csrc/swt_tags.hip). */
#define SWT_TAG_FIRST 0u
#define SWT_TAG_MEAN 1u
#define SWT_TAG_MAX 2u
int swt_word_plan(const uint32_t *word, const int8_t *seq, int32_t side, const uint32_t *sample, uint64_t rows, uint32_t width,
                  uint64_t n_samples, uint64_t *out_word_off, uint64_t *info);
int swt_word_plan_dev(const uint32_t *d_word, const int8_t *d_seq, int32_t side, const uint32_t *d_sample, uint64_t rows, uint32_t width,
                      uint64_t n_samples, uint64_t *d_out_word_off, uint64_t *d_info, void *stream);
int swt_word_predict(const float *logits, const uint32_t *word, const int8_t *seq, int32_t side, const uint32_t *sample, const uint32_t *spans,
                     uint64_t rows, uint32_t width, uint32_t n_labels, const uint64_t *word_off, uint64_t n_samples, uint64_t n_words,
                     uint32_t strategy, int32_t *out_label, float *out_score, int32_t *out_row, int32_t *out_col, int32_t *out_ncols,
                     uint32_t *out_char_start, uint32_t *out_char_end, float *out_logits, uint64_t *info);
int swt_word_predict_dev(const float *d_logits, const uint32_t *d_word, const int8_t *d_seq, int32_t side, const uint32_t *d_sample,
                         const uint32_t *d_spans, uint64_t rows, uint32_t width, uint32_t n_labels, const uint64_t *d_word_off,
                         uint64_t n_samples, uint64_t n_words, uint32_t strategy, int32_t *d_out_label, float *d_out_score, int32_t *d_out_row,
                         int32_t *d_out_col, int32_t *d_out_ncols, uint32_t *d_out_char_start, uint32_t *d_out_char_end, float *d_out_logits,
                         uint64_t *d_info, void *stream);
int swt_entity_spans(const int32_t *label, const float *score, const uint32_t *char_start, const uint32_t *char_end, const uint64_t *word_off,
                     uint64_t n_samples, uint64_t n_words, const int32_t *etype, const uint8_t *begins, uint32_t n_labels, int32_t *ent_text,
                     int32_t *ent_type, int32_t *ent_first_word, int32_t *ent_last_word, uint32_t *ent_char_start, uint32_t *ent_char_end,
                     float *ent_score, uint64_t *info);
int swt_entity_spans_dev(const int32_t *d_label, const float *d_score, const uint32_t *d_char_start, const uint32_t *d_char_end,
                         const uint64_t *d_word_off, uint64_t n_samples, uint64_t n_words, const int32_t *d_etype, const uint8_t *d_begins,
                         uint32_t n_labels, int32_t *d_ent_text, int32_t *d_ent_type, int32_t *d_ent_first_word, int32_t *d_ent_last_word,
                         uint32_t *d_ent_char_start, uint32_t *d_ent_char_end, float *d_ent_score, uint64_t *d_info, void *stream);
int swt_tag_capacity(uint32_t *cols_per_step, uint32_t *text_rows, uint32_t *scan_words);

/* ------------------------------------------------------------------------------------------------
 * Masked-LM inference: from a model's logits (float32[rows, width, n_vocab], C-contiguous, aligned to 4 bytes and no more) the
 * scores of SELECTED cells only -- the counterpart of the masked-LM block above, which makes the masked rows and their labels.
 * A cell is named by its flat index row * width + col.  The reference has nothing of the sort; tests/fill_cases.py holds these
 * semantics.  The argument checks and the `_dev` forms follow the labels block.
 *
 * 1. swt_mlm_positions: over ids[rows, width] (int32, int64 with SWT_FILL_IDS64; any input_ids or labels of the calls above) the
 * cells with ids == value (SWT_FILL_EQUAL: input_ids == [MASK]) or ids != value (SWT_FILL_NOT_EQUAL: labels != -100); the compare
 * is signed, of the id widened to 64 bits.  out_pos (uint64[rows * width]): the flat indices of the selected cells in ascending
 * order, every element from the count on UINT64_MAX.  info[2] (required): the count, the cells looked at.  The plan half of a
 * plan / rows pair: the caller reads the count back and sizes the arrays of 2. with it.  Fewer than 2^32 cells.
 *
 * 2. swt_mlm_predict: for position p < n_pos the row x[0, n_vocab) = logits[pos[p]] is read, and nothing of any other cell.
 * labels[rows, width] (int32, int64 with SWT_FILL_IDS64) may be NULL, and then the three label outputs must be; 0 <= k <= 64,
 * and k == 0 needs out_top_id and out_top_logit NULL.  Every output may be NULL.
 *   THE ORDER of the entries of a row that are no NaN: the greater logit first (-0.0 == 0.0), among equal logits the smaller
 *   index.  It is total, so that nothing below depends on how it is reduced.  A NaN is never in it.
 *   out_lse[p] (float32) = m + logf(S), m = max x_i, S = sum of expf(x_i - m), in float32.  NaN when any entry is a NaN, -inf
 *   when m is -inf, +inf when m is +inf.  The order of the additions is the kernel's own and THE ONLY THING HERE THAT IS NOT
 *   EXACT: with s = floats_per_step of swt_fill_capacity a term expf(x_i - m) passes at most
 *       chain(V) = min(V - 1, ceil(V / s) + 8)
 *   float32 additions with another nonzero term -- ceil(V / s) in its lane (a sum per column of the lane's quad, one addition a
 *   step, and a lane has ceil(quads / 64) <= ceil(V / s) steps; the first sum starts from the lane's float of the peeled head
 *   or tail, which costs no addition), 2 to add the lane's four sums, 6 over the wavefront; V - 1 is what any order is held to.
 *   There is no rescaling: m is the exact maximum from a pass before.  x_i - m is one IEEE subtraction, expf and logf are
 *   libm's (1 ulp).  tests/fill_cases.py makes its tolerance of exactly this.
 *   out_top_id[p, k] (int32), out_top_logit[p, k] (float32, a bit copy of the input): the first k entries in the order; the
 *   slots beyond the number of entries that are no NaN hold id -1 and logit NaN.
 *   out_label_id[p] (int32): l = labels[pos[p]] where 0 <= l < n_vocab, else -1.  out_label_logit[p] (float32, a bit copy):
 *   x[l], NaN for a label out of range.  out_label_rank[p] (int32): the entries that come before (x[l], l) in the order -- 0
 *   for the argmax of the smallest index; -1 for a label out of range or one whose logit is a NaN.
 *   info[5] (may be NULL): positions, labels of rank 0, labels of rank 0 <= r < max(k, 1), positions whose row holds a NaN,
 *   labels out of range.  Without labels the second, third and fifth are 0.
 *   A pos[p] >= rows * width is SWT_ERR_INVALID in the host form.  The `_dev` form gives such a position the "nothing" record --
 *   lse NaN, ids -1, logits NaN, rank -1 -- counts it as a position and in nothing else, and reads neither logits nor labels.
 * Log-probabilities and probabilities are top_logit - lse and its exp over n_pos * k elements: the callers make them.
 *
 * SWT_ERR_INVALID, swt_last_error naming the argument: NULL ids, out_pos, info (1.), logits, pos (2.); width == 0 with rows > 0;
 * 2^32 rows or more; 2^31 columns or more; an unknown mode or flag; n_vocab == 0 or >= 2^31; k > 64; rows * width * n_vocab
 * >= 2^62; 2^32 positions or more; top outputs with k == 0; label outputs without labels; an array that is not aligned to its
 * element type; an output that shares a byte with another array.  Zero rows (1.) and zero positions (2.) succeed without a
 * device, info zeroed.  The host forms check everything before anything touches the device.  The `_dev` forms take device
 * pointers, enqueue on the stream and do not synchronise; they write every element of every output given and nothing else,
 * whatever the inputs hold.  They keep the workgroups' counts in a workspace of the process, and 1. scans in the workspace of
 * the plans: no two such calls at once on different streams.
 * swt_fill_capacity: the floats of a row one step of a wavefront covers (s above), the positions of one workgroup of 2., the
 * greatest k, and the cells of one scan group of 1. (csrc/swt_fill.hip). */
#define SWT_FILL_EQUAL 0u
#define SWT_FILL_NOT_EQUAL 1u
#define SWT_FILL_IDS64 4u /* the value of SWT_BATCH_IDS64 */
int swt_mlm_positions(const void *ids, uint64_t rows, uint32_t width, int64_t value, uint32_t mode, uint32_t flags, uint64_t *out_pos,
                      uint64_t *info);
int swt_mlm_positions_dev(const void *d_ids, uint64_t rows, uint32_t width, int64_t value, uint32_t mode, uint32_t flags, uint64_t *d_out_pos,
                          uint64_t *d_info, void *stream);
int swt_mlm_predict(const float *logits, uint64_t rows, uint32_t width, uint64_t n_vocab, const uint64_t *pos, uint64_t n_pos, const void *labels,
                    uint32_t flags, uint32_t k, float *out_lse, int32_t *out_top_id, float *out_top_logit, int32_t *out_label_id,
                    float *out_label_logit, int32_t *out_label_rank, uint64_t *info);
int swt_mlm_predict_dev(const float *d_logits, uint64_t rows, uint32_t width, uint64_t n_vocab, const uint64_t *d_pos, uint64_t n_pos,
                        const void *d_labels, uint32_t flags, uint32_t k, float *d_out_lse, int32_t *d_out_top_id, float *d_out_top_logit,
                        int32_t *d_out_label_id, float *d_out_label_logit, int32_t *d_out_label_rank, uint64_t *d_info, void *stream);
int swt_fill_capacity(uint32_t *floats_per_step, uint32_t *positions_per_workgroup, uint32_t *k_max, uint32_t *scan_cells);

/* ------------------------------------------------------------------------------------------------
 * Added and special tokens written in the text ("[MASK]", "[SEP]", "<user>", a domain term kept whole): one stage in front of the
 * encoders, which finds them and hides them from the pre-tokenizer, and one behind, which splices them into the encoders'
 * streams.  No encoder and no row kernel knows of them.  The reference has nothing of the sort; the `tokenizers` wheel calls it
 * the added vocabulary.  tests/added_cases.py holds these semantics as plain Python.
 *
 * PATTERNS.  A handle holds n patterns (1 .. 4096), pattern k the bytes [pat_off[k], pat_off[k + 1]) of pat_bytes: 1 .. 64 bytes
 * of strict UTF-8 -- no surrogate, no code point past U+FFFF, no U+0000, no code point of class SWT_CLS_BERT_WS -- and no
 * pattern twice; anything else is SWT_ERR_INVALID, swt_last_error saying why.  The caller lowercases: the patterns are matched
 * against the text the encoders see (the lowercased UTF-8 of the callers).  swt_added_create needs no device; the tables go up
 * with the first find.  The handle keeps a byte trie with a table of the root's children by first byte in front (the
 * first-byte reject): the work of a text position is bounded by the longest pattern, not by the number of patterns
 * (csrc/swt_added.h, where the lookup "the longest pattern that matches here" is one function for host and device).
 *
 * 1. swt_added_find: over the texts [sent_off[s], sent_off[s + 1]) of `text`.
 *   THE MATCHES of a text: among the patterns that match at a byte position the longest wins; scanning from the left, a match
 *   is taken at the first position that has one and does not lie inside the match before it, and the scan goes on at the
 *   match's end: leftmost-longest, non-overlapping.  A match never crosses a text's end.  Matches may lie inside a word.
 *   out_text (n_bytes, a buffer of its own): the text with every code point of every match overwritten by a whitespace code
 *   point of the same UTF-8 length -- U+0020, U+00A0, U+2003 -- so that the byte and code-point offsets of everything else stay
 *   what they were; every other byte is a copy.
 *   m_off (uint64[n_sent + 1]): the matches of text s are [m_off[s], m_off[s + 1]), in text order.  m_pat (uint32): the pattern.
 *   m_span (uint32[2] per match): the match's (start, end) in code points inside its text, the unit of SWT_SPAN_CODEPOINTS; a
 *   code point is a byte that is no continuation byte (10xxxxxx), which on well-formed UTF-8 is the count of the span calls.
 *   info[3] (required): matches, texts with a match, bytes blanked.
 *   SIZES.  A match takes a byte at least, so a call has no more matches than bytes: the `_dev` form takes m_pat of n_bytes and
 *   m_span of 2 * n_bytes elements and needs no plan call.  Between its kernels the matches stand in a grow-only workspace of
 *   the handle (12 bytes per text byte), as swt_token_spans_dev keeps one: no two calls on one handle at once on different
 *   streams; the counts are scanned in the workspace of the plans.  The host form takes m_cap, the matches m_pat and m_span
 *   have room for; with more matches it returns SWT_ERR_CAPACITY, out_text, m_off and info written.
 *
 * 2. swt_added_splice: the matches into the four streams of a span call over the blanked text (ids, tok_off, spans in code
 * points, word).  With j = the matches of its text that start before a token's span, the token moves j slots up and its word
 * index grows by j; with i = the tokens of its text that start before a match, match k of the text takes slot i + k of the
 * text's new run, its span is m_span, its id added_base + m_pat (never flagged with SWT_BPE_CONT), and it is a word of its own:
 * the word after that of the token before it, the first where there is none, plus k.  out_tok_off[s] = tok_off[s] + m_off[s].
 * The outputs are arrays of their own with room for tok_off[n_sent] + m_off[n_sent] tokens, which is no more than n_bytes.
 * Spans that do not ascend inside a text give an arrangement that is not defined, inside the text's own run.
 *
 * The `_dev` forms take device pointers, enqueue on the stream and do not synchronise.  n_sent == 0, and for 1. n_bytes == 0,
 * succeed with the offsets and info zeroed.  Fewer than 2^32 texts, each of fewer than 2^32 bytes: the host form refuses a longer
 * one, the `_dev` form takes it for an empty text.
 * swt_added_capacity: the bytes of one step of a wavefront's walk through a text, the bytes of halo staged behind a step (a match
 * may straddle a step), the bytes of one tile, the greatest number of patterns and of bytes of a pattern (csrc/swt_added.hip). */
typedef struct swt_added swt_added;
int swt_added_create(const uint8_t *pat_bytes, const uint64_t *pat_off, uint32_t n, swt_added **out);
void swt_added_destroy(swt_added *h);
int swt_added_find(swt_added *h, const uint8_t *text, const uint64_t *sent_off, uint64_t n_sent, uint8_t *out_text, uint64_t *m_off,
                   uint32_t *m_pat, uint32_t *m_span, uint64_t m_cap, uint64_t *info);
int swt_added_find_dev(swt_added *h, const uint8_t *d_text, uint64_t n_bytes, const uint64_t *d_sent_off, uint64_t n_sent, uint8_t *d_out_text,
                       uint64_t *d_m_off, uint32_t *d_m_pat, uint32_t *d_m_span, uint64_t *d_info, void *stream);
int swt_added_splice(const uint32_t *ids, const uint64_t *tok_off, const uint32_t *spans, const uint32_t *word, uint64_t n_sent,
                     const uint64_t *m_off, const uint32_t *m_pat, const uint32_t *m_span, uint32_t added_base, uint32_t *out_ids,
                     uint64_t *out_tok_off, uint32_t *out_spans, uint32_t *out_word);
int swt_added_splice_dev(const uint32_t *d_ids, const uint64_t *d_tok_off, const uint32_t *d_spans, const uint32_t *d_word, uint64_t n_sent,
                         const uint64_t *d_m_off, const uint32_t *d_m_pat, const uint32_t *d_m_span, uint32_t added_base, uint32_t *d_out_ids,
                         uint64_t *d_out_tok_off, uint32_t *d_out_spans, uint32_t *d_out_word, void *stream);
int swt_added_capacity(uint32_t *step_bytes, uint32_t *halo_bytes, uint32_t *tile_bytes, uint32_t *max_patterns, uint32_t *max_pattern_bytes);
#ifdef __cplusplus
}
#endif
#endif /* SWT_H */
