// swt_spans.hip -- token spans on the device: for every token of an id stream, the characters of the text it came from
// (offset_mapping) and the index of its pre-tokenizer word (word_ids).
//
// Rests on one fact about NaiveBPE, FastBPE and NaiveWP: the tokens of a sentence are grouped by pre-tokenizer word
// (source/utils.py:15-29, SubwordTokenizer.preprocessing) and the tokens of a word tile it -- each token covers
// as many code points as its string has after the '##', and NaiveWP's "[UNK]" (source/wordpiece.py:132-159)
// covers its whole word.  So nothing is encoded again: one pass over the text (the split) and one over the ids (the lengths).
//
// token_spans_kernel, one wavefront per sentence, a workgroup of four per tile (a tile owns the sentences whose first byte lies
// in its kSpTile bytes of text: swt_tile.h, launch_plan):
//   text pass   the sentence in chunks of kSpChunk bytes staged in the wave's LDS (16-byte loads), each chunk in blocks of
//               kSpBlock = 64 bytes, one byte per lane.  Code-point starts, whitespace, punctuation and word starts are
//               ballot masks, so every rank a lane needs is a popcount: no scan.  Carried from block to block (and so from
//               chunk to chunk): the lead/continuation masks of the last three bytes, whether the last code point left a run
//               open, and the running counts of code points, non-whitespace code points and words.  Leaves in the workspace,
//               at the sentence's own byte offset (a sentence never has more words or code points than bytes):
//                 cp[b0 + r]  = (start, end) of the sentence's r-th non-whitespace code point, in the caller's unit
//                 wr[b0 + k]  = r of the first code point of its k-th word
//   token pass  the sentence's ids in blocks of 64, one token per lane.  A group starts at a token that is not a continuation;
//               the group index is a popcount over the ballot of heads, the prefix inside the group a wave scan cut at the
//               last head.  Carried: groups so far, the open group's prefix.  Token t of group g with prefix P and length L
//               covers the code points wr[g] + P .. wr[g] + P + L - 1 of the sentence: its span is cp[first].start,
//               cp[last].end.  A sentence of more than 64 tokens is walked twice, first to validate (a sentence that does not
//               tile gets zeros everywhere), then to write; a shorter one once.
// Output slots are the input token slots: no compaction, no scan over sentences, no atomics.
#include "swt_tile.h"

namespace swt {

constexpr int kSpThreads = 256;
constexpr int kSpWaves = kSpThreads / 64;
constexpr uint32_t kSpBlock = 64;
constexpr uint32_t kSpChunk = 1024;
constexpr uint32_t kSpTile = 2048;
constexpr uint32_t kSpStage = kSpChunk + 32;  // 15 bytes of alignment in front, 3 bytes of look-ahead behind, rounded to 16
constexpr uint32_t kSpBadSentence = 0xFFFFFFFFu;
static_assert(kSpChunk % kSpBlock == 0 && kSpChunk == 64 * 16, "one 16-byte load per lane stages a chunk");

struct SpanArgs {
  const uint8_t *text;
  uint64_t n_bytes;
  const uint64_t *sent_off;
  const uint32_t *ids;
  const uint64_t *tok_off;
  const uint32_t *len;
  uint32_t len_base, n_len;
  int flagged;
  uint32_t flags;
  uint32_t *spans, *word;
  uint8_t *status;
  const uint64_t *plan;
  const uint8_t *cls_tab;
  uint2 *cp;     // workspace, n_bytes entries
  uint32_t *wr;  // workspace, n_bytes entries
};

struct SpanLds {
  __attribute__((aligned(16))) uint8_t txt[kSpWaves][kSpStage];
  __attribute__((aligned(16))) uint8_t cls_lo[1024];
};

__device__ __forceinline__ unsigned long long sp_shl(unsigned long long x, unsigned long long prev, int k) {
  return (x << k) | (prev >> (64 - k));
}

// The split of one sentence [b0, b1).  Returns (words, non-whitespace code points).
__device__ __forceinline__ uint2 sp_text_pass(const SpanArgs &A, uint8_t *txt, const uint8_t *cls_lo, uint64_t b0, uint64_t b1, int lane) {
  const unsigned long long lt = (1ull << lane) - 1ull;
  const bool unit_cp = (A.flags & SWT_SPAN_CODEPOINTS) != 0;
  unsigned long long pC = 0, pG1 = 0, pG2 = 0, pG3 = 0;  // the previous block's masks, its last byte at bit 63
  bool prev_run = false;                                 // the last code point so far belongs to a run that may go on
  uint32_t n_cp = 0, n_nw = 0, n_words = 0;
  for (uint64_t cb = b0; cb < b1; cb += kSpChunk) {
    const uint64_t abase = cb & ~15ull;
    const uint32_t off0 = (uint32_t)(cb - abase);
    const uint32_t n = b1 - cb < (uint64_t)kSpChunk ? (uint32_t)(b1 - cb) : kSpChunk;
    const uint32_t need = off0 + n + 3;  // <= 15 + 1024 + 3 < kSpStage
    __builtin_amdgcn_wave_barrier();     // the last chunk's reads are done
    for (uint32_t c = lane * 16; c < need; c += 64 * 16) {
      const uint64_t g = abase + c;
      if (g + 16 <= A.n_bytes && ((reinterpret_cast<uintptr_t>(A.text + g) & 15) == 0)) {
        *reinterpret_cast<uint4 *>(&txt[c]) = *reinterpret_cast<const uint4 *>(A.text + g);
      } else {
        for (int i = 0; i < 16; i++) txt[c + i] = (g + i < A.n_bytes) ? A.text[g + i] : (uint8_t)' ';
      }
    }
    __builtin_amdgcn_wave_barrier();
    for (uint32_t base = 0; base < n; base += kSpBlock) {
      const uint32_t q = base + lane;  // byte of the chunk
      const bool inr = q < n;
      const uint32_t valid = n - base < kSpBlock ? n - base : kSpBlock;  // bytes of this block, >= 1
      const uint8_t *p = txt + off0 + q;
      const uint8_t b = inr ? p[0] : (uint8_t)' ';
      const bool multi = b >= 0xC0 && b < 0xF8;
      const unsigned long long C = __ballot(inr && utf8_is_cont(b));
      const unsigned long long G1 = __ballot(inr && multi), G2 = __ballot(inr && multi && b >= 0xE0), G3 = __ballot(inr && multi && b >= 0xF0);
      // a continuation byte belongs to the lead 1, 2 or 3 bytes back when that lead is long enough and only continuation
      // bytes lie between; every other byte starts a code point (a stray continuation byte is one code point)
      const unsigned long long C1 = sp_shl(C, pC, 1), C2 = sp_shl(C, pC, 2);
      const unsigned long long covered = C & (sp_shl(G1, pG1, 1) | (sp_shl(G2, pG2, 2) & C1) | (sp_shl(G3, pG3, 3) & C1 & C2));
      const unsigned long long INR = valid == 64 ? ~0ull : ((1ull << valid) - 1ull);
      const unsigned long long START = INR & ~covered;
      const bool st = (START >> lane) & 1ull;
      uint32_t cp = b, blen = 1;
      if (st && multi) {
        const int want = utf8_len(b);
        cp = b & (0xFF >> (want + 1));
        const uint64_t left = b1 - (cb + q);  // bytes of the sentence from this one on, >= 1
        for (int i = 1; i < want && (uint64_t)i < left && utf8_is_cont(p[i]); i++) { cp = (cp << 6) | (p[i] & 0x3F); blen++; }
      }
      uint8_t c = 0;
      if (st) c = cp < 1024u ? cls_lo[cp] : (cp < kNumCodePoints ? A.cls_tab[cp] : (uint8_t)0);
      const unsigned long long WS = __ballot(st && (c & SWT_CLS_BERT_WS));
      const unsigned long long PN = __ballot(st && (c & SWT_CLS_BERT_PUNCT)) & ~WS;
      const unsigned long long NW = START & ~WS;
      const unsigned long long RUN = NW & ~PN;  // code points that leave a run open
      bool after_run = prev_run;
      const unsigned long long before = START & lt;
      if (before) after_run = (RUN >> (63 - __builtin_clzll(before))) & 1ull;
      const bool nw = (NW >> lane) & 1ull;
      const unsigned long long WSTART = __ballot(nw && (((PN >> lane) & 1ull) || !after_run));
      const uint32_t r = n_nw + __popcll(NW & lt);
      if (nw) {
        const uint32_t s = unit_cp ? n_cp + __popcll(START & lt) : (uint32_t)(cb + q - b0);
        A.cp[b0 + r] = make_uint2(s, s + (unit_cp ? 1u : blen));
      }
      if ((WSTART >> lane) & 1ull) A.wr[b0 + n_words + __popcll(WSTART & lt)] = r;
      n_cp += __popcll(START);
      n_nw += __popcll(NW);
      n_words += __popcll(WSTART);
      if (START) prev_run = (RUN >> (63 - __builtin_clzll(START))) & 1ull;
      const int up = 64 - (int)valid;  // a short block ends its chunk: its last byte goes to bit 63 all the same
      pC = C << up; pG1 = G1 << up; pG2 = G2 << up; pG3 = G3 << up;
    }
  }
  return make_uint2(n_words, n_nw);
}

struct SpTokCarry {
  uint32_t groups;            // groups begun so far
  unsigned long long prefix;  // code points of the open group so far
};

struct SpTok {
  uint32_t group;  // index of the token's group (0xFFFFFFFF: a continuation with no head in front)
  unsigned long long prefix;
  uint32_t len;    // code points; 0: the whole word
  bool bad;        // this lane saw something that does not tile
};

// Length entry of one id (include/swt.h): code points covered (0: the whole word), continuation, or no length at all.
__device__ __forceinline__ void sp_token_info(const SpanArgs &A, uint32_t id, uint32_t &len, bool &cont, bool &nolen) {
  const uint32_t s = id & 0x7FFFFFFFu;
  cont = A.flagged && (id >> 31);
  if (s < A.len_base) {
    len = 1;
  } else if (s - A.len_base >= A.n_len) {
    nolen = true;
  } else {
    const uint32_t e = A.len[s - A.len_base];
    len = e & 0xFFFFFFu;
    if (!A.flagged) cont = e >> 31;
  }
}

// One block of up to 64 tokens [t, t + valid) of a sentence with n_words words and n_nw non-whitespace code points.
// last_block: the sentence ends with this block.
__device__ __forceinline__ SpTok sp_token_block(const SpanArgs &A, uint64_t b0, uint32_t n_words, uint32_t n_nw, uint64_t t, uint32_t valid,
                                                bool last_block, SpTokCarry &K, int lane) {
  SpTok T;
  const bool act = (uint32_t)lane < valid;
  uint32_t len = 0;
  bool cont = false, nolen = false;
  if (act) sp_token_info(A, A.ids[t + lane], len, cont, nolen);
  // the block's last token closes its group when the sentence ends here or the next block opens with a head
  bool closes = last_block;
  if (!last_block && (uint32_t)lane + 1 == valid) {
    uint32_t len2 = 0;
    bool cont2 = false, nolen2 = false;
    sp_token_info(A, A.ids[t + valid], len2, cont2, nolen2);
    closes = !cont2;
  }
  const unsigned long long H = __ballot(act && !cont);
  const unsigned long long le = lane == 63 ? ~0ull : ((2ull << lane) - 1ull);
  const unsigned long long heads = H & le;
  T.group = K.groups + (uint32_t)__popcll(heads) - 1u;
  // inclusive wave scan of the lengths, cut at the token's head
  unsigned long long incl = len;
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long v = __shfl_up(incl, d, 64);
    if (lane >= d) incl += v;
  }
  const unsigned long long excl = incl - len;
  const int head_lane = heads ? 63 - __builtin_clzll(heads) : 0;
  const unsigned long long at_head = __shfl(excl, head_lane, 64);
  T.prefix = heads ? excl - at_head : K.prefix + excl;
  T.len = len;
  const bool is_head = act && !cont;
  const bool is_last = act && (((uint32_t)lane + 1 < valid) ? (((H >> (lane + 1)) & 1ull) != 0) : closes);
  bool bad = nolen || (act && T.group == 0xFFFFFFFFu) || (act && T.group != 0xFFFFFFFFu && T.group >= n_words);
  if (act && !bad) {
    if (len == 0 && !(is_head && is_last)) bad = true;  // the whole-word token has company
    if (is_last && len != 0) {
      const uint32_t w0 = A.wr[b0 + T.group], w1 = T.group + 1 < n_words ? A.wr[b0 + T.group + 1] : n_nw;
      if (T.prefix + len != (unsigned long long)(w1 - w0)) bad = true;
    }
  }
  T.bad = bad;
  // carry: the open group is the one of the last token
  const int last_lane = (int)valid - 1;
  const unsigned long long p_end = __shfl(T.prefix + len, last_lane, 64);
  K.groups += (uint32_t)__popcll(H);
  K.prefix = p_end;
  return T;
}

__device__ __forceinline__ void sp_write(const SpanArgs &A, uint64_t b0, uint32_t n_words, uint32_t n_nw, uint64_t t, const SpTok &T, bool ok) {
  uint32_t s = 0, e = 0, w = 0;
  if (ok) {
    const uint32_t w0 = A.wr[b0 + T.group];
    uint32_t L = T.len;
    if (!L) L = (T.group + 1 < n_words ? A.wr[b0 + T.group + 1] : n_nw) - w0;
    const uint64_t first = b0 + w0 + T.prefix;
    s = A.cp[first].x;
    e = A.cp[first + L - 1].y;
    w = T.group;
  }
  A.spans[2 * t] = s;
  A.spans[2 * t + 1] = e;
  if (A.word) A.word[t] = w;
}

__global__ __launch_bounds__(kSpThreads) void token_spans_kernel(SpanArgs A) {
  __shared__ SpanLds L;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t tile = blockIdx.x;
  const uint64_t s_lo = A.plan[tile], s_hi = A.plan[tile + 1];
  if (s_lo == s_hi) return;
  if (threadIdx.x < 64) reinterpret_cast<uint4 *>(L.cls_lo)[threadIdx.x] = reinterpret_cast<const uint4 *>(A.cls_tab)[threadIdx.x];
  __syncthreads();
  for (uint64_t s = s_lo + wave; s < s_hi; s += kSpWaves) {
    const uint64_t b0 = A.sent_off[s], b1 = A.sent_off[s + 1];
    const uint64_t t0 = A.tok_off[s], t1 = A.tok_off[s + 1];
    if (t1 < t0) {  // nothing of this sentence can be written
      if (lane == 0) A.status[s] = SWT_SPAN_MISMATCH;
      continue;
    }
    uint2 m = make_uint2(kSpBadSentence, 0);
    if (b0 <= b1 && b1 <= A.n_bytes && b1 - b0 < (1ull << 32)) {
      m = sp_text_pass(A, L.txt[wave], L.cls_lo, b0, b1, lane);
      __threadfence_block();  // the workspace entries are read back by other lanes of this wave
    }
    const uint32_t n_words = m.x, n_nw = m.y;
    bool ok = n_words != kSpBadSentence;
    const uint64_t n_tok = t1 - t0;
    SpTokCarry K{0, 0};
    if (n_tok <= 64) {
      SpTok T{0, 0, 0, false};
      if (ok && n_tok) {
        T = sp_token_block(A, b0, n_words, n_nw, t0, (uint32_t)n_tok, true, K, lane);
        ok = !__any(T.bad);
      }
      ok = ok && K.groups == n_words;
      if ((uint64_t)lane < n_tok) sp_write(A, b0, n_words, n_nw, t0 + lane, T, ok);
    } else {
      if (ok) {
        bool bad = false;
        for (uint64_t t = t0; t < t1; t += 64) {
          const uint32_t valid = t1 - t < 64 ? (uint32_t)(t1 - t) : 64u;
          bad |= sp_token_block(A, b0, n_words, n_nw, t, valid, t + 64 >= t1, K, lane).bad;
        }
        ok = !__any(bad) && K.groups == n_words;
      }
      K = SpTokCarry{0, 0};
      for (uint64_t t = t0; t < t1; t += 64) {
        const uint32_t valid = t1 - t < 64 ? (uint32_t)(t1 - t) : 64u;
        SpTok T{0, 0, 0, false};
        if (ok) T = sp_token_block(A, b0, n_words, n_nw, t, valid, t + 64 >= t1, K, lane);
        if ((uint32_t)lane < valid) sp_write(A, b0, n_words, n_nw, t + lane, T, ok);
      }
    }
    if (lane == 0) A.status[s] = ok ? SWT_SPAN_OK : SWT_SPAN_MISMATCH;
  }
}

// grow-only, shared by all calls of the process (the calls carry no handle); a call uses it on its own stream, so calls
// on different streams must not overlap -- the header says so
struct SpanWorkspace {
  DevBuf plan, cp, wr;
};
static SpanWorkspace g_span_ws;

}  // namespace swt

using namespace swt;

extern "C" {

int swt_token_spans_capacity(uint32_t *block, uint32_t *chunk, uint32_t *tile) try {
  if (block) *block = kSpBlock;
  if (chunk) *chunk = kSpChunk;
  if (tile) *tile = kSpTile;
  return SWT_OK;
} SWT_API_CATCH

int swt_token_spans_dev(const uint8_t *d_text, uint64_t n_bytes, const uint64_t *d_sent_off, uint64_t n_sent, const uint32_t *d_ids,
                        const uint64_t *d_tok_off, const uint32_t *d_len, uint32_t len_base, uint32_t n_len, int flagged, uint32_t flags,
                        uint32_t *d_spans, uint32_t *d_word, uint8_t *d_status, void *stream) try {
  if (!n_sent) return SWT_OK;
  if ((n_bytes && !d_text) || !d_sent_off || !d_tok_off || !d_ids || (n_len && !d_len) || !d_spans || !d_status)
    return fail(SWT_ERR_INVALID, "null argument");
  if (flags & ~SWT_SPAN_CODEPOINTS) return fail(SWT_ERR_INVALID, "unknown flag");
  int rc = ensure_device();
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const uint8_t *d_cls = nullptr;
  if ((rc = device_class_table(&d_cls))) return rc;
  const uint64_t n_tiles = tile_count(n_bytes, kSpTile);
  SpanWorkspace &ws = g_span_ws;
  if ((rc = ws.plan.reserve((n_tiles + 1) * 8)) || (rc = ws.cp.reserve((size_t)n_bytes * 8 + 16)) || (rc = ws.wr.reserve((size_t)n_bytes * 4 + 16))) return rc;
  launch_plan(d_sent_off, n_sent, n_tiles, kSpTile, ws.plan.as<uint64_t>(), st);
  SWT_HIP(hipGetLastError());
  SpanArgs A{d_text, n_bytes, d_sent_off, d_ids, d_tok_off, d_len, len_base, n_len, flagged, flags, d_spans, d_word, d_status,
             ws.plan.as<uint64_t>(), d_cls, ws.cp.as<uint2>(), ws.wr.as<uint32_t>()};
  prof_begin(st);
  hipLaunchKernelGGL(token_spans_kernel, dim3((unsigned)n_tiles), dim3(kSpThreads), 0, st, A);
  prof_end(st);
  SWT_HIP(hipGetLastError());
  return SWT_OK;
} SWT_API_CATCH

int swt_token_spans(const uint8_t *text, const uint64_t *sent_off, uint64_t n_sent, const uint32_t *ids, const uint64_t *tok_off,
                    const uint32_t *len, uint32_t len_base, uint32_t n_len, int flagged, uint32_t flags, uint32_t *spans, uint32_t *word,
                    uint8_t *status) try {
  if (!n_sent) return SWT_OK;
  if (!sent_off || !tok_off || !status) return fail(SWT_ERR_INVALID, "null argument");
  if (flags & ~SWT_SPAN_CODEPOINTS) return fail(SWT_ERR_INVALID, "unknown flag");
  for (uint64_t s = 0; s < n_sent; s++) {
    if (sent_off[s] > sent_off[s + 1] || tok_off[s] > tok_off[s + 1]) return fail(SWT_ERR_INVALID, "offsets must not decrease");
    if (sent_off[s + 1] - sent_off[s] >= (1ull << 32)) return fail(SWT_ERR_INVALID, "a sentence of 2^32 bytes or more");
  }
  const uint64_t n_bytes = sent_off[n_sent], n_tok = tok_off[n_sent];
  if ((n_bytes && !text) || (n_tok && (!ids || !spans)) || (n_len && !len)) return fail(SWT_ERR_INVALID, "null argument");
  int rc = ensure_device();
  if (rc) return rc;
  DevBuf d[8];  // text, sentence offsets, ids, token offsets, lengths; spans, word, status
  struct Guard { DevBuf *d; ~Guard() { for (int i = 0; i < 8; i++) d[i].release(); } } guard{d};
  const void *src[5] = {text, sent_off, ids, tok_off, len};
  const size_t bytes[8] = {(size_t)n_bytes, (size_t)(n_sent + 1) * 8, (size_t)n_tok * 4, (size_t)(n_sent + 1) * 8, (size_t)n_len * 4,
                           (size_t)n_tok * 8, word ? (size_t)n_tok * 4 : 0, (size_t)n_sent};
  for (int i = 0; i < 8; i++) {
    if ((rc = d[i].reserve(bytes[i] + 16))) return rc;
    if (i < 5 && bytes[i]) SWT_HIP(hipMemcpy(d[i].p, src[i], bytes[i], hipMemcpyHostToDevice));
  }
  if ((rc = swt_token_spans_dev(d[0].as<uint8_t>(), n_bytes, d[1].as<uint64_t>(), n_sent, d[2].as<uint32_t>(), d[3].as<uint64_t>(),
                                d[4].as<uint32_t>(), len_base, n_len, flagged, flags, d[5].as<uint32_t>(), word ? d[6].as<uint32_t>() : nullptr,
                                d[7].as<uint8_t>(), nullptr)))
    return rc;
  SWT_HIP(hipStreamSynchronize(nullptr));
  if (n_tok) SWT_HIP(hipMemcpy(spans, d[5].p, (size_t)n_tok * 8, hipMemcpyDeviceToHost));
  if (n_tok && word) SWT_HIP(hipMemcpy(word, d[6].p, (size_t)n_tok * 4, hipMemcpyDeviceToHost));
  SWT_HIP(hipMemcpy(status, d[7].p, (size_t)n_sent, hipMemcpyDeviceToHost));
  return SWT_OK;
} SWT_API_CATCH

}  // extern "C"
