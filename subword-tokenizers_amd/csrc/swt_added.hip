// swt_added.hip -- added and special tokens written in the text: found and blanked in front of the encoders, spliced into
// their streams behind them (include/swt.h has the rule; csrc/swt_added.h the pattern table and the per-position lookup).
//
// added_find_kernel, one wavefront per text, a workgroup of four per tile (a tile owns the texts whose first byte lies in its
// kAdTile bytes: swt_tile.h, launch_plan).  The wave walks its text in steps of kAdStep bytes staged in its LDS with a halo of
// kAddedMaxBytes - 1 bytes behind, so that a match may straddle a step; a step in blocks of 64 positions, one per lane:
//   reject   root[byte] == 0 (the table of the root's children, in LDS): no pattern starts here.  The common block ends after
//            the ballot of the lanes that pass.
//   lookup   a lane that passes walks the trie over the staged bytes (added_longest): the longest pattern at its position.
//   choose   a scalar loop over the set bits of the ballot applies the leftmost-longest rule with the carried `blocked`: the
//            first position a match may start at.
//   write    a chosen lane writes its match -- pattern, code-point span -- to the workspace at the text's own byte offset plus
//            the match's rank (a text never has more matches than bytes) and overwrites the match's bytes in the output text.
// The running code-point count is a popcount over the ballot of the bytes that are no continuation bytes.  The output text is a
// device copy of the input made before the kernel, so the kernel stores the blanked bytes and nothing else.
// The counts of the texts are scanned in the workspace of the plans (launch_scan_bases) into m_off, and added_compact_kernel
// moves the matches from the workspace to their places.
//
// added_splice_kernel, one wavefront per text: a token moves up by the matches of its text that start before it (a search in
// the text's matches), a match takes the slot after the tokens that start before it (a search in the text's tokens).
#include "swt_added.h"
#include "swt_batch.h"
#include "swt_tile.h"

namespace swt {

constexpr int kAdThreads = 256;
constexpr int kAdWaves = kAdThreads / 64;
constexpr uint32_t kAdStep = 1024;
constexpr uint32_t kAdHalo = kAddedMaxBytes - 1;
constexpr uint32_t kAdTile = 2048;
constexpr uint32_t kAdStage = 16 + kAdStep + 64;  // 15 bytes of alignment in front, the halo behind, rounded to 16
static_assert(kAdStage % 16 == 0 && 15 + kAdStep + kAdHalo <= kAdStage, "the stage holds a step, its halo and the alignment");

struct FindArgs {
  AddedTable T;
  const uint8_t *text;
  uint64_t n_bytes;
  const uint64_t *sent_off;
  const uint64_t *plan;
  uint8_t *out_text;
  unsigned long long *count;  // per text (m_off before the scan)
  uint32_t *ws_pat;           // workspace, n_bytes entries
  uint2 *ws_span;             // workspace, n_bytes entries
  unsigned long long *info;
};

__global__ __launch_bounds__(kAdThreads) void added_find_kernel(FindArgs A) {
  __shared__ __attribute__((aligned(16))) uint8_t s_txt[kAdWaves][kAdStage];
  __shared__ uint32_t s_root[256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t s_lo = A.plan[blockIdx.x], s_hi = A.plan[blockIdx.x + 1];
  if (s_lo == s_hi) return;
  s_root[threadIdx.x] = A.T.root[threadIdx.x];
  __syncthreads();
  uint8_t *txt = s_txt[wave];
  const unsigned long long lt = (1ull << lane) - 1ull;
  unsigned long long texts_hit = 0, bytes_hit = 0;
  for (uint64_t s = s_lo + wave; s < s_hi; s += kAdWaves) {
    uint64_t b0 = A.sent_off[s], b1 = A.sent_off[s + 1];
    // offsets that name no text, or one of 2^32 bytes or more (the host form refuses it; the counts are 32 bits): an empty one
    if (!(b0 <= b1 && b1 <= A.n_bytes && b1 - b0 < (1ull << 32))) b1 = b0 = 0;
    uint64_t blocked = b0;                            // the first byte a match may start at
    uint32_t n_cp = 0, n_match = 0;
    for (uint64_t cb = b0; cb < b1; cb += kAdStep) {
      const uint64_t abase = cb & ~15ull;
      const uint32_t off0 = (uint32_t)(cb - abase);
      const uint32_t n = b1 - cb < (uint64_t)kAdStep ? (uint32_t)(b1 - cb) : kAdStep;  // positions of this step
      const uint64_t left = b1 - cb;                                                    // bytes of the text from cb on
      const uint32_t have = left < (uint64_t)(n + kAdHalo) ? (uint32_t)left : n + kAdHalo;  // staged bytes that are the text's
      const uint32_t need = off0 + have;                                                // <= 15 + kAdStep + kAdHalo <= kAdStage
      __builtin_amdgcn_wave_barrier();  // the last step's reads are done
      for (uint32_t c = lane * 16; c < need; c += 64 * 16) {
        const uint64_t g = abase + c;
        if (g + 16 <= A.n_bytes && ((reinterpret_cast<uintptr_t>(A.text + g) & 15) == 0)) {
          *reinterpret_cast<uint4 *>(&txt[c]) = *reinterpret_cast<const uint4 *>(A.text + g);
        } else {
          for (int i = 0; i < 16; i++) txt[c + i] = (g + i < A.n_bytes) ? A.text[g + i] : (uint8_t)' ';
        }
      }
      __builtin_amdgcn_wave_barrier();
      for (uint32_t base = 0; base < n; base += 64) {
        const uint32_t q = base + lane;
        const bool inr = q < n;
        const uint8_t *p = txt + off0 + q;  // read only where inr
        const uint8_t b = inr ? p[0] : (uint8_t)' ';
        const unsigned long long START = __ballot(inr && !utf8_is_cont(b));
        const uint64_t pos = cb + q;
        uint32_t len = 0, pat = 0;
        if (inr && s_root[b] && pos >= blocked) {  // (`blocked` only grows: a position behind it is never chosen)
          AddedTable T = A.T;
          T.root = s_root;
          len = added_longest(T, p, have - q, &pat);
        }
        unsigned long long cand = __ballot(len != 0);
        if (cand) {
          unsigned long long taken = 0;
          while (cand) {
            const int i = __builtin_ctzll(cand);
            cand &= cand - 1;
            const uint64_t at = cb + base + i;
            if (at < blocked) continue;
            blocked = at + (uint32_t)__shfl((int)len, i, 64);
            taken |= 1ull << i;
          }
          if ((taken >> lane) & 1ull) {
            uint32_t cps = 0;
            uint8_t lead = 0;
            uint32_t k = 0;
            for (uint32_t i = 0; i < len; i++) {
              const uint8_t c = p[i];
              if (!utf8_is_cont(c)) { cps++; lead = c; k = 0; }
              A.out_text[pos + i] = added_blank_byte(lead, k++);
            }
            const uint32_t start = n_cp + (uint32_t)__popcll(START & lt);
            const uint64_t slot = b0 + n_match + (uint32_t)__popcll(taken & lt);
            A.ws_pat[slot] = pat;
            A.ws_span[slot] = make_uint2(start, start + cps);
            bytes_hit += len;
          }
          n_match += (uint32_t)__popcll(taken);
        }
        n_cp += (uint32_t)__popcll(START);
      }
    }
    if (lane == 0) {
      A.count[s] = n_match;
      if (n_match) texts_hit++;
    }
  }
  for (int d = 32; d; d >>= 1) bytes_hit += __shfl_xor(bytes_hit, d, 64);
  if (lane == 0 && texts_hit) {
    atomicAdd(&A.info[1], texts_hit);
    atomicAdd(&A.info[2], bytes_hit);
  }
}

// the matches of every text from the workspace to [m_off[s], m_off[s + 1])
__global__ __launch_bounds__(kAdThreads) void added_compact_kernel(const uint64_t *__restrict__ sent_off, uint64_t n_bytes,
                                                                   const uint64_t *__restrict__ plan, const uint64_t *__restrict__ m_off,
                                                                   const uint32_t *__restrict__ ws_pat, const uint2 *__restrict__ ws_span,
                                                                   uint32_t *__restrict__ m_pat, uint32_t *__restrict__ m_span) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t s_lo = plan[blockIdx.x], s_hi = plan[blockIdx.x + 1];
  for (uint64_t s = s_lo + wave; s < s_hi; s += kAdWaves) {
    const uint64_t m0 = m_off[s], n = m_off[s + 1] - m0, b0 = sent_off[s];
    if (b0 > n_bytes || n > n_bytes - b0) continue;  // (a count comes from a text of at least as many bytes)
    for (uint64_t k = lane; k < n; k += 64) {
      m_pat[m0 + k] = ws_pat[b0 + k];
      const uint2 sp = ws_span[b0 + k];
      m_span[2 * (m0 + k)] = sp.x;
      m_span[2 * (m0 + k) + 1] = sp.y;
    }
  }
}

struct SpliceArgs {
  const uint32_t *ids;
  const uint64_t *tok_off;
  const uint32_t *spans, *word;
  uint64_t n_sent;
  const uint64_t *m_off;
  const uint32_t *m_pat, *m_span;
  uint32_t added_base;
  uint32_t *out_ids;
  uint64_t *out_tok_off;
  uint32_t *out_spans, *out_word;
};

__global__ __launch_bounds__(kAdThreads) void added_splice_kernel(SpliceArgs A) {
  const int lane = threadIdx.x & 63;
  const uint64_t s = (uint64_t)blockIdx.x * kAdWaves + (threadIdx.x >> 6);
  if (s >= A.n_sent) return;
  const uint64_t t0 = A.tok_off[s], t1 = A.tok_off[s + 1], m0 = A.m_off[s], m1 = A.m_off[s + 1];
  if (lane == 0) {
    A.out_tok_off[s] = t0 + m0;
    if (s + 1 == A.n_sent) A.out_tok_off[s + 1] = t1 + m1;
  }
  if (t1 < t0 || m1 < m0) return;
  const uint64_t nt = t1 - t0, nm = m1 - m0, o0 = t0 + m0;
  for (uint64_t i = lane; i < nt; i += 64) {
    const uint32_t start = A.spans[2 * (t0 + i)];
    uint64_t lo = 0, hi = nm;  // j = the matches that start before the token
    while (lo < hi) {
      const uint64_t mid = (lo + hi) >> 1;
      if (A.m_span[2 * (m0 + mid)] < start) lo = mid + 1; else hi = mid;
    }
    const uint64_t o = o0 + i + lo;
    A.out_ids[o] = A.ids[t0 + i];
    A.out_spans[2 * o] = start;
    A.out_spans[2 * o + 1] = A.spans[2 * (t0 + i) + 1];
    A.out_word[o] = A.word[t0 + i] + (uint32_t)lo;
  }
  for (uint64_t k = lane; k < nm; k += 64) {
    const uint32_t start = A.m_span[2 * (m0 + k)];
    uint64_t lo = 0, hi = nt;  // i = the tokens that start before the match
    while (lo < hi) {
      const uint64_t mid = (lo + hi) >> 1;
      if (A.spans[2 * (t0 + mid)] < start) lo = mid + 1; else hi = mid;
    }
    const uint64_t o = o0 + lo + k;
    A.out_ids[o] = A.added_base + A.m_pat[m0 + k];
    A.out_spans[2 * o] = start;
    A.out_spans[2 * o + 1] = A.m_span[2 * (m0 + k) + 1];
    A.out_word[o] = (lo ? A.word[t0 + lo - 1] + 1u : 0u) + (uint32_t)k;
  }
}

}  // namespace swt

using namespace swt;

struct swt_added {
  AddedHost H;
  uint32_t *d_root = nullptr, *d_end = nullptr;
  uint64_t *d_edges = nullptr;
  DevBuf plan, ws_pat, ws_span;  // grow-only, the handle's own: calls on one handle must not overlap on different streams
};

static int added_upload(swt_added *h) {
  if (h->d_root) return SWT_OK;
  const AddedHost &H = h->H;
  // the handle takes the three tables together, after the last copy: a failure on the way frees what was allocated
  void *p[3] = {nullptr, nullptr, nullptr};
  const void *src[3] = {H.root.data(), H.end.data(), H.edges.data()};
  const size_t bytes[3] = {256 * 4, H.end.size() * 4, H.edges.size() * 8};
  hipError_t e = hipSuccess;
  for (int i = 0; i < 3 && e == hipSuccess; i++) {
    e = hipMalloc(&p[i], bytes[i]);
    if (e == hipSuccess) e = hipMemcpy(p[i], src[i], bytes[i], hipMemcpyHostToDevice);
  }
  if (e != hipSuccess) {
    for (int i = 0; i < 3; i++)
      if (p[i]) (void)hipFree(p[i]);
    return fail(e == hipErrorOutOfMemory ? SWT_ERR_NOMEM : SWT_ERR_HIP, "the added-token tables did not go up: %s", hipGetErrorString(e));
  }
  h->d_end = static_cast<uint32_t *>(p[1]);
  h->d_edges = static_cast<uint64_t *>(p[2]);
  h->d_root = static_cast<uint32_t *>(p[0]);
  return SWT_OK;
}

extern "C" {

int swt_added_capacity(uint32_t *step_bytes, uint32_t *halo_bytes, uint32_t *tile_bytes, uint32_t *max_patterns,
                       uint32_t *max_pattern_bytes) try {
  if (step_bytes) *step_bytes = kAdStep;
  if (halo_bytes) *halo_bytes = kAdHalo;
  if (tile_bytes) *tile_bytes = kAdTile;
  if (max_patterns) *max_patterns = kAddedMaxPatterns;
  if (max_pattern_bytes) *max_pattern_bytes = kAddedMaxBytes;
  return SWT_OK;
} SWT_API_CATCH

int swt_added_create(const uint8_t *pat_bytes, const uint64_t *pat_off, uint32_t n, swt_added **out) try {
  if (!out || !pat_off || !pat_bytes) return fail(SWT_ERR_INVALID, "null argument");
  *out = nullptr;
  auto *h = new swt_added();
  const char *why = h->H.build(pat_bytes, pat_off, n, host_class_table(), SWT_CLS_BERT_WS);
  if (why) {
    delete h;
    return fail(SWT_ERR_INVALID, "added tokens: %s", why);
  }
  *out = h;
  return SWT_OK;
} SWT_API_CATCH

void swt_added_destroy(swt_added *h) try {
  if (!h) return;
  if (h->d_root) (void)hipFree(h->d_root);
  if (h->d_end) (void)hipFree(h->d_end);
  if (h->d_edges) (void)hipFree(h->d_edges);
  h->plan.release();
  h->ws_pat.release();
  h->ws_span.release();
  delete h;
} SWT_API_CATCH_VOID

int swt_added_find_dev(swt_added *h, const uint8_t *d_text, uint64_t n_bytes, const uint64_t *d_sent_off, uint64_t n_sent, uint8_t *d_out_text,
                       uint64_t *d_m_off, uint32_t *d_m_pat, uint32_t *d_m_span, uint64_t *d_info, void *stream) try {
  if (!h || !d_m_off || !d_info || (n_sent && !d_sent_off) || (n_bytes && (!d_text || !d_out_text || !d_m_pat || !d_m_span)))
    return fail(SWT_ERR_INVALID, "null argument");
  if (n_bytes && d_out_text == d_text) return fail(SWT_ERR_INVALID, "the blanked text needs a buffer of its own");
  if (n_sent > 0xFFFFFFFFull) return fail(SWT_ERR_INVALID, "2^32 texts or more");
  int rc = ensure_device();
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  SWT_HIP(hipMemsetAsync(d_info, 0, 24, st));
  if (!n_sent || !n_bytes) {
    SWT_HIP(hipMemsetAsync(d_m_off, 0, (size_t)(n_sent + 1) * 8, st));
    return SWT_OK;
  }
  if ((rc = added_upload(h))) return rc;
  const uint64_t n_tiles = tile_count(n_bytes, kAdTile);
  if ((rc = h->plan.reserve((n_tiles + 1) * 8)) || (rc = h->ws_pat.reserve((size_t)n_bytes * 4 + 16)) ||
      (rc = h->ws_span.reserve((size_t)n_bytes * 8 + 16)) || (rc = g_batch_ws.reserve(n_sent)))
    return rc;
  SWT_HIP(hipMemcpyAsync(d_out_text, d_text, (size_t)n_bytes, hipMemcpyDeviceToDevice, st));
  launch_plan(d_sent_off, n_sent, n_tiles, kAdTile, h->plan.as<uint64_t>(), st);
  SWT_HIP(hipGetLastError());
  unsigned long long *count = reinterpret_cast<unsigned long long *>(d_m_off);
  FindArgs A{AddedTable{h->d_root, h->d_edges, h->d_end, h->H.bits, h->H.max_len}, d_text, n_bytes, d_sent_off, h->plan.as<uint64_t>(),
             d_out_text, count, h->ws_pat.as<uint32_t>(), h->ws_span.as<uint2>(), reinterpret_cast<unsigned long long *>(d_info)};
  prof_begin(st);
  hipLaunchKernelGGL(added_find_kernel, dim3((unsigned)n_tiles), dim3(kAdThreads), 0, st, A);
  prof_end(st);
  launch_scan_bases(n_sent, count, d_info, st);  // the counts to offsets, the total to m_off[n_sent] and info[0]
  hipLaunchKernelGGL(added_compact_kernel, dim3((unsigned)n_tiles), dim3(kAdThreads), 0, st, d_sent_off, n_bytes, h->plan.as<uint64_t>(), d_m_off,
                     h->ws_pat.as<uint32_t>(), h->ws_span.as<uint2>(), d_m_pat, d_m_span);
  SWT_HIP(hipGetLastError());
  return SWT_OK;
} SWT_API_CATCH

int swt_added_find(swt_added *h, const uint8_t *text, const uint64_t *sent_off, uint64_t n_sent, uint8_t *out_text, uint64_t *m_off,
                   uint32_t *m_pat, uint32_t *m_span, uint64_t m_cap, uint64_t *info) try {
  if (!h || !m_off || !info || (n_sent && !sent_off)) return fail(SWT_ERR_INVALID, "null argument");
  if (n_sent > 0xFFFFFFFFull) return fail(SWT_ERR_INVALID, "2^32 texts or more");
  for (uint64_t s = 0; s < n_sent; s++) {
    if (sent_off[s] > sent_off[s + 1]) return fail(SWT_ERR_INVALID, "offsets must not decrease");
    if (sent_off[s + 1] - sent_off[s] >= (1ull << 32)) return fail(SWT_ERR_INVALID, "a text of 2^32 bytes or more");
  }
  const uint64_t n_bytes = n_sent ? sent_off[n_sent] : 0;
  if (n_bytes && (!text || !out_text)) return fail(SWT_ERR_INVALID, "null argument");
  if (n_bytes && out_text == text) return fail(SWT_ERR_INVALID, "the blanked text needs a buffer of its own");
  if (!n_sent || !n_bytes) {
    for (uint64_t s = 0; s <= n_sent; s++) m_off[s] = 0;
    info[0] = info[1] = info[2] = 0;
    return SWT_OK;
  }
  int rc = ensure_device();
  if (rc) return rc;
  BatchStage S;
  const uint8_t *d_text = S.in(text, (size_t)n_bytes);
  const uint64_t *d_off = S.in(sent_off, (size_t)(n_sent + 1) * 8);
  uint8_t *d_out = S.out(out_text, (size_t)n_bytes);
  uint64_t *d_m_off = S.out(m_off, (size_t)(n_sent + 1) * 8), *d_info = S.out(info, 24);
  uint32_t *d_pat = static_cast<uint32_t *>(S.room((size_t)n_bytes * 4)), *d_span = static_cast<uint32_t *>(S.room((size_t)n_bytes * 8));
  if (S.rc) return S.rc;
  if ((rc = swt_added_find_dev(h, d_text, n_bytes, d_off, n_sent, d_out, d_m_off, d_pat, d_span, d_info, nullptr))) return rc;
  if ((rc = S.fetch())) return rc;
  if (info[0] > m_cap) return fail(SWT_ERR_CAPACITY, "%llu matches, room for %llu", (unsigned long long)info[0], (unsigned long long)m_cap);
  if (info[0] && (!m_pat || !m_span)) return fail(SWT_ERR_INVALID, "null argument");
  if ((rc = S.copy(m_pat, d_pat, (size_t)info[0] * 4, hipMemcpyDeviceToHost)) || (rc = S.copy(m_span, d_span, (size_t)info[0] * 8, hipMemcpyDeviceToHost)))
    return rc;
  return SWT_OK;
} SWT_API_CATCH

int swt_added_splice_dev(const uint32_t *d_ids, const uint64_t *d_tok_off, const uint32_t *d_spans, const uint32_t *d_word, uint64_t n_sent,
                         const uint64_t *d_m_off, const uint32_t *d_m_pat, const uint32_t *d_m_span, uint32_t added_base, uint32_t *d_out_ids,
                         uint64_t *d_out_tok_off, uint32_t *d_out_spans, uint32_t *d_out_word, void *stream) try {
  if (!d_out_tok_off) return fail(SWT_ERR_INVALID, "null argument");
  int rc = ensure_device();
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (!n_sent) {
    SWT_HIP(hipMemsetAsync(d_out_tok_off, 0, 8, st));
    return SWT_OK;
  }
  if (!d_ids || !d_tok_off || !d_spans || !d_word || !d_m_off || !d_m_pat || !d_m_span || !d_out_ids || !d_out_spans || !d_out_word)
    return fail(SWT_ERR_INVALID, "null argument");
  if (n_sent > 0xFFFFFFFFull) return fail(SWT_ERR_INVALID, "2^32 texts or more");
  SpliceArgs A{d_ids, d_tok_off, d_spans, d_word, n_sent, d_m_off, d_m_pat, d_m_span, added_base, d_out_ids, d_out_tok_off, d_out_spans, d_out_word};
  hipLaunchKernelGGL(added_splice_kernel, dim3((unsigned)((n_sent + kAdWaves - 1) / kAdWaves)), dim3(kAdThreads), 0, st, A);
  SWT_HIP(hipGetLastError());
  return SWT_OK;
} SWT_API_CATCH

int swt_added_splice(const uint32_t *ids, const uint64_t *tok_off, const uint32_t *spans, const uint32_t *word, uint64_t n_sent,
                     const uint64_t *m_off, const uint32_t *m_pat, const uint32_t *m_span, uint32_t added_base, uint32_t *out_ids,
                     uint64_t *out_tok_off, uint32_t *out_spans, uint32_t *out_word) try {
  if (!out_tok_off) return fail(SWT_ERR_INVALID, "null argument");
  if (!n_sent) {
    out_tok_off[0] = 0;
    return SWT_OK;
  }
  if (!tok_off || !m_off) return fail(SWT_ERR_INVALID, "null argument");
  if (n_sent > 0xFFFFFFFFull) return fail(SWT_ERR_INVALID, "2^32 texts or more");
  if (tok_off[0] || m_off[0]) return fail(SWT_ERR_INVALID, "offsets start at 0");
  for (uint64_t s = 0; s < n_sent; s++)
    if (tok_off[s] > tok_off[s + 1] || m_off[s] > m_off[s + 1]) return fail(SWT_ERR_INVALID, "offsets must not decrease");
  const size_t n_tok = (size_t)tok_off[n_sent], n_m = (size_t)m_off[n_sent], n_out = n_tok + n_m;
  if ((n_tok && (!ids || !spans || !word)) || (n_m && (!m_pat || !m_span)) || (n_out && (!out_ids || !out_spans || !out_word)))
    return fail(SWT_ERR_INVALID, "null argument");
  int rc = ensure_device();
  if (rc) return rc;
  BatchStage S;
  const uint32_t *d_ids = S.in(ids, n_tok * 4, true), *d_spans = S.in(spans, n_tok * 8, true), *d_word = S.in(word, n_tok * 4, true);
  const uint64_t *d_tok_off = S.in(tok_off, (size_t)(n_sent + 1) * 8), *d_m_off = S.in(m_off, (size_t)(n_sent + 1) * 8);
  const uint32_t *d_m_pat = S.in(m_pat, n_m * 4, true), *d_m_span = S.in(m_span, n_m * 8, true);
  uint64_t *d_out_off = S.out(out_tok_off, (size_t)(n_sent + 1) * 8);
  uint32_t *d_out_ids = static_cast<uint32_t *>(S.room(n_out * 4)), *d_out_spans = static_cast<uint32_t *>(S.room(n_out * 8)),
           *d_out_word = static_cast<uint32_t *>(S.room(n_out * 4));
  if (S.rc) return S.rc;
  if (n_out) {
    S.outs.push_back({out_ids, d_out_ids, n_out * 4});
    S.outs.push_back({out_spans, d_out_spans, n_out * 8});
    S.outs.push_back({out_word, d_out_word, n_out * 4});
  }
  if ((rc = swt_added_splice_dev(d_ids, d_tok_off, d_spans, d_word, n_sent, d_m_off, d_m_pat, d_m_span, added_base, d_out_ids, d_out_off,
                                 d_out_spans, d_out_word, nullptr)))
    return rc;
  return S.fetch();
} SWT_API_CATCH

}  // extern "C"
