// swt_batch.hip -- model-ready batches on the device: the CSR pair every encoder ends at (ids, tok_off) as dense, padded,
// fixed-width rows with the attention mask, the row lengths, the row -> sample map and, when given, the spans and word indices
// of the span calls in the same layout; and sentence pairs, [cls] A [sep] B [sep] rows out of two offset arrays into one id
// stream, with token types, the special-tokens mask and sequence ids.  Semantics: include/swt.h; the design and its
// measurements: DESIGN.md 4.9 (single rows) and 4.10 (pairs).
//
// Single rows and pairs are two instantiations of one skeleton, told apart at compile time (SingleLayout, PairLayout): the
// single kernels hold nothing of the pairs, neither a load nor a register (the compiler report of DESIGN.md 4.10).
//
// plan   count_kernel<pair> leaves k(r) in row_base[r] and the longest row (pairs: the largest na + nb) in info[1], one
//        atomicMax per wavefront; pairs also get status[r] and the refused rows in info[3].  launch_scan_bases makes row_base of
//        the counts.
// rows   rows_kernel<Layout>: a group of lanes per SOURCE row (swt_rows.h), a wavefront walking kBtIter sets of rows.  A group
//        walks its row's windows: an output row is found from its source row (row_base[r] + w), never searched for.  A column's
//        content follows from its position p in the row: the layout says whether p is a special or which token it is -- one id
//        load and one map load per token column.  A lane's four columns are one 16-byte store of ids (two with 64-bit ids), one
//        dword of mask, two 16-byte stores of spans; pairs store types as ids are, and special and sequence bytes as one dword
//        each; element by element where the width is no multiple of four or an output is not aligned.  The counters of info are
//        added once per workgroup.  No scratch; no other atomics.
//
// Also here, for every file of the family (declared in swt_batch.h): the scan workspace, launch_scan_bases, launch_counts_sum.
#include "swt_batch.h"

namespace swt {

constexpr int kBtThreads = 256;
constexpr int kBtWaves = kBtThreads / 64;
constexpr uint32_t kBtIter = 4;                // sets of rows one wavefront walks
constexpr uint32_t kBtFlags = SWT_BATCH_WINDOWS | SWT_BATCH_PAD_LEFT | SWT_BATCH_IDS64;

// Output rows of a source row of n tokens in windows of cap tokens that advance by step.
__host__ __device__ inline uint64_t bt_windows(uint64_t n, uint32_t cap, uint32_t step) {
  return n <= cap ? 1 : 1 + (n - cap + step - 1) / step;
}

__device__ inline unsigned long long bt_add_sat(uint64_t a, uint64_t b) { return a + b < a ? ~0ull : a + b; }

constexpr uint32_t kPairWinA = 1, kPairWinB = 2;

// What a pair of na and nb tokens keeps in a row of cap tokens, and how the cut side is windowed.
struct PairCut {
  uint32_t keep_a, keep_b;  // tokens of each side in a row (a window's last may hold fewer of the windowed side)
  uint32_t side, step;      // the windowed side (0: none, kPairWinA, kPairWinB) and the step of its windows
  uint64_t k;               // output rows
  bool fits, refused;
};

__host__ __device__ inline PairCut pair_cut(uint64_t na, uint64_t nb, uint32_t cap, uint32_t stride, bool windows, uint32_t strategy) {
  PairCut c{0, 0, 0, 0, 1, false, false};
  if (na <= cap && nb <= cap - na) {
    c.keep_a = (uint32_t)na; c.keep_b = (uint32_t)nb; c.fits = true;
    return c;
  }
  if (strategy == SWT_PAIR_LONGEST_FIRST) {
    const bool swap = na > nb;
    uint64_t n1 = swap ? nb : na, n2 = n1 > cap ? n1 : (n1 > cap - n1 ? n1 : cap - n1);
    if (n1 > cap || n1 + n2 > cap) { n1 = cap / 2; n2 = n1 + cap % 2; }
    c.keep_a = (uint32_t)(swap ? n2 : n1); c.keep_b = (uint32_t)(swap ? n1 : n2);
    return c;
  }
  const bool first = strategy == SWT_PAIR_ONLY_FIRST;
  const uint64_t kept = first ? nb : na, cut = first ? na : nb;
  if (kept >= cap || (windows && stride >= cap - kept)) { c.refused = true; return c; }
  const uint32_t budget = cap - (uint32_t)kept;  // 1 .. cap, and below the cut side's length: the row does not fit
  c.keep_a = first ? budget : (uint32_t)kept; c.keep_b = first ? (uint32_t)kept : budget;
  if (windows) {
    c.side = first ? kPairWinA : kPairWinB;
    c.step = budget - stride;
    c.k = bt_windows(cut, budget, c.step);
  }
  return c;
}

struct RowsArgs {
  const uint32_t *ids;
  const uint64_t *off_a, *off_b;  // single rows: off_a alone
  uint64_t n_rows;
  const uint32_t *map;
  uint32_t n_map;
  int flagged;
  const uint32_t *spans, *word;
  uint32_t width, cap, stride, step, flags, strategy, pad_id, unk_id, cls_id, sep_id;  // step = cap - stride: of a single row's windows
  const uint64_t *row_base;
  uint64_t rows_cap;
  void *out_ids;
  uint8_t *out_mask;
  void *out_type;  // type, special, seq: pairs only
  uint8_t *out_special;
  int8_t *out_seq;
  uint32_t *out_spans, *out_word, *out_sample, *out_len;
  unsigned long long *info;
  int vec;  // every output takes the wide stores: the width is a multiple of four and the pointers are aligned
  uint32_t group;  // lanes per source row: a power of two, 1 .. 64
};

// ---- what a single row and a pair differ in.  rows_kernel asks its layout per source row (row: the offsets, the token counts;
// then rows() and lost()), per output row (window: its length, and the first token of each side) and per position p < len of
// the row's content (is_cls, is_sep, or token: the index of its token in the stream; pairs: in_b, its type).

struct SingleLayout {  // [cls] tokens [sep], cls and sep each there or not
  static constexpr bool kPair = false;
  uint32_t has_cls, has_sep;
  uint64_t t0, n, k, tok0;
  __device__ explicit SingleLayout(const RowsArgs &A) : has_cls(A.cls_id != SWT_BATCH_NONE), has_sep(A.sep_id != SWT_BATCH_NONE) {}
  __device__ void row(const RowsArgs &A, uint64_t r, bool have, bool windows) {
    t0 = 0; n = 0;
    if (have) n = bt_tokens(A.off_a, r, t0);
    k = windows ? bt_windows(n, A.cap, A.step) : 1;
  }
  __device__ uint64_t rows() const { return k; }
  __device__ bool lost(const RowsArgs &A, bool windows) const { return !windows && n > A.cap; }
  __device__ uint32_t window(const RowsArgs &A, uint64_t w, bool windows) {
    const uint64_t first = windows ? w * A.step : 0;  // the row's first token, < n (or n == 0)
    tok0 = t0 + first - has_cls;                       // token of position p: tok0 + p (wraps back for p >= has_cls)
    return (n - first < (uint64_t)A.cap ? (uint32_t)(n - first) : A.cap) + has_cls + has_sep;
  }
  __device__ bool is_cls(uint32_t p) const { return has_cls && p == 0; }
  __device__ bool is_sep(uint32_t p, uint32_t len) const { return has_sep && p == len - 1; }
  __device__ uint64_t token(uint32_t p) const { return tok0 + p; }
};

struct PairLayout {  // [cls] A [sep] B [sep], all three specials or none; only the windowed side moves with w
  static constexpr bool kPair = true;
  uint32_t sp, pa, pb;  // specials there; the positions of A's and B's first tokens
  uint64_t a0, b0, na, nb, fa, fb;
  PairCut cut;
  __device__ explicit PairLayout(const RowsArgs &A) : sp(A.cls_id != SWT_BATCH_NONE) {}
  __device__ void row(const RowsArgs &A, uint64_t r, bool have, bool windows) {
    a0 = 0; b0 = 0; na = 0; nb = 0;
    if (have) { na = bt_tokens(A.off_a, r, a0); nb = bt_tokens(A.off_b, r, b0); }
    cut = pair_cut(na, nb, A.cap, A.stride, windows, A.strategy);
  }
  __device__ uint64_t rows() const { return cut.k; }
  __device__ bool lost(const RowsArgs &, bool windows) const { return !windows && !cut.fits && !cut.refused; }
  __device__ uint32_t window(const RowsArgs &, uint64_t w, bool) {
    // the window's first token of each side and what it keeps of them: first < n on the windowed side (w < k)
    fa = cut.side == kPairWinA ? w * cut.step : 0; fb = cut.side == kPairWinB ? w * cut.step : 0;
    const uint32_t la = cut.side == kPairWinA && na - fa < (uint64_t)cut.keep_a ? (uint32_t)(na - fa) : cut.keep_a;
    const uint32_t lb = cut.side == kPairWinB && nb - fb < (uint64_t)cut.keep_b ? (uint32_t)(nb - fb) : cut.keep_b;
    pa = sp; pb = la + 2 * sp;
    return cut.refused ? 0 : la + lb + 3 * sp;  // a refused pair: one row of padding
  }
  __device__ bool is_cls(uint32_t p) const { return sp && p == 0; }
  __device__ bool is_sep(uint32_t p, uint32_t len) const { return sp && (p + 1 == pb || p + 1 == len); }
  __device__ uint32_t in_b(uint32_t p) const { return p >= pb; }  // the type of a position: B from its first token on
  __device__ uint64_t token(uint32_t p) const { return in_b(p) ? b0 + fb + (p - pb) : a0 + fa + (p - pa); }
};

__device__ inline void bt_store_spans(uint32_t *out, uint64_t slot, const uint32_t (&a)[kBtQuad], const uint32_t (&b)[kBtQuad]) {
  uint4 *o = reinterpret_cast<uint4 *>(out + 2 * slot);
  o[0] = make_uint4(a[0], b[0], a[1], b[1]);
  o[1] = make_uint4(a[2], b[2], a[3], b[3]);
}

template <class Layout>
__global__ __launch_bounds__(kBtThreads) void rows_kernel(RowsArgs A) {
  constexpr bool kPair = Layout::kPair;
  __shared__ unsigned long long counts[kBtWaves][kPair ? 4 : 2];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t sub = lane & (A.group - 1), per_wave = 64 / A.group;  // lane of its group; rows a wavefront holds at a time
  const bool windows = (A.flags & SWT_BATCH_WINDOWS) != 0, pad_left = (A.flags & SWT_BATCH_PAD_LEFT) != 0;
  const bool ids64 = (A.flags & SWT_BATCH_IDS64) != 0;
  Layout L(A);
  if (blockIdx.x == 0 && threadIdx.x == 0 && A.info) {
    const uint64_t need = A.row_base ? A.row_base[A.n_rows] : A.n_rows;
    A.info[0] = need < A.rows_cap ? need : A.rows_cap;
  }
  const uint64_t r0 = ((uint64_t)blockIdx.x * kBtWaves + wave) * per_wave * kBtIter + lane / A.group;
  uint32_t n_unk = 0, n_lost = 0;
  [[maybe_unused]] uint32_t n_refused = 0;           // pairs only, as longest
  [[maybe_unused]] unsigned long long longest = 0;
  for (uint32_t it = 0; it < kBtIter; it++) {
    const uint64_t r = r0 + (uint64_t)it * per_wave;
    const bool have = r < A.n_rows;
    uint64_t base = A.rows_cap;
    if (have) base = A.row_base ? A.row_base[r] : r;  // ahead of the layout's loads and arithmetic: the loads go out together
    L.row(A, r, have, windows);
    if (have && sub == 0) {
      if constexpr (kPair) {
        const unsigned long long both = bt_add_sat(L.na, L.nb);
        longest = both > longest ? both : longest;
      }
      if (L.lost(A, windows) && base < A.rows_cap) n_lost++;
      if constexpr (kPair) n_refused += L.cut.refused && base < A.rows_cap;
    }
    for (uint64_t w = 0;; w++) {
      const bool live = have && w < L.rows() && base < A.rows_cap && w < A.rows_cap - base;
      if (!__any(live)) break;  // the groups of a wavefront walk their windows together, each as far as its own row goes
      if (!live) continue;
      const uint64_t row = base + w;
      const uint32_t len = L.window(A, w, windows);
      const uint32_t shift = pad_left ? A.width - len : 0;
      const uint64_t slot0 = row * A.width;
      for (uint32_t c0 = sub * kBtQuad; c0 < A.width; c0 += A.group * kBtQuad) {
        uint32_t id[kBtQuad], sa[kBtQuad], sb[kBtQuad], wd[kBtQuad], mask = 0;
        [[maybe_unused]] uint32_t ty[kBtQuad], special = 0x01010101u, seq = 0xFFFFFFFFu;  // pairs only
#pragma unroll
        for (uint32_t j = 0; j < kBtQuad; j++) {
          const uint32_t p = c0 + j - shift;  // position in the row's content; a pad in front wraps to a large value
          id[j] = A.pad_id; sa[j] = 0; sb[j] = 0; wd[j] = SWT_BATCH_NONE;
          if constexpr (kPair) ty[j] = 0;
          if (p >= len) continue;
          mask |= 1u << (8 * j);
          if constexpr (kPair) ty[j] = L.in_b(p);
          if (L.is_cls(p)) { id[j] = A.cls_id; continue; }
          if (L.is_sep(p, len)) { id[j] = A.sep_id; continue; }
          const uint64_t t = L.token(p);
          if constexpr (kPair) {
            special &= ~(1u << (8 * j));
            seq &= ~((ty[j] ? 0xFEu : 0xFFu) << (8 * j));
          }
          id[j] = bt_dense_id(A.ids[t], A.map, A.n_map, A.flagged, A.unk_id, n_unk);
          if (A.spans) { sa[j] = A.spans[2 * t]; sb[j] = A.spans[2 * t + 1]; }
          if (A.word) wd[j] = A.word[t];
        }
        const uint64_t slot = slot0 + c0;
        if (A.vec) {
          bt_store_quad(A.out_ids, slot, ids64, id);
          *reinterpret_cast<uint32_t *>(A.out_mask + slot) = mask;
          if constexpr (kPair) {
            if (A.out_type) bt_store_quad(A.out_type, slot, ids64, ty);
            if (A.out_special) *reinterpret_cast<uint32_t *>(A.out_special + slot) = special;
            if (A.out_seq) *reinterpret_cast<uint32_t *>(A.out_seq + slot) = seq;
          }
          if (A.out_spans) bt_store_spans(A.out_spans, slot, sa, sb);
          if (A.out_word) *reinterpret_cast<uint4 *>(A.out_word + slot) = make_uint4(wd[0], wd[1], wd[2], wd[3]);
        } else {
#pragma unroll
          for (uint32_t j = 0; j < kBtQuad; j++) {
            if (c0 + j >= A.width) break;
            bt_store_one(A.out_ids, slot + j, ids64, id[j]);
            A.out_mask[slot + j] = (uint8_t)((mask >> (8 * j)) & 1u);
            if constexpr (kPair) {
              if (A.out_type) bt_store_one(A.out_type, slot + j, ids64, ty[j]);
              if (A.out_special) A.out_special[slot + j] = (uint8_t)((special >> (8 * j)) & 1u);
              if (A.out_seq) A.out_seq[slot + j] = (int8_t)(uint8_t)(seq >> (8 * j));
            }
            if (A.out_spans) { A.out_spans[2 * (slot + j)] = sa[j]; A.out_spans[2 * (slot + j) + 1] = sb[j]; }
            if (A.out_word) A.out_word[slot + j] = wd[j];
          }
        }
      }
      if (sub == 0) {
        if (A.out_sample) A.out_sample[row] = (uint32_t)r;
        if (A.out_len) A.out_len[row] = len;
      }
    }
  }
  if (!A.info) return;  // uniform over the workgroup
  // info: single rows [1] lost, [2] unknowns; pairs [1] the largest na + nb, [2] unknowns, [3] refused, [4] lost
  // rows_kernel's own fold, the pairs' maximum in the same pass: with bt_fold_counts rows of width 512 measured 1.2 - 1.5 % slower
  // 
  for (int d = 32; d; d >>= 1) {
    n_unk += __shfl_xor(n_unk, d, 64);
    n_lost += __shfl_xor(n_lost, d, 64);
    if constexpr (kPair) {
      n_refused += __shfl_xor(n_refused, d, 64);
      const unsigned long long o = __shfl_xor(longest, d, 64);
      longest = o > longest ? o : longest;
    }
  }
  if (lane == 0) {
    counts[wave][0] = n_lost; counts[wave][1] = n_unk;
    if constexpr (kPair) { counts[wave][2] = n_refused; counts[wave][3] = longest; }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long lost = 0, unk = 0, refused = 0, most = 0;
    for (int v = 0; v < kBtWaves; v++) {
      lost += counts[v][0]; unk += counts[v][1];
      if constexpr (kPair) { refused += counts[v][2]; most = counts[v][3] > most ? counts[v][3] : most; }
    }
    if (lost) atomicAdd(&A.info[kPair ? 4 : 1], lost);
    if (unk) atomicAdd(&A.info[2], unk);
    if constexpr (kPair) {
      if (refused) atomicAdd(&A.info[3], refused);
      if (most) atomicMax(&A.info[1], most);
    }
  }
}

// Plan, first pass: row_base[r] = k(r) with windows (to be scanned), r itself without; info[1] = the longest row, of pairs the
// largest na + nb.  Pairs: status[r], and info[3] = the refused rows.  One atomic each per wavefront that has something to add.
template <bool kPair>
__global__ __launch_bounds__(kBtThreads) void count_kernel(const uint64_t *__restrict__ off_a, const uint64_t *__restrict__ off_b,
                                                           uint64_t n_rows, uint32_t cap, uint32_t stride, int windows, uint32_t strategy,
                                                           unsigned long long *__restrict__ row_base, uint8_t *__restrict__ status,
                                                           unsigned long long *__restrict__ info) {
  const uint64_t i = (uint64_t)blockIdx.x * kBtThreads + threadIdx.x;
  unsigned long long n = 0;
  [[maybe_unused]] uint32_t refused = 0;
  if (i < n_rows) {
    uint64_t first, k;
    n = bt_tokens(off_a, i, first);
    if constexpr (kPair) {
      const uint64_t nb = bt_tokens(off_b, i, first);
      const PairCut cut = pair_cut(n, nb, cap, stride, windows != 0, strategy);
      n = bt_add_sat(n, nb);
      refused = cut.refused;
      k = cut.k;
      status[i] = cut.refused ? SWT_PAIR_REFUSED : SWT_PAIR_OK;
    } else {
      k = windows ? bt_windows(n, cap, cap - stride) : 1;
    }
    row_base[i] = windows ? k : i;
  }
  if (!windows && i == n_rows) {
    row_base[n_rows] = n_rows;
    info[0] = n_rows;
  }
  for (int d = 32; d; d >>= 1) {
    const unsigned long long o = __shfl_xor(n, d, 64);
    n = o > n ? o : n;
    if constexpr (kPair) refused += __shfl_xor(refused, d, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    if (n) atomicMax(&info[1], n);
    if constexpr (kPair) {
      if (refused) atomicAdd(&info[3], (unsigned long long)refused);
    }
  }
}

// A plan's last pass: the group bases on top of the scan inside the groups; the total closes the array.
__global__ __launch_bounds__(kBtThreads) void scan_bases_kernel(const unsigned long long *__restrict__ local,
                                                                const unsigned long long *__restrict__ blk_base, uint64_t n,
                                                                unsigned long long *__restrict__ out,
                                                                const unsigned long long *__restrict__ total) {
  const uint64_t i = (uint64_t)blockIdx.x * kBtThreads + threadIdx.x;
  if (i < n) out[i] = blk_base[i / kBtScanGroup] + local[i];
  else if (i == n) out[n] = *total;
}

// out[k] = the workgroups' counts of counter k = blockIdx.x, summed
__global__ __launch_bounds__(kBtThreads) void counts_sum_kernel(const unsigned long long *__restrict__ part, uint64_t n_blocks,
                                                                uint32_t n_counts, unsigned long long *__restrict__ out) {
  __shared__ unsigned long long waves[kBtWaves][1];
  unsigned long long s[1] = {0};
  for (uint64_t i = threadIdx.x; i < n_blocks; i += kBtThreads) s[0] += part[i * n_counts + blockIdx.x];
  const unsigned long long sum = bt_fold_counts(s, waves);
  if (threadIdx.x == 0) out[blockIdx.x] = sum;
}

BatchWorkspace g_batch_ws;

void launch_scan_bases(uint64_t n, unsigned long long *d_vals, uint64_t *d_total, hipStream_t st) {
  unsigned long long *local = g_batch_ws.local.as<unsigned long long>(), *blk = g_batch_ws.blk.as<unsigned long long>();
  const uint64_t nb = (n + kBtScanGroup - 1) / kBtScanGroup;
  launch_scan_u64(n, d_vals, local, blk, d_total, st);
  hipLaunchKernelGGL(scan_bases_kernel, dim3((unsigned)((n + 1 + kBtThreads - 1) / kBtThreads)), dim3(kBtThreads), 0, st, local, blk + 1 + nb, n,
                     d_vals, reinterpret_cast<const unsigned long long *>(d_total));
}

void launch_counts_sum(const unsigned long long *d_part, uint64_t n_blocks, uint32_t n_counts, unsigned long long *d_out, hipStream_t st) {
  hipLaunchKernelGGL(counts_sum_kernel, dim3(n_counts), dim3(kBtThreads), 0, st, d_part, n_blocks, n_counts, d_out);
}

int BatchWorkspace::reserve(uint64_t n_rows) {
  int rc;
  const uint64_t nb = (n_rows + kBtScanGroup - 1) / kBtScanGroup;
  if ((rc = local.reserve((size_t)n_rows * 8 + 16))) return rc;
  const void *before = blk.p;
  if ((rc = blk.reserve((size_t)(2 * nb + 4) * 8))) return rc;
  if (blk.p != before) {  // a new buffer: zero the scan's ticket once (the scan resets it itself afterwards)
    SWT_HIP(hipMemset(blk.p, 0, 8));
    SWT_HIP(hipDeviceSynchronize());
  }
  return SWT_OK;
}

// The spec of a call.  strategy: null for single rows (cls and sep each count), else the pair's: cls and sep together or not at
// all, three specials with them.  The width is looked at with need_width only; *cap_out = the tokens of a row, 0 without.
static int batch_check_spec(const swt_batch_spec *spec, const uint32_t *strategy, bool need_width, uint32_t *cap_out) {
  if (!spec) return fail(SWT_ERR_INVALID, "null argument");
  if (spec->flags & ~kBtFlags) return fail(SWT_ERR_INVALID, "unknown flag");
  const uint32_t has_cls = spec->cls_id != SWT_BATCH_NONE, has_sep = spec->sep_id != SWT_BATCH_NONE;
  if (strategy) {
    if (has_cls != has_sep) return fail(SWT_ERR_INVALID, "a pair row has cls_id and sep_id or neither");
    if (*strategy > SWT_PAIR_ONLY_SECOND) return fail(SWT_ERR_INVALID, "unknown truncation strategy");
    if (*strategy == SWT_PAIR_LONGEST_FIRST && (spec->flags & SWT_BATCH_WINDOWS))
      return fail(SWT_ERR_INVALID, "longest_first has no windows: take only_first or only_second");
  }
  *cap_out = 0;
  if (!need_width) return SWT_OK;
  const uint32_t n_special = strategy ? 3 * has_cls : has_cls + has_sep;
  if (spec->width <= n_special) return fail(SWT_ERR_INVALID, "the width leaves no room for a token");
  const uint32_t cap = spec->width - n_special;
  if (spec->stride >= cap) return fail(SWT_ERR_INVALID, "the stride must be smaller than the tokens of a row");
  if (spec->pad_id == SWT_BATCH_NONE || spec->unk_id == SWT_BATCH_NONE) return fail(SWT_ERR_INVALID, "pad_id and unk_id must be ids");
  *cap_out = cap;
  return SWT_OK;
}

// What a rows call may not be without, device or host pointers alike.
static int batch_check_rows(const uint32_t *map, int flagged, const uint32_t *spans, const uint32_t *word, const swt_batch_spec *spec,
                            const uint64_t *row_base, uint64_t n_rows, const void *out_ids, const uint8_t *out_mask,
                            const uint32_t *out_spans, const uint32_t *out_word) {
  if (!out_ids || !out_mask) return fail(SWT_ERR_INVALID, "null argument");
  if (flagged && !map) return fail(SWT_ERR_INVALID, "a flagged stream needs a map");
  if ((spans != nullptr) != (out_spans != nullptr) || (word != nullptr) != (out_word != nullptr))
    return fail(SWT_ERR_INVALID, "a payload and its output are given together");
  if ((spec->flags & SWT_BATCH_WINDOWS) && !row_base) return fail(SWT_ERR_INVALID, "windows need row_base");
  if (n_rows > 0xFFFFFFFFull) return fail(SWT_ERR_INVALID, "2^32 rows or more");
  return SWT_OK;
}

// The plan of both kinds on device pointers, the spec checked: info cleared (16 bytes; 40 for pairs), count, scan, bases.
template <bool kPair>
static int batch_plan_launch(const uint64_t *d_off_a, const uint64_t *d_off_b, uint64_t n_rows, const swt_batch_spec *spec, uint32_t cap,
                             uint32_t strategy, uint64_t *d_row_base, uint8_t *d_status, uint64_t *d_info, void *stream) {
  int rc = ensure_device();
  if (rc) return rc;
  const bool windows = (spec->flags & SWT_BATCH_WINDOWS) != 0;
  hipStream_t st = (hipStream_t)stream;
  unsigned long long *rb = reinterpret_cast<unsigned long long *>(d_row_base), *info = reinterpret_cast<unsigned long long *>(d_info);
  if (windows && n_rows && (rc = g_batch_ws.reserve(n_rows))) return rc;
  SWT_HIP(hipMemsetAsync(d_info, 0, kPair ? 40 : 16, st));
  if (!n_rows) {
    SWT_HIP(hipMemsetAsync(d_row_base, 0, 8, st));
    return SWT_OK;
  }
  const unsigned grid = (unsigned)((n_rows + 1 + kBtThreads - 1) / kBtThreads);
  hipLaunchKernelGGL(count_kernel<kPair>, dim3(grid), dim3(kBtThreads), 0, st, d_off_a, d_off_b, n_rows, cap, spec->stride, windows ? 1 : 0,
                     strategy, rb, d_status, info);
  if (windows) launch_scan_bases(n_rows, rb, d_info, st);
  SWT_HIP(hipGetLastError());
  return SWT_OK;
}

// The rows of both kinds on device pointers, the arguments checked: the alignment of the outputs, info cleared (24 bytes; 40 for
// pairs), the wide stores or not, the lanes of a row, the launch.
template <class Layout>
static int batch_rows_launch(RowsArgs A, void *stream) {
  const uintptr_t id_bytes = (A.flags & SWT_BATCH_IDS64) ? 8 : 4;
  if (!bt_aligned(id_bytes, {A.out_ids, A.out_type}) || !bt_aligned(4, {A.out_spans, A.out_word, A.out_sample, A.out_len}) ||
      !bt_aligned(8, {A.info}))
    return fail(SWT_ERR_INVALID, "an output is not aligned to its element type");
  int rc = ensure_device();
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (A.info) SWT_HIP(hipMemsetAsync(A.info, 0, Layout::kPair ? 40 : 24, st));
  if (!A.n_rows || !A.rows_cap) return SWT_OK;
  A.vec = A.width % kBtQuad == 0 && bt_aligned(16, {A.out_ids, A.out_type, A.out_spans, A.out_word}) &&
          bt_aligned(4, {A.out_mask, A.out_special, A.out_seq});
  A.group = bt_group(A.width);
  const uint64_t per_block = (uint64_t)kBtWaves * (64 / A.group) * kBtIter;  // source rows of a workgroup
  prof_begin(st);
  hipLaunchKernelGGL(rows_kernel<Layout>, dim3((unsigned)((A.n_rows + per_block - 1) / per_block)), dim3(kBtThreads), 0, st, A);
  prof_end(st);
  SWT_HIP(hipGetLastError());
  return SWT_OK;
}

}  // namespace swt

using namespace swt;

extern "C" {

int swt_batch_capacity(uint32_t *cols_per_step, uint32_t *scan_group) try {
  if (cols_per_step) *cols_per_step = kBtCols;
  if (scan_group) *scan_group = kBtScanGroup;
  return SWT_OK;
} SWT_API_CATCH

int swt_batch_plan_dev(const uint64_t *d_tok_off, uint64_t n_rows, const swt_batch_spec *spec, uint64_t *d_row_base, uint64_t *d_info,
                       void *stream) try {
  uint32_t cap = 0;
  int rc = batch_check_spec(spec, nullptr, spec && (spec->flags & SWT_BATCH_WINDOWS), &cap);  // without windows the width is not looked at
  if (rc) return rc;
  if (!d_tok_off || !d_row_base || !d_info) return fail(SWT_ERR_INVALID, "null argument");
  return batch_plan_launch<false>(d_tok_off, nullptr, n_rows, spec, cap, 0, d_row_base, nullptr, d_info, stream);
} SWT_API_CATCH

int swt_batch_plan(const uint64_t *tok_off, uint64_t n_rows, const swt_batch_spec *spec, uint64_t *row_base, uint64_t *info) try {
  uint32_t cap = 0;
  int rc = batch_check_spec(spec, nullptr, spec && (spec->flags & SWT_BATCH_WINDOWS), &cap);
  if (rc) return rc;
  if (!tok_off || !row_base || !info) return fail(SWT_ERR_INVALID, "null argument");
  for (uint64_t r = 0; r < n_rows; r++)
    if (tok_off[r] > tok_off[r + 1]) return fail(SWT_ERR_INVALID, "offsets must not decrease");
  if ((rc = ensure_device())) return rc;
  BatchStage s;
  const size_t off_bytes = (size_t)(n_rows + 1) * 8;
  const uint64_t *d_off = s.in(tok_off, off_bytes);
  uint64_t *d_base = s.out(row_base, off_bytes), *d_info = s.out(info, 16);
  if (s.rc) return s.rc;
  if ((rc = swt_batch_plan_dev(d_off, n_rows, spec, d_base, d_info, nullptr))) return rc;
  return s.fetch();
} SWT_API_CATCH

int swt_batch_rows_dev(const uint32_t *d_ids, const uint64_t *d_tok_off, uint64_t n_rows, const uint32_t *d_map, uint32_t n_map, int flagged,
                       const uint32_t *d_spans, const uint32_t *d_word, const swt_batch_spec *spec, const uint64_t *d_row_base,
                       uint64_t rows_cap, void *d_out_ids, uint8_t *d_out_mask, uint32_t *d_out_spans, uint32_t *d_out_word,
                       uint32_t *d_out_sample, uint32_t *d_out_len, uint64_t *d_info, void *stream) try {
  uint32_t cap = 0;
  int rc = batch_check_spec(spec, nullptr, true, &cap);
  if (rc) return rc;
  if ((rc = batch_check_rows(d_map, flagged, d_spans, d_word, spec, d_row_base, n_rows, d_out_ids, d_out_mask, d_out_spans, d_out_word)))
    return rc;
  if (n_rows && (!d_tok_off || !d_ids)) return fail(SWT_ERR_INVALID, "null argument");
  return batch_rows_launch<SingleLayout>(
      {d_ids, d_tok_off, nullptr, n_rows, d_map, n_map, flagged ? 1 : 0, d_spans, d_word, spec->width, cap, spec->stride, cap - spec->stride,
       spec->flags, 0, spec->pad_id, spec->unk_id, spec->cls_id, spec->sep_id, d_row_base, rows_cap, d_out_ids, d_out_mask, nullptr, nullptr,
       nullptr, d_out_spans, d_out_word, d_out_sample, d_out_len, reinterpret_cast<unsigned long long *>(d_info), 0, 1},
      stream);
} SWT_API_CATCH

int swt_batch_rows(const uint32_t *ids, const uint64_t *tok_off, uint64_t n_rows, const uint32_t *map, uint32_t n_map, int flagged,
                   const uint32_t *spans, const uint32_t *word, const swt_batch_spec *spec, const uint64_t *row_base, uint64_t rows_cap,
                   void *out_ids, uint8_t *out_mask, uint32_t *out_spans, uint32_t *out_word, uint32_t *out_sample, uint32_t *out_len,
                   uint64_t *info) try {
  uint32_t cap = 0;
  int rc = batch_check_spec(spec, nullptr, true, &cap);
  if (rc) return rc;
  if ((rc = batch_check_rows(map, flagged, spans, word, spec, row_base, n_rows, out_ids, out_mask, out_spans, out_word))) return rc;
  if (n_rows && !tok_off) return fail(SWT_ERR_INVALID, "null argument");
  const bool windows = (spec->flags & SWT_BATCH_WINDOWS) != 0;
  uint64_t need = 0;
  for (uint64_t r = 0; r < n_rows; r++) {
    if (tok_off[r] > tok_off[r + 1]) return fail(SWT_ERR_INVALID, "offsets must not decrease");
    if (row_base && row_base[r] != need) return fail(SWT_ERR_INVALID, "row_base is not the plan of these offsets");
    need += windows ? bt_windows(tok_off[r + 1] - tok_off[r], cap, cap - spec->stride) : 1;
  }
  if (n_rows && row_base && row_base[n_rows] != need) return fail(SWT_ERR_INVALID, "row_base is not the plan of these offsets");
  const uint64_t n_tok = n_rows ? tok_off[n_rows] : 0;
  if (n_tok && !ids) return fail(SWT_ERR_INVALID, "null argument");
  if (info) { info[0] = need; info[1] = 0; info[2] = 0; }
  if (need > rows_cap) return fail(SWT_ERR_CAPACITY, "%llu rows needed, room for %llu", (unsigned long long)need, (unsigned long long)rows_cap);
  if (!n_rows) return SWT_OK;
  if ((rc = ensure_device())) return rc;
  const size_t slots = (size_t)need * spec->width, n_map_all = map ? (size_t)n_map * (flagged ? 2 : 1) : 0;
  const size_t id_bytes = (spec->flags & SWT_BATCH_IDS64) ? 8 : 4, off_bytes = (size_t)(n_rows + 1) * 8;
  BatchStage s;
  const uint32_t *d_ids = s.in(ids, n_tok * 4, true), *d_map = s.in(map, n_map_all * 4);
  const uint32_t *d_spans = s.in(spans, n_tok * 8), *d_word = s.in(word, n_tok * 4);
  const uint64_t *d_off = s.in(tok_off, off_bytes), *d_base = s.in(row_base, off_bytes);
  void *d_out = s.out(out_ids, slots * id_bytes);
  uint8_t *d_mask = s.out(out_mask, slots);
  uint32_t *d_out_spans = s.out(out_spans, slots * 8), *d_out_word = s.out(out_word, slots * 4);
  uint32_t *d_sample = s.out(out_sample, (size_t)need * 4), *d_len = s.out(out_len, (size_t)need * 4);
  uint64_t *d_info = s.out(info, 24);
  if (s.rc) return s.rc;
  if ((rc = swt_batch_rows_dev(d_ids, d_off, n_rows, d_map, n_map, flagged, d_spans, d_word, spec, d_base, need, d_out, d_mask, d_out_spans,
                               d_out_word, d_sample, d_len, d_info, nullptr)))
    return rc;
  return s.fetch();
} SWT_API_CATCH

int swt_batch_pair_capacity(uint32_t *cols_per_step, uint32_t *scan_group) try {
  return swt_batch_capacity(cols_per_step, scan_group);  // the pair kernels are the skeleton and the scan of the single ones
} SWT_API_CATCH

int swt_batch_pair_plan_dev(const uint64_t *d_off_a, const uint64_t *d_off_b, uint64_t n_rows, const swt_batch_spec *spec, uint32_t strategy,
                            uint64_t *d_row_base, uint8_t *d_status, uint64_t *d_info, void *stream) try {
  uint32_t cap = 0;
  const bool sized = spec && spec->width != 0;  // a zero width: only the largest pair is asked for, every row counts as fitting
  int rc = batch_check_spec(spec, &strategy, sized || (spec && (spec->flags & SWT_BATCH_WINDOWS)), &cap);
  if (rc) return rc;
  if (!d_off_a || !d_off_b || !d_row_base || !d_status || !d_info) return fail(SWT_ERR_INVALID, "null argument");
  if (n_rows > 0xFFFFFFFFull) return fail(SWT_ERR_INVALID, "2^32 rows or more");
  return batch_plan_launch<true>(d_off_a, d_off_b, n_rows, spec, sized ? cap : 0xFFFFFFFFu, strategy, d_row_base, d_status, d_info, stream);
} SWT_API_CATCH

int swt_batch_pair_plan(const uint64_t *off_a, const uint64_t *off_b, uint64_t n_rows, const swt_batch_spec *spec, uint32_t strategy,
                        uint64_t *row_base, uint8_t *status, uint64_t *info) try {
  uint32_t cap = 0;
  int rc = batch_check_spec(spec, &strategy, spec && ((spec->flags & SWT_BATCH_WINDOWS) || spec->width != 0), &cap);
  if (rc) return rc;
  if (!off_a || !off_b || !row_base || !status || !info) return fail(SWT_ERR_INVALID, "null argument");
  for (uint64_t r = 0; r < n_rows; r++)
    if (off_a[r] > off_a[r + 1] || off_b[r] > off_b[r + 1]) return fail(SWT_ERR_INVALID, "offsets must not decrease");
  if ((rc = ensure_device())) return rc;
  BatchStage s;
  const size_t off_bytes = (size_t)(n_rows + 1) * 8;
  const uint64_t *d_a = s.in(off_a, off_bytes), *d_b = s.in(off_b, off_bytes);
  uint64_t *d_base = s.out(row_base, off_bytes), *d_info = s.out(info, 40);
  uint8_t *d_status = s.out(status, (size_t)n_rows);
  if (s.rc) return s.rc;
  if ((rc = swt_batch_pair_plan_dev(d_a, d_b, n_rows, spec, strategy, d_base, d_status, d_info, nullptr))) return rc;
  return s.fetch();
} SWT_API_CATCH

int swt_batch_pair_rows_dev(const uint32_t *d_ids, const uint64_t *d_off_a, const uint64_t *d_off_b, uint64_t n_rows, const uint32_t *d_map,
                            uint32_t n_map, int flagged, const uint32_t *d_spans, const uint32_t *d_word, const swt_batch_spec *spec,
                            uint32_t strategy, const uint64_t *d_row_base, const uint8_t *d_status, uint64_t rows_cap, void *d_out_ids,
                            uint8_t *d_out_mask, void *d_out_type, uint8_t *d_out_special, int8_t *d_out_seq, uint32_t *d_out_spans,
                            uint32_t *d_out_word, uint32_t *d_out_sample, uint32_t *d_out_len, uint64_t *d_info, void *stream) try {
  uint32_t cap = 0;
  int rc = batch_check_spec(spec, &strategy, true, &cap);
  if (rc) return rc;
  if ((rc = batch_check_rows(d_map, flagged, d_spans, d_word, spec, d_row_base, n_rows, d_out_ids, d_out_mask, d_out_spans, d_out_word)))
    return rc;
  if (n_rows && (!d_off_a || !d_off_b || !d_ids)) return fail(SWT_ERR_INVALID, "null argument");
  (void)d_status;  // the kernel takes every row's cut from its offsets, as it takes the window counts: nothing a caller hands in steers a store
  return batch_rows_launch<PairLayout>(
      {d_ids, d_off_a, d_off_b, n_rows, d_map, n_map, flagged ? 1 : 0, d_spans, d_word, spec->width, cap, spec->stride, cap - spec->stride,
       spec->flags, strategy, spec->pad_id, spec->unk_id, spec->cls_id, spec->sep_id, d_row_base, rows_cap, d_out_ids, d_out_mask, d_out_type,
       d_out_special, d_out_seq, d_out_spans, d_out_word, d_out_sample, d_out_len, reinterpret_cast<unsigned long long *>(d_info), 0, 1},
      stream);
} SWT_API_CATCH

int swt_batch_pair_rows(const uint32_t *ids, const uint64_t *off_a, const uint64_t *off_b, uint64_t n_rows, const uint32_t *map, uint32_t n_map,
                        int flagged, const uint32_t *spans, const uint32_t *word, const swt_batch_spec *spec, uint32_t strategy,
                        const uint64_t *row_base, const uint8_t *status, uint64_t rows_cap, void *out_ids, uint8_t *out_mask, void *out_type,
                        uint8_t *out_special, int8_t *out_seq, uint32_t *out_spans, uint32_t *out_word, uint32_t *out_sample, uint32_t *out_len,
                        uint64_t *info) try {
  uint32_t cap = 0;
  int rc = batch_check_spec(spec, &strategy, true, &cap);
  if (rc) return rc;
  if ((rc = batch_check_rows(map, flagged, spans, word, spec, row_base, n_rows, out_ids, out_mask, out_spans, out_word))) return rc;
  if (n_rows && (!off_a || !off_b)) return fail(SWT_ERR_INVALID, "null argument");
  const bool windows = (spec->flags & SWT_BATCH_WINDOWS) != 0;
  uint64_t need = 0, n_tok = 0;
  for (uint64_t r = 0; r < n_rows; r++) {
    if (off_a[r] > off_a[r + 1] || off_b[r] > off_b[r + 1]) return fail(SWT_ERR_INVALID, "offsets must not decrease");
    if (row_base && row_base[r] != need) return fail(SWT_ERR_INVALID, "row_base is not the plan of these offsets");
    const PairCut cut = pair_cut(off_a[r + 1] - off_a[r], off_b[r + 1] - off_b[r], cap, spec->stride, windows, strategy);
    if (status && status[r] != (cut.refused ? SWT_PAIR_REFUSED : SWT_PAIR_OK)) return fail(SWT_ERR_INVALID, "status is not the plan of these offsets");
    need += cut.k;
  }
  if (n_rows && row_base && row_base[n_rows] != need) return fail(SWT_ERR_INVALID, "row_base is not the plan of these offsets");
  if (n_rows) n_tok = off_a[n_rows] > off_b[n_rows] ? off_a[n_rows] : off_b[n_rows];  // the stream reaches as far as either side does
  if (n_tok && !ids) return fail(SWT_ERR_INVALID, "null argument");
  if (info) { info[0] = need; info[1] = info[2] = info[3] = info[4] = 0; }
  if (need > rows_cap) return fail(SWT_ERR_CAPACITY, "%llu rows needed, room for %llu", (unsigned long long)need, (unsigned long long)rows_cap);
  if (!n_rows) return SWT_OK;
  if ((rc = ensure_device())) return rc;
  const size_t slots = (size_t)need * spec->width, n_map_all = map ? (size_t)n_map * (flagged ? 2 : 1) : 0;
  const size_t id_bytes = (spec->flags & SWT_BATCH_IDS64) ? 8 : 4, off_bytes = (size_t)(n_rows + 1) * 8;
  BatchStage s;
  const uint32_t *d_ids = s.in(ids, n_tok * 4, true), *d_map = s.in(map, n_map_all * 4);
  const uint32_t *d_spans = s.in(spans, n_tok * 8), *d_word = s.in(word, n_tok * 4);
  const uint64_t *d_a = s.in(off_a, off_bytes), *d_b = s.in(off_b, off_bytes), *d_base = s.in(row_base, off_bytes);
  void *d_out = s.out(out_ids, slots * id_bytes), *d_type = s.out(out_type, slots * id_bytes);
  uint8_t *d_mask = s.out(out_mask, slots), *d_special = s.out(out_special, slots);
  int8_t *d_seq = s.out(out_seq, slots);
  uint32_t *d_out_spans = s.out(out_spans, slots * 8), *d_out_word = s.out(out_word, slots * 4);
  uint32_t *d_sample = s.out(out_sample, (size_t)need * 4), *d_len = s.out(out_len, (size_t)need * 4);
  uint64_t *d_info = s.out(info, 40);
  if (s.rc) return s.rc;
  if ((rc = swt_batch_pair_rows_dev(d_ids, d_a, d_b, n_rows, d_map, n_map, flagged, d_spans, d_word, spec, strategy, d_base, nullptr, need, d_out,
                                    d_mask, d_type, d_special, d_seq, d_out_spans, d_out_word, d_sample, d_len, d_info, nullptr)))
    return rc;
  return s.fetch();
} SWT_API_CATCH

}  // extern "C"
