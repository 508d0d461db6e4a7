// swt_batch.hip -- model-ready batches on the device: the CSR pair every encoder ends at (ids, tok_off) as dense, padded,
// fixed-width rows with the attention mask, the row lengths, the row -> sample map and, when given, the spans and word indices
// of the span calls in the same layout.  Semantics: include/swt.h; the design and its measurements: DESIGN.md 4.9.
//
// plan   batch_count_kernel leaves k(r) in row_base[r] (and the longest row in info[1], one atomicMax per wavefront),
//        launch_scan_u64 (swt_tile.h) scans it in groups of kBtScanGroup, batch_base_kernel adds the group bases.
// rows   batch_rows_kernel: a group of g lanes per SOURCE row, g the power of two that covers the width at four columns a lane,
//        so a wavefront holds 64 / g rows at a time and walks kBtIter such sets.  A group walks its row's windows: an output row
//        is found from its source row (row_base[r] + w), never searched for.  A lane's four columns are one 16-byte store of
//        ids (two with 64-bit ids), one dword of mask, two 16-byte stores of spans; element by element where the width is no
//        multiple of four or an output is not aligned.  The counters of info are summed over the wavefront, then the workgroup
//        (64 bytes of LDS), and added once per workgroup.  No scratch; no other atomics.
#include "swt_tile.h"

namespace swt {

constexpr int kBtThreads = 256;
constexpr int kBtWaves = kBtThreads / 64;
constexpr uint32_t kBtQuad = 4;                // columns of one lane per step
constexpr uint32_t kBtCols = 64 * kBtQuad;     // columns of one wavefront per step
constexpr uint32_t kBtIter = 4;                // sets of rows one wavefront walks
constexpr uint32_t kBtScanGroup = 1024;        // rows of one scan group (launch_scan_u64)
constexpr uint32_t kBtFlags = SWT_BATCH_WINDOWS | SWT_BATCH_PAD_LEFT | SWT_BATCH_IDS64;

// Output rows of a source row of n tokens in windows of cap tokens that advance by step.
__host__ __device__ inline uint64_t bt_windows(uint64_t n, uint32_t cap, uint32_t step) {
  return n <= cap ? 1 : 1 + (n - cap + step - 1) / step;
}

struct BatchArgs {
  const uint32_t *ids;
  const uint64_t *tok_off;
  uint64_t n_rows;
  const uint32_t *map;
  uint32_t n_map;
  int flagged;
  const uint32_t *spans, *word;
  uint32_t width, cap, step, flags, pad_id, unk_id, cls_id, sep_id;
  const uint64_t *row_base;
  uint64_t rows_cap;
  void *out_ids;
  uint8_t *out_mask;
  uint32_t *out_spans, *out_word, *out_sample, *out_len;
  unsigned long long *info;
  int vec;  // every output takes the wide stores: the width is a multiple of four and the pointers are aligned
  uint32_t group;  // lanes per source row: a power of two, 1 .. 64
};

__global__ __launch_bounds__(kBtThreads) void batch_rows_kernel(BatchArgs A) {
  __shared__ unsigned long long counts[kBtWaves][2];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t sub = lane & (A.group - 1), per_wave = 64 / A.group;  // lane of its group; rows a wavefront holds at a time
  const bool windows = (A.flags & SWT_BATCH_WINDOWS) != 0, pad_left = (A.flags & SWT_BATCH_PAD_LEFT) != 0;
  const bool ids64 = (A.flags & SWT_BATCH_IDS64) != 0;
  const uint32_t has_cls = A.cls_id != SWT_BATCH_NONE, has_sep = A.sep_id != SWT_BATCH_NONE;
  if (blockIdx.x == 0 && threadIdx.x == 0 && A.info) {
    const uint64_t need = A.row_base ? A.row_base[A.n_rows] : A.n_rows;
    A.info[0] = need < A.rows_cap ? need : A.rows_cap;
  }
  const uint64_t r0 = ((uint64_t)blockIdx.x * kBtWaves + wave) * per_wave * kBtIter + lane / A.group;
  uint32_t n_unk = 0, n_lost = 0;
  for (uint32_t it = 0; it < kBtIter; it++) {
    const uint64_t r = r0 + (uint64_t)it * per_wave;
    const bool have = r < A.n_rows;
    uint64_t t0 = 0, n = 0, base = A.rows_cap;
    if (have) {
      t0 = A.tok_off[r];
      const uint64_t t1 = A.tok_off[r + 1];
      n = t1 > t0 ? t1 - t0 : 0;
      base = A.row_base ? A.row_base[r] : r;
    }
    const uint64_t k = windows ? bt_windows(n, A.cap, A.step) : 1;
    if (have && sub == 0 && !windows && n > A.cap && base < A.rows_cap) n_lost++;
    for (uint64_t w = 0;; w++) {
      const bool live = have && w < k && base < A.rows_cap && w < A.rows_cap - base;
      if (!__any(live)) break;  // the groups of a wavefront walk their windows together, each as far as its own row goes
      if (!live) continue;
      const uint64_t row = base + w;
      const uint64_t first = windows ? w * A.step : 0;  // the row's first token, < n (or n == 0)
      const uint32_t body = n - first < (uint64_t)A.cap ? (uint32_t)(n - first) : A.cap;
      const uint32_t len = body + has_cls + has_sep;
      const uint32_t shift = pad_left ? A.width - len : 0;
      const uint64_t slot0 = row * A.width;
      const uint64_t tok0 = t0 + first - has_cls;  // token of position p: tok0 + p (wraps back for p >= has_cls)
      for (uint32_t c0 = sub * kBtQuad; c0 < A.width; c0 += A.group * kBtQuad) {
        uint32_t id[kBtQuad], sa[kBtQuad], sb[kBtQuad], wd[kBtQuad], mask = 0;
#pragma unroll
        for (uint32_t j = 0; j < kBtQuad; j++) {
          const uint32_t p = c0 + j - shift;  // position in the row's content; a pad in front wraps to a large value
          id[j] = A.pad_id; sa[j] = 0; sb[j] = 0; wd[j] = SWT_BATCH_NONE;
          if (p >= len) continue;
          mask |= 1u << (8 * j);
          if (has_cls && p == 0) { id[j] = A.cls_id; continue; }
          if (has_sep && p == len - 1) { id[j] = A.sep_id; continue; }
          const uint64_t t = tok0 + p;
          const uint32_t raw = A.ids[t], s = raw & 0x7FFFFFFFu;
          uint32_t d = SWT_BATCH_NONE;
          if (s < A.n_map) d = A.map ? A.map[(uint64_t)s + ((A.flagged && (raw >> 31)) ? (uint64_t)A.n_map : 0ull)] : s;
          if (d == SWT_BATCH_NONE) { d = A.unk_id; n_unk++; }
          id[j] = d;
          if (A.spans) { sa[j] = A.spans[2 * t]; sb[j] = A.spans[2 * t + 1]; }
          if (A.word) wd[j] = A.word[t];
        }
        const uint64_t slot = slot0 + c0;
        if (A.vec) {
          if (ids64) {
            uint4 *o = reinterpret_cast<uint4 *>(reinterpret_cast<uint64_t *>(A.out_ids) + slot);
            o[0] = make_uint4(id[0], 0, id[1], 0);
            o[1] = make_uint4(id[2], 0, id[3], 0);
          } else {
            *reinterpret_cast<uint4 *>(reinterpret_cast<uint32_t *>(A.out_ids) + slot) = make_uint4(id[0], id[1], id[2], id[3]);
          }
          *reinterpret_cast<uint32_t *>(A.out_mask + slot) = mask;
          if (A.out_spans) {
            uint4 *o = reinterpret_cast<uint4 *>(A.out_spans + 2 * slot);
            o[0] = make_uint4(sa[0], sb[0], sa[1], sb[1]);
            o[1] = make_uint4(sa[2], sb[2], sa[3], sb[3]);
          }
          if (A.out_word) *reinterpret_cast<uint4 *>(A.out_word + slot) = make_uint4(wd[0], wd[1], wd[2], wd[3]);
        } else {
#pragma unroll
          for (uint32_t j = 0; j < kBtQuad; j++) {
            if (c0 + j >= A.width) break;
            if (ids64) reinterpret_cast<uint64_t *>(A.out_ids)[slot + j] = id[j];
            else reinterpret_cast<uint32_t *>(A.out_ids)[slot + j] = id[j];
            A.out_mask[slot + j] = (uint8_t)((mask >> (8 * j)) & 1u);
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
  for (int d = 32; d; d >>= 1) {
    n_unk += __shfl_xor(n_unk, d, 64);
    n_lost += __shfl_xor(n_lost, d, 64);
  }
  if (lane == 0) { counts[wave][0] = n_lost; counts[wave][1] = n_unk; }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long lost = 0, unk = 0;
    for (int v = 0; v < kBtWaves; v++) { lost += counts[v][0]; unk += counts[v][1]; }
    if (lost) atomicAdd(&A.info[1], lost);
    if (unk) atomicAdd(&A.info[2], unk);
  }
}

// Plan, first pass: row_base[r] = k(r) with windows (to be scanned), r itself without; info[1] = the longest row.
__global__ __launch_bounds__(kBtThreads) void batch_count_kernel(const uint64_t *__restrict__ tok_off, uint64_t n_rows, uint32_t cap,
                                                                 uint32_t step, int windows, unsigned long long *__restrict__ row_base,
                                                                 unsigned long long *__restrict__ info) {
  const uint64_t i = (uint64_t)blockIdx.x * kBtThreads + threadIdx.x;
  unsigned long long n = 0;
  if (i < n_rows) {
    const uint64_t t0 = tok_off[i], t1 = tok_off[i + 1];
    n = t1 > t0 ? t1 - t0 : 0;
    row_base[i] = windows ? bt_windows(n, cap, step) : i;
  }
  if (!windows && i == n_rows) {
    row_base[n_rows] = n_rows;
    info[0] = n_rows;
  }
  for (int d = 32; d; d >>= 1) {
    const unsigned long long o = __shfl_xor(n, d, 64);
    n = o > n ? o : n;
  }
  if ((threadIdx.x & 63) == 0 && n) atomicMax(&info[1], n);
}

// Plan, last pass: the group bases on top of the scan inside the groups; the total closes the array.
__global__ __launch_bounds__(kBtThreads) void batch_base_kernel(const unsigned long long *__restrict__ local,
                                                                const unsigned long long *__restrict__ blk_base, uint64_t n_rows,
                                                                unsigned long long *__restrict__ row_base,
                                                                const unsigned long long *__restrict__ info) {
  const uint64_t i = (uint64_t)blockIdx.x * kBtThreads + threadIdx.x;
  if (i < n_rows) row_base[i] = blk_base[i / kBtScanGroup] + local[i];
  else if (i == n_rows) row_base[n_rows] = info[0];
}

// ---- sentence pairs: [cls] A [sep] B [sep] rows out of two offset arrays into one id stream (include/swt.h)
//
// plan   pair_count_kernel: k(r) into row_base[r], status[r], the largest na + nb and the refused rows folded per wavefront;
//        then the scan and batch_base_kernel of the single-sequence plan, in the same workspace.
// rows   pair_rows_kernel: the skeleton of batch_rows_kernel.  A column's content follows from its position p in the row against
//        the window's kept lengths la and lb: cls, a token of A, sep, a token of B, sep, padding -- one id load and one map load
//        per token column.  Only the windowed side moves with w.  Types are stored as ids are; mask, special and sequence
//        bytes are one dword per lane each.

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

struct PairArgs {
  const uint32_t *ids;
  const uint64_t *off_a, *off_b;
  uint64_t n_rows;
  const uint32_t *map;
  uint32_t n_map;
  int flagged;
  const uint32_t *spans, *word;
  uint32_t width, cap, stride, flags, strategy, pad_id, unk_id, cls_id, sep_id;
  const uint64_t *row_base;
  uint64_t rows_cap;
  void *out_ids;
  uint8_t *out_mask;
  void *out_type;
  uint8_t *out_special;
  int8_t *out_seq;
  uint32_t *out_spans, *out_word, *out_sample, *out_len;
  unsigned long long *info;
  int vec;
  uint32_t group;
};

// four elements of an id-typed output: one 16-byte store, two with 64-bit ids
__device__ inline void bt_store_quad(void *out, uint64_t slot, bool ids64, const uint32_t (&v)[kBtQuad]) {
  if (ids64) {
    uint4 *o = reinterpret_cast<uint4 *>(reinterpret_cast<uint64_t *>(out) + slot);
    o[0] = make_uint4(v[0], 0, v[1], 0);
    o[1] = make_uint4(v[2], 0, v[3], 0);
  } else {
    *reinterpret_cast<uint4 *>(reinterpret_cast<uint32_t *>(out) + slot) = make_uint4(v[0], v[1], v[2], v[3]);
  }
}

__global__ __launch_bounds__(kBtThreads) void pair_rows_kernel(PairArgs A) {
  __shared__ unsigned long long counts[kBtWaves][4];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t sub = lane & (A.group - 1), per_wave = 64 / A.group;
  const bool windows = (A.flags & SWT_BATCH_WINDOWS) != 0, pad_left = (A.flags & SWT_BATCH_PAD_LEFT) != 0;
  const bool ids64 = (A.flags & SWT_BATCH_IDS64) != 0;
  const uint32_t sp = A.cls_id != SWT_BATCH_NONE;  // cls and both sep, or none of them
  if (blockIdx.x == 0 && threadIdx.x == 0 && A.info) {
    const uint64_t need = A.row_base ? A.row_base[A.n_rows] : A.n_rows;
    A.info[0] = need < A.rows_cap ? need : A.rows_cap;
  }
  const uint64_t r0 = ((uint64_t)blockIdx.x * kBtWaves + wave) * per_wave * kBtIter + lane / A.group;
  uint32_t n_unk = 0, n_lost = 0, n_refused = 0;
  unsigned long long longest = 0;
  for (uint32_t it = 0; it < kBtIter; it++) {
    const uint64_t r = r0 + (uint64_t)it * per_wave;
    const bool have = r < A.n_rows;
    uint64_t a0 = 0, b0 = 0, na = 0, nb = 0, base = A.rows_cap;
    if (have) {
      a0 = A.off_a[r]; b0 = A.off_b[r];
      const uint64_t a1 = A.off_a[r + 1], b1 = A.off_b[r + 1];
      na = a1 > a0 ? a1 - a0 : 0; nb = b1 > b0 ? b1 - b0 : 0;
      base = A.row_base ? A.row_base[r] : r;
    }
    const PairCut cut = pair_cut(na, nb, A.cap, A.stride, windows, A.strategy);
    if (have && sub == 0) {
      const unsigned long long both = na + nb < na ? ~0ull : na + nb;
      longest = both > longest ? both : longest;
      if (base < A.rows_cap) {
        n_refused += cut.refused;
        n_lost += !windows && !cut.fits && !cut.refused;
      }
    }
    for (uint64_t w = 0;; w++) {
      const bool live = have && w < cut.k && base < A.rows_cap && w < A.rows_cap - base;
      if (!__any(live)) break;  // the groups of a wavefront walk their windows together, each as far as its own row goes
      if (!live) continue;
      const uint64_t row = base + w;
      // the window's first token of each side and what it keeps of them: first < n on the windowed side (w < k)
      const uint64_t fa = cut.side == kPairWinA ? w * cut.step : 0, fb = cut.side == kPairWinB ? w * cut.step : 0;
      const uint32_t la = cut.side == kPairWinA && na - fa < (uint64_t)cut.keep_a ? (uint32_t)(na - fa) : cut.keep_a;
      const uint32_t lb = cut.side == kPairWinB && nb - fb < (uint64_t)cut.keep_b ? (uint32_t)(nb - fb) : cut.keep_b;
      const uint32_t pa = sp, pb = la + 2 * sp;  // the positions of A's and B's first tokens
      const uint32_t len = cut.refused ? 0 : la + lb + 3 * sp;
      const uint32_t shift = pad_left ? A.width - len : 0;
      const uint64_t slot0 = row * A.width;
      for (uint32_t c0 = sub * kBtQuad; c0 < A.width; c0 += A.group * kBtQuad) {
        uint32_t id[kBtQuad], ty[kBtQuad], sa[kBtQuad], sb[kBtQuad], wd[kBtQuad], mask = 0, special = 0x01010101u, seq = 0xFFFFFFFFu;
#pragma unroll
        for (uint32_t j = 0; j < kBtQuad; j++) {
          const uint32_t p = c0 + j - shift;  // position in the row's content; a pad in front wraps to a large value
          id[j] = A.pad_id; ty[j] = 0; sa[j] = 0; sb[j] = 0; wd[j] = SWT_BATCH_NONE;
          if (p >= len) continue;
          mask |= 1u << (8 * j);
          const uint32_t in_b = p >= pb;
          ty[j] = in_b;
          if (sp && (p == 0 || p + 1 == pb || p + 1 == len)) { id[j] = p ? A.sep_id : A.cls_id; continue; }
          const uint64_t t = in_b ? b0 + fb + (p - pb) : a0 + fa + (p - pa);
          special &= ~(1u << (8 * j));
          seq &= ~((in_b ? 0xFEu : 0xFFu) << (8 * j));
          const uint32_t raw = A.ids[t], s = raw & 0x7FFFFFFFu;
          uint32_t d = SWT_BATCH_NONE;
          if (s < A.n_map) d = A.map ? A.map[(uint64_t)s + ((A.flagged && (raw >> 31)) ? (uint64_t)A.n_map : 0ull)] : s;
          if (d == SWT_BATCH_NONE) { d = A.unk_id; n_unk++; }
          id[j] = d;
          if (A.spans) { sa[j] = A.spans[2 * t]; sb[j] = A.spans[2 * t + 1]; }
          if (A.word) wd[j] = A.word[t];
        }
        const uint64_t slot = slot0 + c0;
        if (A.vec) {
          bt_store_quad(A.out_ids, slot, ids64, id);
          *reinterpret_cast<uint32_t *>(A.out_mask + slot) = mask;
          if (A.out_type) bt_store_quad(A.out_type, slot, ids64, ty);
          if (A.out_special) *reinterpret_cast<uint32_t *>(A.out_special + slot) = special;
          if (A.out_seq) *reinterpret_cast<uint32_t *>(A.out_seq + slot) = seq;
          if (A.out_spans) {
            uint4 *o = reinterpret_cast<uint4 *>(A.out_spans + 2 * slot);
            o[0] = make_uint4(sa[0], sb[0], sa[1], sb[1]);
            o[1] = make_uint4(sa[2], sb[2], sa[3], sb[3]);
          }
          if (A.out_word) *reinterpret_cast<uint4 *>(A.out_word + slot) = make_uint4(wd[0], wd[1], wd[2], wd[3]);
        } else {
#pragma unroll
          for (uint32_t j = 0; j < kBtQuad; j++) {
            if (c0 + j >= A.width) break;
            if (ids64) reinterpret_cast<uint64_t *>(A.out_ids)[slot + j] = id[j];
            else reinterpret_cast<uint32_t *>(A.out_ids)[slot + j] = id[j];
            A.out_mask[slot + j] = (uint8_t)((mask >> (8 * j)) & 1u);
            if (A.out_type) {
              if (ids64) reinterpret_cast<uint64_t *>(A.out_type)[slot + j] = ty[j];
              else reinterpret_cast<uint32_t *>(A.out_type)[slot + j] = ty[j];
            }
            if (A.out_special) A.out_special[slot + j] = (uint8_t)((special >> (8 * j)) & 1u);
            if (A.out_seq) A.out_seq[slot + j] = (int8_t)(uint8_t)(seq >> (8 * j));
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
  for (int d = 32; d; d >>= 1) {
    n_unk += __shfl_xor(n_unk, d, 64);
    n_lost += __shfl_xor(n_lost, d, 64);
    n_refused += __shfl_xor(n_refused, d, 64);
    const unsigned long long o = __shfl_xor(longest, d, 64);
    longest = o > longest ? o : longest;
  }
  if (lane == 0) { counts[wave][0] = longest; counts[wave][1] = n_unk; counts[wave][2] = n_refused; counts[wave][3] = n_lost; }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long most = 0, unk = 0, refused = 0, lost = 0;
    for (int v = 0; v < kBtWaves; v++) {
      most = counts[v][0] > most ? counts[v][0] : most;
      unk += counts[v][1]; refused += counts[v][2]; lost += counts[v][3];
    }
    if (most) atomicMax(&A.info[1], most);
    if (unk) atomicAdd(&A.info[2], unk);
    if (refused) atomicAdd(&A.info[3], refused);
    if (lost) atomicAdd(&A.info[4], lost);
  }
}

// Pair plan, first pass: row_base[r] = k(r) with windows (to be scanned), r itself without; status[r]; info[1] = the largest
// na + nb and info[3] = the refused rows, one atomic each per wavefront that has something to add.
__global__ __launch_bounds__(kBtThreads) void pair_count_kernel(const uint64_t *__restrict__ off_a, const uint64_t *__restrict__ off_b,
                                                                uint64_t n_rows, uint32_t cap, uint32_t stride, int windows,
                                                                uint32_t strategy, unsigned long long *__restrict__ row_base,
                                                                uint8_t *__restrict__ status, unsigned long long *__restrict__ info) {
  const uint64_t i = (uint64_t)blockIdx.x * kBtThreads + threadIdx.x;
  unsigned long long n = 0;
  uint32_t refused = 0;
  if (i < n_rows) {
    const uint64_t a0 = off_a[i], a1 = off_a[i + 1], b0 = off_b[i], b1 = off_b[i + 1];
    const uint64_t na = a1 > a0 ? a1 - a0 : 0, nb = b1 > b0 ? b1 - b0 : 0;
    n = na + nb < na ? ~0ull : na + nb;
    const PairCut cut = pair_cut(na, nb, cap, stride, windows != 0, strategy);
    refused = cut.refused;
    row_base[i] = windows ? cut.k : i;
    status[i] = cut.refused ? SWT_PAIR_REFUSED : SWT_PAIR_OK;
  }
  if (!windows && i == n_rows) {
    row_base[n_rows] = n_rows;
    info[0] = n_rows;
  }
  for (int d = 32; d; d >>= 1) {
    const unsigned long long o = __shfl_xor(n, d, 64);
    n = o > n ? o : n;
    refused += __shfl_xor(refused, d, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    if (n) atomicMax(&info[1], n);
    if (refused) atomicAdd(&info[3], (unsigned long long)refused);
  }
}

// grow-only, shared by all calls of the process (the calls carry no handle); a plan uses it on its own stream, so plans on
// different streams must not overlap -- the header says so
struct BatchWorkspace {
  DevBuf local, blk;
};
static BatchWorkspace g_batch_ws;

static int batch_check_spec(const swt_batch_spec *spec, bool need_width, uint32_t *cap_out, uint32_t *step_out) {
  if (!spec) return fail(SWT_ERR_INVALID, "null argument");
  if (spec->flags & ~kBtFlags) return fail(SWT_ERR_INVALID, "unknown flag");
  *cap_out = 0;
  *step_out = 0;
  if (!need_width) return SWT_OK;
  const uint32_t n_special = (spec->cls_id != SWT_BATCH_NONE) + (spec->sep_id != SWT_BATCH_NONE);
  if (spec->width <= n_special) return fail(SWT_ERR_INVALID, "the width leaves no room for a token");
  const uint32_t cap = spec->width - n_special;
  if (spec->stride >= cap) return fail(SWT_ERR_INVALID, "the stride must be smaller than the tokens of a row");
  if (spec->pad_id == SWT_BATCH_NONE || spec->unk_id == SWT_BATCH_NONE) return fail(SWT_ERR_INVALID, "pad_id and unk_id must be ids");
  *cap_out = cap;
  *step_out = cap - spec->stride;
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

// The spec of a pair call: cls and sep together or not at all; cap = width - 3 with them.  A zero width passes without
// need_width (the plan asked for the largest pair only).
static int pair_check_spec(const swt_batch_spec *spec, uint32_t strategy, bool need_width, uint32_t *cap_out) {
  if (!spec) return fail(SWT_ERR_INVALID, "null argument");
  if (spec->flags & ~kBtFlags) return fail(SWT_ERR_INVALID, "unknown flag");
  if ((spec->cls_id != SWT_BATCH_NONE) != (spec->sep_id != SWT_BATCH_NONE)) return fail(SWT_ERR_INVALID, "a pair row has cls_id and sep_id or neither");
  if (strategy > SWT_PAIR_ONLY_SECOND) return fail(SWT_ERR_INVALID, "unknown truncation strategy");
  if (strategy == SWT_PAIR_LONGEST_FIRST && (spec->flags & SWT_BATCH_WINDOWS))
    return fail(SWT_ERR_INVALID, "longest_first has no windows: take only_first or only_second");
  *cap_out = 0;
  if (!need_width) return SWT_OK;
  const uint32_t n_special = spec->cls_id != SWT_BATCH_NONE ? 3 : 0;
  if (spec->width <= n_special) return fail(SWT_ERR_INVALID, "the width leaves no room for a token");
  const uint32_t cap = spec->width - n_special;
  if (spec->stride >= cap) return fail(SWT_ERR_INVALID, "the stride must be smaller than the tokens of a row");
  if (spec->pad_id == SWT_BATCH_NONE || spec->unk_id == SWT_BATCH_NONE) return fail(SWT_ERR_INVALID, "pad_id and unk_id must be ids");
  *cap_out = cap;
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
  uint32_t cap = 0, step = 0;
  const bool windows = spec && (spec->flags & SWT_BATCH_WINDOWS);
  int rc = batch_check_spec(spec, windows, &cap, &step);
  if (rc) return rc;
  if (!d_tok_off || !d_row_base || !d_info) return fail(SWT_ERR_INVALID, "null argument");
  if ((rc = ensure_device())) return rc;
  hipStream_t st = (hipStream_t)stream;
  unsigned long long *rb = reinterpret_cast<unsigned long long *>(d_row_base), *info = reinterpret_cast<unsigned long long *>(d_info);
  BatchWorkspace &ws = g_batch_ws;
  const uint64_t nb = (n_rows + kBtScanGroup - 1) / kBtScanGroup;
  if (windows && n_rows) {
    if ((rc = ws.local.reserve((size_t)n_rows * 8 + 16))) return rc;
    const void *before = ws.blk.p;
    if ((rc = ws.blk.reserve((size_t)(2 * nb + 4) * 8))) return rc;
    if (ws.blk.p != before) {  // a new buffer: zero the scan's ticket once (the scan resets it itself afterwards)
      SWT_HIP(hipMemset(ws.blk.p, 0, 8));
      SWT_HIP(hipDeviceSynchronize());
    }
  }
  SWT_HIP(hipMemsetAsync(d_info, 0, 16, st));
  if (!n_rows) {
    SWT_HIP(hipMemsetAsync(d_row_base, 0, 8, st));
    return SWT_OK;
  }
  const unsigned grid = (unsigned)((n_rows + 1 + kBtThreads - 1) / kBtThreads);
  hipLaunchKernelGGL(batch_count_kernel, dim3(grid), dim3(kBtThreads), 0, st, d_tok_off, n_rows, cap, step, windows ? 1 : 0, rb, info);
  if (windows) {
    unsigned long long *blk = ws.blk.as<unsigned long long>();
    launch_scan_u64(n_rows, rb, ws.local.as<unsigned long long>(), blk, d_info, st);
    hipLaunchKernelGGL(batch_base_kernel, dim3(grid), dim3(kBtThreads), 0, st, ws.local.as<unsigned long long>(), blk + 1 + nb, n_rows, rb,
                       info);
  }
  SWT_HIP(hipGetLastError());
  return SWT_OK;
} SWT_API_CATCH

int swt_batch_plan(const uint64_t *tok_off, uint64_t n_rows, const swt_batch_spec *spec, uint64_t *row_base, uint64_t *info) try {
  uint32_t cap = 0, step = 0;
  int rc = batch_check_spec(spec, spec && (spec->flags & SWT_BATCH_WINDOWS), &cap, &step);
  if (rc) return rc;
  if (!tok_off || !row_base || !info) return fail(SWT_ERR_INVALID, "null argument");
  for (uint64_t r = 0; r < n_rows; r++)
    if (tok_off[r] > tok_off[r + 1]) return fail(SWT_ERR_INVALID, "offsets must not decrease");
  if ((rc = ensure_device())) return rc;
  DevBuf d[3];  // offsets; row_base, info
  struct Guard { DevBuf *d; ~Guard() { for (int i = 0; i < 3; i++) d[i].release(); } } guard{d};
  const size_t bytes = (size_t)(n_rows + 1) * 8;
  if ((rc = d[0].reserve(bytes + 16)) || (rc = d[1].reserve(bytes + 16)) || (rc = d[2].reserve(32))) return rc;
  SWT_HIP(hipMemcpy(d[0].p, tok_off, bytes, hipMemcpyHostToDevice));
  if ((rc = swt_batch_plan_dev(d[0].as<uint64_t>(), n_rows, spec, d[1].as<uint64_t>(), d[2].as<uint64_t>(), nullptr))) return rc;
  SWT_HIP(hipStreamSynchronize(nullptr));
  SWT_HIP(hipMemcpy(row_base, d[1].p, bytes, hipMemcpyDeviceToHost));
  SWT_HIP(hipMemcpy(info, d[2].p, 16, hipMemcpyDeviceToHost));
  return SWT_OK;
} SWT_API_CATCH

int swt_batch_rows_dev(const uint32_t *d_ids, const uint64_t *d_tok_off, uint64_t n_rows, const uint32_t *d_map, uint32_t n_map, int flagged,
                       const uint32_t *d_spans, const uint32_t *d_word, const swt_batch_spec *spec, const uint64_t *d_row_base,
                       uint64_t rows_cap, void *d_out_ids, uint8_t *d_out_mask, uint32_t *d_out_spans, uint32_t *d_out_word,
                       uint32_t *d_out_sample, uint32_t *d_out_len, uint64_t *d_info, void *stream) try {
  uint32_t cap = 0, step = 0;
  int rc = batch_check_spec(spec, true, &cap, &step);
  if (rc) return rc;
  if ((rc = batch_check_rows(d_map, flagged, d_spans, d_word, spec, d_row_base, n_rows, d_out_ids, d_out_mask, d_out_spans, d_out_word)))
    return rc;
  if (n_rows && (!d_tok_off || !d_ids)) return fail(SWT_ERR_INVALID, "null argument");
  auto aligned = [](const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; };
  if (!aligned(d_out_ids, (spec->flags & SWT_BATCH_IDS64) ? 8 : 4) || !aligned(d_out_spans, 4) || !aligned(d_out_word, 4) ||
      !aligned(d_out_sample, 4) || !aligned(d_out_len, 4) || !aligned(d_info, 8))
    return fail(SWT_ERR_INVALID, "an output is not aligned to its element type");
  if ((rc = ensure_device())) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (d_info) SWT_HIP(hipMemsetAsync(d_info, 0, 24, st));
  if (!n_rows || !rows_cap) return SWT_OK;
  const int vec = spec->width % kBtQuad == 0 && aligned(d_out_ids, 16) && aligned(d_out_mask, 4) && aligned(d_out_spans, 16) &&
                  aligned(d_out_word, 16);
  BatchArgs A{d_ids, d_tok_off, n_rows, d_map, n_map, flagged ? 1 : 0, d_spans, d_word, spec->width, cap, step, spec->flags, spec->pad_id,
              spec->unk_id, spec->cls_id, spec->sep_id, d_row_base, rows_cap, d_out_ids, d_out_mask, d_out_spans, d_out_word, d_out_sample,
              d_out_len, reinterpret_cast<unsigned long long *>(d_info), vec, 1};
  while (A.group < 64 && A.group * kBtQuad < spec->width) A.group *= 2;
  const uint64_t per_block = (uint64_t)kBtWaves * (64 / A.group) * kBtIter;  // source rows of a workgroup
  prof_begin(st);
  hipLaunchKernelGGL(batch_rows_kernel, dim3((unsigned)((n_rows + per_block - 1) / per_block)), dim3(kBtThreads), 0, st, A);
  prof_end(st);
  SWT_HIP(hipGetLastError());
  return SWT_OK;
} SWT_API_CATCH

int swt_batch_rows(const uint32_t *ids, const uint64_t *tok_off, uint64_t n_rows, const uint32_t *map, uint32_t n_map, int flagged,
                   const uint32_t *spans, const uint32_t *word, const swt_batch_spec *spec, const uint64_t *row_base, uint64_t rows_cap,
                   void *out_ids, uint8_t *out_mask, uint32_t *out_spans, uint32_t *out_word, uint32_t *out_sample, uint32_t *out_len,
                   uint64_t *info) try {
  uint32_t cap = 0, step = 0;
  int rc = batch_check_spec(spec, true, &cap, &step);
  if (rc) return rc;
  if ((rc = batch_check_rows(map, flagged, spans, word, spec, row_base, n_rows, out_ids, out_mask, out_spans, out_word))) return rc;
  if (n_rows && !tok_off) return fail(SWT_ERR_INVALID, "null argument");
  const bool windows = (spec->flags & SWT_BATCH_WINDOWS) != 0;
  uint64_t need = 0;
  for (uint64_t r = 0; r < n_rows; r++) {
    if (tok_off[r] > tok_off[r + 1]) return fail(SWT_ERR_INVALID, "offsets must not decrease");
    if (row_base && row_base[r] != need) return fail(SWT_ERR_INVALID, "row_base is not the plan of these offsets");
    need += windows ? bt_windows(tok_off[r + 1] - tok_off[r], cap, step) : 1;
  }
  if (n_rows && row_base && row_base[n_rows] != need) return fail(SWT_ERR_INVALID, "row_base is not the plan of these offsets");
  const uint64_t n_tok = n_rows ? tok_off[n_rows] : 0;
  if (n_tok && !ids) return fail(SWT_ERR_INVALID, "null argument");
  if (info) { info[0] = need; info[1] = 0; info[2] = 0; }
  if (need > rows_cap) return fail(SWT_ERR_CAPACITY, "%llu rows needed, room for %llu", (unsigned long long)need, (unsigned long long)rows_cap);
  if (!n_rows) return SWT_OK;
  if ((rc = ensure_device())) return rc;
  const size_t slots = (size_t)need * spec->width, n_map_all = map ? (size_t)n_map * (flagged ? 2 : 1) : 0;
  const size_t id_bytes = (spec->flags & SWT_BATCH_IDS64) ? 8 : 4;
  DevBuf d[13];  // ids, offsets, map, spans, word, row_base; out ids, mask, spans, word, sample, len, info
  struct Guard { DevBuf *d; ~Guard() { for (int i = 0; i < 13; i++) d[i].release(); } } guard{d};
  const void *src[6] = {ids, tok_off, map, spans, word, row_base};
  void *dst[7] = {out_ids, out_mask, out_spans, out_word, out_sample, out_len, info};
  const size_t bytes[13] = {n_tok * 4, (size_t)(n_rows + 1) * 8, n_map_all * 4, spans ? n_tok * 8 : 0, word ? n_tok * 4 : 0,
                            row_base ? (size_t)(n_rows + 1) * 8 : 0, slots * id_bytes, slots, out_spans ? slots * 8 : 0,
                            out_word ? slots * 4 : 0, out_sample ? (size_t)need * 4 : 0, out_len ? (size_t)need * 4 : 0, info ? (size_t)24 : 0};
  for (int i = 0; i < 13; i++) {
    if ((rc = d[i].reserve(bytes[i] + 16))) return rc;
    if (i < 6 && bytes[i]) SWT_HIP(hipMemcpy(d[i].p, src[i], bytes[i], hipMemcpyHostToDevice));
  }
  auto opt = [&](int i) { return bytes[i] ? d[i].p : nullptr; };
  if ((rc = swt_batch_rows_dev(d[0].as<uint32_t>(), d[1].as<uint64_t>(), n_rows, map ? d[2].as<uint32_t>() : nullptr, n_map, flagged,
                               spans ? d[3].as<uint32_t>() : nullptr, word ? d[4].as<uint32_t>() : nullptr, spec,
                               row_base ? d[5].as<uint64_t>() : nullptr, need, d[6].p, d[7].as<uint8_t>(),
                               out_spans ? d[8].as<uint32_t>() : nullptr, out_word ? d[9].as<uint32_t>() : nullptr,
                               (uint32_t *)opt(10), (uint32_t *)opt(11), (uint64_t *)opt(12), nullptr)))
    return rc;
  SWT_HIP(hipStreamSynchronize(nullptr));
  for (int i = 0; i < 7; i++)
    if (bytes[6 + i]) SWT_HIP(hipMemcpy(dst[i], d[6 + i].p, bytes[6 + i], hipMemcpyDeviceToHost));
  return SWT_OK;
} SWT_API_CATCH

int swt_batch_pair_capacity(uint32_t *cols_per_step, uint32_t *scan_group) try {
  return swt_batch_capacity(cols_per_step, scan_group);  // the pair kernels keep the skeleton and the scan of the single ones
} SWT_API_CATCH

int swt_batch_pair_plan_dev(const uint64_t *d_off_a, const uint64_t *d_off_b, uint64_t n_rows, const swt_batch_spec *spec, uint32_t strategy,
                            uint64_t *d_row_base, uint8_t *d_status, uint64_t *d_info, void *stream) try {
  uint32_t cap = 0;
  const bool windows = spec && (spec->flags & SWT_BATCH_WINDOWS);
  const bool sized = spec && spec->width != 0;  // a zero width: only the largest pair is asked for, every row counts as fitting
  int rc = pair_check_spec(spec, strategy, windows || sized, &cap);
  if (rc) return rc;
  if (!d_off_a || !d_off_b || !d_row_base || !d_status || !d_info) return fail(SWT_ERR_INVALID, "null argument");
  if (n_rows > 0xFFFFFFFFull) return fail(SWT_ERR_INVALID, "2^32 rows or more");
  if ((rc = ensure_device())) return rc;
  if (!sized) cap = 0xFFFFFFFFu;
  hipStream_t st = (hipStream_t)stream;
  unsigned long long *rb = reinterpret_cast<unsigned long long *>(d_row_base), *info = reinterpret_cast<unsigned long long *>(d_info);
  BatchWorkspace &ws = g_batch_ws;
  const uint64_t nb = (n_rows + kBtScanGroup - 1) / kBtScanGroup;
  if (windows && n_rows) {
    if ((rc = ws.local.reserve((size_t)n_rows * 8 + 16))) return rc;
    const void *before = ws.blk.p;
    if ((rc = ws.blk.reserve((size_t)(2 * nb + 4) * 8))) return rc;
    if (ws.blk.p != before) {  // a new buffer: zero the scan's ticket once (the scan resets it itself afterwards)
      SWT_HIP(hipMemset(ws.blk.p, 0, 8));
      SWT_HIP(hipDeviceSynchronize());
    }
  }
  SWT_HIP(hipMemsetAsync(d_info, 0, 40, st));
  if (!n_rows) {
    SWT_HIP(hipMemsetAsync(d_row_base, 0, 8, st));
    return SWT_OK;
  }
  const unsigned grid = (unsigned)((n_rows + 1 + kBtThreads - 1) / kBtThreads);
  hipLaunchKernelGGL(pair_count_kernel, dim3(grid), dim3(kBtThreads), 0, st, d_off_a, d_off_b, n_rows, cap, spec->stride, windows ? 1 : 0,
                     strategy, rb, d_status, info);
  if (windows) {
    unsigned long long *blk = ws.blk.as<unsigned long long>();
    launch_scan_u64(n_rows, rb, ws.local.as<unsigned long long>(), blk, d_info, st);
    hipLaunchKernelGGL(batch_base_kernel, dim3(grid), dim3(kBtThreads), 0, st, ws.local.as<unsigned long long>(), blk + 1 + nb, n_rows, rb,
                       info);
  }
  SWT_HIP(hipGetLastError());
  return SWT_OK;
} SWT_API_CATCH

int swt_batch_pair_plan(const uint64_t *off_a, const uint64_t *off_b, uint64_t n_rows, const swt_batch_spec *spec, uint32_t strategy,
                        uint64_t *row_base, uint8_t *status, uint64_t *info) try {
  uint32_t cap = 0;
  int rc = pair_check_spec(spec, strategy, spec && ((spec->flags & SWT_BATCH_WINDOWS) || spec->width != 0), &cap);
  if (rc) return rc;
  if (!off_a || !off_b || !row_base || !status || !info) return fail(SWT_ERR_INVALID, "null argument");
  for (uint64_t r = 0; r < n_rows; r++)
    if (off_a[r] > off_a[r + 1] || off_b[r] > off_b[r + 1]) return fail(SWT_ERR_INVALID, "offsets must not decrease");
  if ((rc = ensure_device())) return rc;
  DevBuf d[5];  // offsets of A, of B; row_base, status, info
  struct Guard { DevBuf *d; ~Guard() { for (int i = 0; i < 5; i++) d[i].release(); } } guard{d};
  const size_t bytes = (size_t)(n_rows + 1) * 8;
  if ((rc = d[0].reserve(bytes + 16)) || (rc = d[1].reserve(bytes + 16)) || (rc = d[2].reserve(bytes + 16)) ||
      (rc = d[3].reserve((size_t)n_rows + 16)) || (rc = d[4].reserve(48)))
    return rc;
  SWT_HIP(hipMemcpy(d[0].p, off_a, bytes, hipMemcpyHostToDevice));
  SWT_HIP(hipMemcpy(d[1].p, off_b, bytes, hipMemcpyHostToDevice));
  if ((rc = swt_batch_pair_plan_dev(d[0].as<uint64_t>(), d[1].as<uint64_t>(), n_rows, spec, strategy, d[2].as<uint64_t>(), d[3].as<uint8_t>(),
                                    d[4].as<uint64_t>(), nullptr)))
    return rc;
  SWT_HIP(hipStreamSynchronize(nullptr));
  SWT_HIP(hipMemcpy(row_base, d[2].p, bytes, hipMemcpyDeviceToHost));
  if (n_rows) SWT_HIP(hipMemcpy(status, d[3].p, (size_t)n_rows, hipMemcpyDeviceToHost));
  SWT_HIP(hipMemcpy(info, d[4].p, 40, hipMemcpyDeviceToHost));
  return SWT_OK;
} SWT_API_CATCH

int swt_batch_pair_rows_dev(const uint32_t *d_ids, const uint64_t *d_off_a, const uint64_t *d_off_b, uint64_t n_rows, const uint32_t *d_map,
                            uint32_t n_map, int flagged, const uint32_t *d_spans, const uint32_t *d_word, const swt_batch_spec *spec,
                            uint32_t strategy, const uint64_t *d_row_base, const uint8_t *d_status, uint64_t rows_cap, void *d_out_ids,
                            uint8_t *d_out_mask, void *d_out_type, uint8_t *d_out_special, int8_t *d_out_seq, uint32_t *d_out_spans,
                            uint32_t *d_out_word, uint32_t *d_out_sample, uint32_t *d_out_len, uint64_t *d_info, void *stream) try {
  uint32_t cap = 0;
  int rc = pair_check_spec(spec, strategy, true, &cap);
  if (rc) return rc;
  if ((rc = batch_check_rows(d_map, flagged, d_spans, d_word, spec, d_row_base, n_rows, d_out_ids, d_out_mask, d_out_spans, d_out_word)))
    return rc;
  if (n_rows && (!d_off_a || !d_off_b || !d_ids)) return fail(SWT_ERR_INVALID, "null argument");
  (void)d_status;  // the kernel takes every row's cut from its offsets, as it takes the window counts: nothing a caller hands in steers a store
  auto aligned = [](const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; };
  const uintptr_t id_bytes = (spec->flags & SWT_BATCH_IDS64) ? 8 : 4;
  if (!aligned(d_out_ids, id_bytes) || !aligned(d_out_type, id_bytes) || !aligned(d_out_spans, 4) || !aligned(d_out_word, 4) ||
      !aligned(d_out_sample, 4) || !aligned(d_out_len, 4) || !aligned(d_info, 8))
    return fail(SWT_ERR_INVALID, "an output is not aligned to its element type");
  if ((rc = ensure_device())) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (d_info) SWT_HIP(hipMemsetAsync(d_info, 0, 40, st));
  if (!n_rows || !rows_cap) return SWT_OK;
  const int vec = spec->width % kBtQuad == 0 && aligned(d_out_ids, 16) && aligned(d_out_mask, 4) && aligned(d_out_type, 16) &&
                  aligned(d_out_special, 4) && aligned(d_out_seq, 4) && aligned(d_out_spans, 16) && aligned(d_out_word, 16);
  PairArgs A{d_ids, d_off_a, d_off_b, n_rows, d_map, n_map, flagged ? 1 : 0, d_spans, d_word, spec->width, cap, spec->stride, spec->flags,
             strategy, spec->pad_id, spec->unk_id, spec->cls_id, spec->sep_id, d_row_base, rows_cap, d_out_ids, d_out_mask, d_out_type,
             d_out_special, d_out_seq, d_out_spans, d_out_word, d_out_sample, d_out_len, reinterpret_cast<unsigned long long *>(d_info), vec, 1};
  while (A.group < 64 && A.group * kBtQuad < spec->width) A.group *= 2;
  const uint64_t per_block = (uint64_t)kBtWaves * (64 / A.group) * kBtIter;  // pairs of a workgroup
  prof_begin(st);
  hipLaunchKernelGGL(pair_rows_kernel, dim3((unsigned)((n_rows + per_block - 1) / per_block)), dim3(kBtThreads), 0, st, A);
  prof_end(st);
  SWT_HIP(hipGetLastError());
  return SWT_OK;
} SWT_API_CATCH

int swt_batch_pair_rows(const uint32_t *ids, const uint64_t *off_a, const uint64_t *off_b, uint64_t n_rows, const uint32_t *map, uint32_t n_map,
                        int flagged, const uint32_t *spans, const uint32_t *word, const swt_batch_spec *spec, uint32_t strategy,
                        const uint64_t *row_base, const uint8_t *status, uint64_t rows_cap, void *out_ids, uint8_t *out_mask, void *out_type,
                        uint8_t *out_special, int8_t *out_seq, uint32_t *out_spans, uint32_t *out_word, uint32_t *out_sample, uint32_t *out_len,
                        uint64_t *info) try {
  uint32_t cap = 0;
  int rc = pair_check_spec(spec, strategy, true, &cap);
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
  constexpr int kIn = 7, kOut = 10;
  DevBuf d[kIn + kOut];  // ids, offsets of A, of B, map, spans, word, row_base; out ids, mask, type, special, seq, spans, word, sample, len, info
  struct Guard { DevBuf *d; ~Guard() { for (int i = 0; i < kIn + kOut; i++) d[i].release(); } } guard{d};
  const void *src[kIn] = {ids, off_a, off_b, map, spans, word, row_base};
  void *dst[kOut] = {out_ids, out_mask, out_type, out_special, out_seq, out_spans, out_word, out_sample, out_len, info};
  const size_t bytes[kIn + kOut] = {n_tok * 4, off_bytes, off_bytes, n_map_all * 4, spans ? n_tok * 8 : 0, word ? n_tok * 4 : 0,
                                    row_base ? off_bytes : 0, slots * id_bytes, slots, out_type ? slots * id_bytes : 0, out_special ? slots : 0,
                                    out_seq ? slots : 0, out_spans ? slots * 8 : 0, out_word ? slots * 4 : 0, out_sample ? (size_t)need * 4 : 0,
                                    out_len ? (size_t)need * 4 : 0, info ? (size_t)40 : 0};
  for (int i = 0; i < kIn + kOut; i++) {
    if ((rc = d[i].reserve(bytes[i] + 16))) return rc;
    if (i < kIn && bytes[i]) SWT_HIP(hipMemcpy(d[i].p, src[i], bytes[i], hipMemcpyHostToDevice));
  }
  auto opt = [&](int i, const void *given) { return given ? d[i].p : nullptr; };
  if ((rc = swt_batch_pair_rows_dev(d[0].as<uint32_t>(), d[1].as<uint64_t>(), d[2].as<uint64_t>(), n_rows, (const uint32_t *)opt(3, map), n_map,
                                    flagged, (const uint32_t *)opt(4, spans), (const uint32_t *)opt(5, word), spec, strategy,
                                    (const uint64_t *)opt(6, row_base), nullptr, need, d[7].p, d[8].as<uint8_t>(), opt(9, out_type),
                                    (uint8_t *)opt(10, out_special), (int8_t *)opt(11, out_seq), (uint32_t *)opt(12, out_spans),
                                    (uint32_t *)opt(13, out_word), (uint32_t *)opt(14, out_sample), (uint32_t *)opt(15, out_len),
                                    (uint64_t *)opt(16, info), nullptr)))
    return rc;
  SWT_HIP(hipStreamSynchronize(nullptr));
  for (int i = 0; i < kOut; i++)
    if (bytes[kIn + i]) SWT_HIP(hipMemcpy(dst[i], d[kIn + i].p, bytes[kIn + i], hipMemcpyDeviceToHost));
  return SWT_OK;
} SWT_API_CATCH

}  // extern "C"
