// swt_decode.hip -- decoding on the device: finished rows of dense ids back to text, as the reference's recover_sentence spells
// the rows' tokens.  Semantics: include/swt.h; tests/decode_cases.py holds them in Python; the design and its measurements:
// DESIGN.md 4.13.
//
// decode_kernel<T, kRows>: one routine, two instantiations -- the plan (kRows = false: a row's byte length and status, the
// workgroup's counts) and the rows (kRows = true: the bytes).  ROW-major: a group of g lanes per row (swt_rows.h), so that narrow
// rows share a wavefront; a row wider than 4 g columns takes several steps.  A step:
//   load     the lane's quad of ids (bt_load_quad) and of the mask (one 4-byte load), when the width is a multiple of four and
//            the pointer is aligned; else column by column
//   flags    which columns are kept, which of them write, the status bits, the token's flags and bytes
//   previous "the last writing column before this one: none, one that takes a space after it, one that is NO_SPACE_AFTER" --
//            last-nonzero-scanned inside the quad, then over the lanes of the group (__shfl_up, a lane taking nothing from below
//            its group), then joined with the carry of the steps before
//   lengths  token bytes, minus two if glued, plus one if spaced; exclusive sum the same three ways, with a byte carry
//   stores   (rows) by output byte: the step's (output offset, source offset) of every column staged in LDS, a lane takes every
//            g-th byte of its group's step and finds the byte's column by search -- coalesced stores.  A lane writing its own
//            tokens byte by byte was the first build and lost (profiles/decode_rows.txt)
// The loop over the steps and the sets is uniform over the wavefront (the width and the sets are the launch's), a row beyond
// `rows` is masked, not skipped: every lane meets every shuffle.  The two counts of the plan are stored per workgroup;
// launch_counts_sum sums them into info.  No atomic anywhere.
#include "swt_batch.h"

namespace swt {

constexpr int kDcThreads = 256;
constexpr int kDcWaves = kDcThreads / 64;
constexpr uint32_t kDcFlags = SWT_DECODE_SKIP_SPECIAL | SWT_DECODE_IDS64;
constexpr uint32_t kDcCounts = 2;  // rows with a nonzero status, kept columns: info[1], info[2]

struct DecodeArgs {
  const void *ids;
  const uint8_t *mask;
  uint64_t rows;
  uint32_t width;
  const uint8_t *tok_bytes;
  const uint32_t *tok_off;
  const uint8_t *tok_flags;
  uint32_t n_tok, skip;
  unsigned long long *row_len;  // plan: the bytes of every row (the scan makes text_off of them in place)
  uint8_t *status;
  unsigned long long *part;  // plan: the counts of every workgroup, kDcCounts each
  const unsigned long long *text_off;  // rows
  uint8_t *out_text;
  uint64_t text_cap;
  int vec_ids, vec_mask;  // the wide loads: the width is a multiple of four and the pointer is aligned
  uint32_t group;         // lanes per row: a power of two, 1 .. 64
  uint32_t sets;          // sets of rows a wavefront walks
};

template <class T, bool kRows>
__global__ __launch_bounds__(kDcThreads) void decode_kernel(DecodeArgs A) {
  __shared__ unsigned long long counts[kDcWaves][kDcCounts];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t g = A.group, sub = lane & (g - 1), per_wave = 64 / g;
  const uint32_t group_last = lane | (g - 1);  // the last lane of this lane's group
  const T *ids = reinterpret_cast<const T *>(A.ids);
  uint32_t n[kDcCounts] = {0, 0};
  const uint64_t b0 = ((uint64_t)blockIdx.x * kDcWaves + wave) * per_wave * A.sets + lane / g;
  for (uint32_t it = 0; it < A.sets; it++) {
    const uint64_t b = b0 + (uint64_t)it * per_wave;
    const bool live = b < A.rows;
    const uint64_t at = live ? b * A.width : 0;
    uint64_t lo = 0, hi = 0;  // rows: the row's own range, cut at the capacity; an empty range stores nothing
    if constexpr (kRows) {
      if (live) {
        lo = A.text_off[b];
        hi = A.text_off[b + 1];
        if (hi > A.text_cap) hi = A.text_cap;
      }
    }
    uint32_t carry_prev = 0;   // the last writing column of the steps before: 0 none, 1 takes a space after it, 2 NO_SPACE_AFTER
    uint64_t carry_bytes = 0;  // the row's bytes of the steps before
    uint32_t status = 0;
    for (uint64_t base = 0; base < A.width; base += (uint64_t)g * kBtQuad) {
      const uint64_t c0 = base + (uint64_t)sub * kBtQuad;
      const bool whole = live && c0 + kBtQuad <= A.width;
      T v[kBtQuad];
      uint32_t m = 0x01010101u;  // the quad's mask bytes
      if (A.vec_ids) {
        if (whole) bt_load_quad<T>(ids + at + c0, v);
      } else {
#pragma unroll
        for (uint32_t j = 0; j < kBtQuad; j++)
          if (live && c0 + j < A.width) v[j] = ids[at + c0 + j];
      }
      if (A.mask) {
        if (A.vec_mask) {
          if (whole) m = *reinterpret_cast<const uint32_t *>(A.mask + at + c0);
        } else {
          m = 0;
#pragma unroll
          for (uint32_t j = 0; j < kBtQuad; j++)
            if (live && c0 + j < A.width) m |= (uint32_t)A.mask[at + c0 + j] << (8 * j);
        }
      }
      uint32_t own[kBtQuad], fl[kBtQuad], src[kBtQuad], nb[kBtQuad];
#pragma unroll
      for (uint32_t j = 0; j < kBtQuad; j++) {
        own[j] = fl[j] = src[j] = nb[j] = 0;
        if (!live || c0 + j >= A.width || !((m >> (8 * j)) & 0xFFu)) continue;  // nothing is looked up for such a column
        const int64_t id = (int64_t)v[j];
        if (id < 0 || id >= (int64_t)A.n_tok) { status |= 1u; n[1]++; continue; }
        const uint32_t f = A.tok_flags[id];
        if (A.skip && (f & SWT_TOK_SPECIAL)) continue;
        n[1]++;
        if (f & SWT_TOK_BAD) { status |= 2u; continue; }
        fl[j] = f;
        own[j] = (f & SWT_TOK_NO_SPACE_AFTER) ? 2u : 1u;
        src[j] = A.tok_off[id];
        const uint32_t end = A.tok_off[id + 1];
        nb[j] = end > src[j] ? end - src[j] : 0;
      }
      // the last writing column up to and including each lane's quad, over the lanes of the group
      uint32_t run = 0;
#pragma unroll
      for (uint32_t j = 0; j < kBtQuad; j++)
        if (own[j]) run = own[j];
      for (uint32_t d = 1; d < g; d <<= 1) {
        const uint32_t o = __shfl_up(run, d, 64);
        if (sub >= d && !run) run = o;
      }
      uint32_t prev = __shfl_up(run, 1, 64);
      if (!sub) prev = 0;  // nothing from below the group
      if (!prev) prev = carry_prev;
      const uint32_t step_last = __shfl(run, group_last, 64);
      if (step_last) carry_prev = step_last;

      // a step's bytes fit 32 bits: 256 columns of a vocabulary below 2^23 bytes (the header's bound), a space each
      uint32_t len[kBtQuad], cut[kBtQuad], space[kBtQuad], mine = 0;
#pragma unroll
      for (uint32_t j = 0; j < kBtQuad; j++) {
        len[j] = cut[j] = space[j] = 0;
        if (!own[j]) continue;
        const bool glue = prev && (fl[j] & SWT_TOK_GLUE);
        if (glue) cut[j] = nb[j] < 2 ? nb[j] : 2;
        space[j] = prev == 1 && !glue && !(fl[j] & SWT_TOK_NO_SPACE_BEFORE);
        len[j] = nb[j] - cut[j] + space[j];
        mine += len[j];
        prev = own[j];
      }
      uint32_t x = mine;
      for (uint32_t d = 1; d < g; d <<= 1) {
        const uint32_t o = __shfl_up(x, d, 64);
        if (sub >= d) x += o;
      }
      const uint32_t step_bytes = __shfl(x, group_last, 64);
      if constexpr (kRows) {
        // the step's (output offset, source offset, space) of every column goes to LDS; a lane takes every g-th byte of its
        // group's step and finds the byte's column by search, so neighbouring lanes store neighbouring bytes
        __shared__ uint32_t s_off[kDcWaves][kBtCols], s_src[kDcWaves][kBtCols];
        __shared__ uint8_t s_space[kDcWaves][kBtCols];
        uint32_t e = x - mine;
#pragma unroll
        for (uint32_t j = 0; j < kBtQuad; j++) {
          s_off[wave][lane * kBtQuad + j] = e;
          s_src[wave][lane * kBtQuad + j] = src[j] + cut[j] - space[j];  // of the column's byte 0, were the space a byte of the token
          s_space[wave][lane * kBtQuad + j] = (uint8_t)space[j];
          e += len[j];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const uint32_t first = (lane - sub) * kBtQuad, n_col = g * kBtQuad;
        for (uint32_t k = sub; k < step_bytes; k += g) {
          uint32_t c = 0;  // the last column that starts at or before byte k: columns of no byte share their successor's offset
          for (uint32_t s = n_col >> 1; s; s >>= 1)
            if (s_off[wave][first + c + s] <= k) c += s;
          const uint32_t d = k - s_off[wave][first + c];
          const uint8_t byte = s_space[wave][first + c] && !d ? (uint8_t)0x20 : A.tok_bytes[s_src[wave][first + c] + d];
          const uint64_t o = lo + carry_bytes + k;
          if (o < hi) A.out_text[o] = byte;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();  // the reads are done before the next step stages its columns
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      }
      carry_bytes += step_bytes;
    }
    if constexpr (!kRows) {
      for (uint32_t d = 1; d < g; d <<= 1) status |= __shfl_xor(status, d, 64);  // stays inside the group: g is a power of two
      if (live && !sub) {
        A.row_len[b] = carry_bytes;
        A.status[b] = (uint8_t)status;
        if (status) n[0]++;
      }
    }
  }
  if constexpr (!kRows) {
    const unsigned long long sum = bt_fold_counts(n, counts);
    if (threadIdx.x < kDcCounts) A.part[(uint64_t)blockIdx.x * kDcCounts + threadIdx.x] = sum;
  }
}

// the workgroups' counts between the launches of a plan: grow-only and shared by all calls of the process, as the scan workspace
static DevBuf g_decode_ws;

// What every form refuses, from the arguments alone.
static int decode_check(const void *ids, uint64_t rows, uint32_t width, const uint32_t *tok_off, const uint8_t *tok_flags, uint32_t n_tok,
                        uint32_t flags) {
  if (!ids) return fail(SWT_ERR_INVALID, "null argument: ids");
  if (!tok_off) return fail(SWT_ERR_INVALID, "null argument: tok_off");
  if (!tok_flags) return fail(SWT_ERR_INVALID, "null argument: tok_flags");
  if (int rc = bt_check_shape(rows, width)) return rc;
  if (flags & ~kDcFlags) return fail(SWT_ERR_INVALID, "flags: unknown flag");
  if (!n_tok) return fail(SWT_ERR_INVALID, "n_tok: a vocabulary of no token");
  return SWT_OK;
}

static int decode_check_table(const uint32_t *tok_off, uint32_t n_tok) {
  if (tok_off[n_tok] >= (1u << 23)) return fail(SWT_ERR_INVALID, "tok_off: a vocabulary of 2^23 bytes or more");
  for (uint32_t i = 0; i < n_tok; i++)
    if (tok_off[i] > tok_off[i + 1]) return fail(SWT_ERR_INVALID, "tok_off: offsets must not decrease");
  return SWT_OK;
}

// The lanes of a row, the sets of a wavefront, the wide loads; -> the workgroups of the launch.
static unsigned decode_shape(DecodeArgs &A) {
  A.vec_ids = A.width % kBtQuad == 0 && bt_aligned(16, {A.ids});
  A.vec_mask = A.width % kBtQuad == 0 && bt_aligned(4, {A.mask});
  A.group = bt_group(A.width);
  const RowShape shape = bt_shape(A.rows, A.group, kDcWaves);
  A.sets = (uint32_t)shape.sets;
  return shape.grid;
}

// The bytes and the status of one row on the host: what swt_decode_rows holds text_off against before the device is touched.
template <class T>
static uint64_t decode_row_host(const T *ids, const uint8_t *mask, uint32_t width, const uint32_t *tok_off, const uint8_t *tok_flags,
                                uint32_t n_tok, bool skip) {
  uint64_t bytes = 0;
  uint32_t prev = 0;
  for (uint32_t c = 0; c < width; c++) {
    if (mask && !mask[c]) continue;
    const int64_t id = (int64_t)ids[c];
    if (id < 0 || id >= (int64_t)n_tok) continue;
    const uint32_t f = tok_flags[id];
    if ((skip && (f & SWT_TOK_SPECIAL)) || (f & SWT_TOK_BAD)) continue;
    const uint32_t nb = tok_off[id + 1] - tok_off[id];
    const bool glue = prev && (f & SWT_TOK_GLUE);
    bytes += glue ? nb - (nb < 2 ? nb : 2) : nb + (prev == 1 && !(f & SWT_TOK_NO_SPACE_BEFORE));
    prev = (f & SWT_TOK_NO_SPACE_AFTER) ? 2 : 1;
  }
  return bytes;
}

}  // namespace swt

using namespace swt;

extern "C" {

int swt_decode_capacity(uint32_t *cols_per_step, uint32_t *scan_group) try {
  if (cols_per_step) *cols_per_step = kBtCols;
  if (scan_group) *scan_group = kBtScanGroup;
  return SWT_OK;
} SWT_API_CATCH

int swt_decode_plan_dev(const void *d_ids, const uint8_t *d_mask, uint64_t rows, uint32_t width, const uint32_t *d_tok_off,
                        const uint8_t *d_tok_flags, uint32_t n_tok, uint32_t flags, uint64_t *d_text_off, uint8_t *d_status, uint64_t *d_info,
                        void *stream) try {
  int rc = decode_check(d_ids, rows, width, d_tok_off, d_tok_flags, n_tok, flags);
  if (rc) return rc;
  if (!d_text_off) return fail(SWT_ERR_INVALID, "null argument: text_off");
  if (!d_status) return fail(SWT_ERR_INVALID, "null argument: status");
  if (!d_info) return fail(SWT_ERR_INVALID, "null argument: info");
  if (!bt_aligned((flags & SWT_DECODE_IDS64) ? 8 : 4, {d_ids}) || !bt_aligned(4, {d_tok_off}) || !bt_aligned(8, {d_text_off, d_info}))
    return fail(SWT_ERR_INVALID, "an array is not aligned to its element type");
  if ((rc = ensure_device())) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (!rows) {
    SWT_HIP(hipMemsetAsync(d_info, 0, 24, st));
    SWT_HIP(hipMemsetAsync(d_text_off, 0, 8, st));
    return SWT_OK;
  }
  DecodeArgs A{d_ids, d_mask, rows, width, nullptr, d_tok_off, d_tok_flags, n_tok, (flags & SWT_DECODE_SKIP_SPECIAL) ? 1u : 0u,
               reinterpret_cast<unsigned long long *>(d_text_off), d_status, nullptr, nullptr, nullptr, 0, 0, 0, 1, 1};
  const unsigned grid = decode_shape(A);
  if ((rc = g_batch_ws.reserve(rows))) return rc;
  if ((rc = g_decode_ws.reserve((size_t)grid * kDcCounts * 8))) return rc;
  A.part = g_decode_ws.as<unsigned long long>();
  if (flags & SWT_DECODE_IDS64) hipLaunchKernelGGL((decode_kernel<int64_t, false>), dim3(grid), dim3(kDcThreads), 0, st, A);
  else hipLaunchKernelGGL((decode_kernel<int32_t, false>), dim3(grid), dim3(kDcThreads), 0, st, A);
  launch_scan_bases(rows, A.row_len, d_info, st);
  launch_counts_sum(A.part, grid, kDcCounts, reinterpret_cast<unsigned long long *>(d_info) + 1, st);
  SWT_HIP(hipGetLastError());
  return SWT_OK;
} SWT_API_CATCH

int swt_decode_rows_dev(const void *d_ids, const uint8_t *d_mask, uint64_t rows, uint32_t width, const uint8_t *d_tok_bytes,
                        const uint32_t *d_tok_off, const uint8_t *d_tok_flags, uint32_t n_tok, uint32_t flags, const uint64_t *d_text_off,
                        uint8_t *d_out_text, uint64_t text_cap, void *stream) try {
  int rc = decode_check(d_ids, rows, width, d_tok_off, d_tok_flags, n_tok, flags);
  if (rc) return rc;
  if (!d_tok_bytes) return fail(SWT_ERR_INVALID, "null argument: tok_bytes");
  if (!d_text_off) return fail(SWT_ERR_INVALID, "null argument: text_off");
  if (!d_out_text) return fail(SWT_ERR_INVALID, "null argument: out_text");
  if (!bt_aligned((flags & SWT_DECODE_IDS64) ? 8 : 4, {d_ids}) || !bt_aligned(4, {d_tok_off}) || !bt_aligned(8, {d_text_off}))
    return fail(SWT_ERR_INVALID, "an array is not aligned to its element type");
  if ((rc = ensure_device())) return rc;
  if (!rows || !text_cap) return SWT_OK;
  DecodeArgs A{d_ids, d_mask, rows, width, d_tok_bytes, d_tok_off, d_tok_flags, n_tok, (flags & SWT_DECODE_SKIP_SPECIAL) ? 1u : 0u,
               nullptr, nullptr, nullptr, reinterpret_cast<const unsigned long long *>(d_text_off), d_out_text, text_cap, 0, 0, 1, 1};
  const unsigned grid = decode_shape(A);
  hipStream_t st = (hipStream_t)stream;
  if (flags & SWT_DECODE_IDS64) hipLaunchKernelGGL((decode_kernel<int64_t, true>), dim3(grid), dim3(kDcThreads), 0, st, A);
  else hipLaunchKernelGGL((decode_kernel<int32_t, true>), dim3(grid), dim3(kDcThreads), 0, st, A);
  SWT_HIP(hipGetLastError());
  return SWT_OK;
} SWT_API_CATCH

int swt_decode_plan(const void *ids, const uint8_t *mask, uint64_t rows, uint32_t width, const uint32_t *tok_off, const uint8_t *tok_flags,
                    uint32_t n_tok, uint32_t flags, uint64_t *text_off, uint8_t *status, uint64_t *info) try {
  int rc = decode_check(ids, rows, width, tok_off, tok_flags, n_tok, flags);
  if (rc) return rc;
  if (!text_off) return fail(SWT_ERR_INVALID, "null argument: text_off");
  if (!status) return fail(SWT_ERR_INVALID, "null argument: status");
  if (!info) return fail(SWT_ERR_INVALID, "null argument: info");
  if ((rc = decode_check_table(tok_off, n_tok))) return rc;
  info[0] = info[1] = info[2] = 0;
  text_off[0] = 0;
  if (!rows) return SWT_OK;
  if ((rc = ensure_device())) return rc;
  const size_t cells = (size_t)rows * width;
  BatchStage s;
  const void *d_ids = s.in(static_cast<const uint8_t *>(ids), cells * ((flags & SWT_DECODE_IDS64) ? 8 : 4));
  const uint8_t *d_mask = s.in(mask, cells);
  const uint32_t *d_off = s.in(tok_off, ((size_t)n_tok + 1) * 4);
  const uint8_t *d_flags = s.in(tok_flags, n_tok);
  uint64_t *d_text_off = s.out(text_off, (size_t)(rows + 1) * 8), *d_info = s.out(info, 24);
  uint8_t *d_status = s.out(status, rows);
  if (s.rc) return s.rc;
  if ((rc = swt_decode_plan_dev(d_ids, d_mask, rows, width, d_off, d_flags, n_tok, flags, d_text_off, d_status, d_info, nullptr))) return rc;
  return s.fetch();
} SWT_API_CATCH

int swt_decode_rows(const void *ids, const uint8_t *mask, uint64_t rows, uint32_t width, const uint8_t *tok_bytes, const uint32_t *tok_off,
                    const uint8_t *tok_flags, uint32_t n_tok, uint32_t flags, const uint64_t *text_off, uint8_t *out_text,
                    uint64_t text_cap) try {
  int rc = decode_check(ids, rows, width, tok_off, tok_flags, n_tok, flags);
  if (rc) return rc;
  if (!tok_bytes) return fail(SWT_ERR_INVALID, "null argument: tok_bytes");
  if (!text_off) return fail(SWT_ERR_INVALID, "null argument: text_off");
  if (!out_text) return fail(SWT_ERR_INVALID, "null argument: out_text");
  if ((rc = decode_check_table(tok_off, n_tok))) return rc;
  const bool skip = (flags & SWT_DECODE_SKIP_SPECIAL) != 0, ids64 = (flags & SWT_DECODE_IDS64) != 0;
  if (text_off[0]) return fail(SWT_ERR_INVALID, "text_off: not the plan of these ids");
  for (uint64_t r = 0; r < rows; r++) {
    const uint8_t *m = mask ? mask + r * width : nullptr;
    const uint64_t bytes = ids64 ? decode_row_host(static_cast<const int64_t *>(ids) + r * width, m, width, tok_off, tok_flags, n_tok, skip)
                                 : decode_row_host(static_cast<const int32_t *>(ids) + r * width, m, width, tok_off, tok_flags, n_tok, skip);
    if (text_off[r + 1] < text_off[r] || text_off[r + 1] - text_off[r] != bytes)
      return fail(SWT_ERR_INVALID, "text_off: not the plan of these ids");
  }
  const uint64_t total = text_off[rows];
  if (text_cap < total) return fail(SWT_ERR_CAPACITY, "text_cap is below the bytes of the plan");
  if (!rows || !total) return SWT_OK;
  if ((rc = ensure_device())) return rc;
  const size_t cells = (size_t)rows * width;
  BatchStage s;
  const void *d_ids = s.in(static_cast<const uint8_t *>(ids), cells * (ids64 ? 8 : 4));
  const uint8_t *d_mask = s.in(mask, cells);
  const uint8_t *d_bytes = s.in(tok_bytes, tok_off[n_tok], true);
  const uint32_t *d_off = s.in(tok_off, ((size_t)n_tok + 1) * 4);
  const uint8_t *d_flags = s.in(tok_flags, n_tok);
  const uint64_t *d_text_off = s.in(text_off, (size_t)(rows + 1) * 8);
  uint8_t *d_out = s.out(out_text, total);
  if (s.rc) return s.rc;
  if ((rc = swt_decode_rows_dev(d_ids, d_mask, rows, width, d_bytes, d_off, d_flags, n_tok, flags, d_text_off, d_out, total, nullptr))) return rc;
  return s.fetch();
} SWT_API_CATCH

}  // extern "C"
