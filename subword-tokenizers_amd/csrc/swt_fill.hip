// swt_fill.hip -- masked-LM inference on the device, over a model's logits [rows, width, V] at selected cells only: which cells
// (swt_mlm_positions), and per selected cell the log-sum-exp of its row of V floats, the first k entries of the row under one
// total order, and the label's logit and rank (swt_mlm_predict).  Semantics: include/swt.h; tests/fill_cases.py holds them in
// NumPy; the design: DESIGN.md 4.16.
//
//   fill_count_kernel    a thread per cell: the workgroup's selected cells (bt_fold_counts) into the scan's values, the cells
//                        looked at into the workgroup's count; launch_scan_bases makes the workgroups' bases and the total
//   fill_scatter_kernel  a thread per cell again: the selected cell's rank inside its workgroup from one ballot per wavefront and
//                        the wavefronts' totals in LDS, its flat index to pos[base + rank]; the thread of a cell at or beyond
//                        the total stores UINT64_MAX at its own index.  Every element of pos is stored once.
//   fill_predict_kernel  ONE WAVEFRONT OWNS ONE POSITION.  Its row is V floats at float offset pos * V, aligned to 4 bytes only:
//                        up to three head floats before the first 16-byte boundary and up to three tail floats behind the last
//                        whole quad are one PEEL step (a float a lane), the quads between are 16-byte loads, 64 quads a step, the
//                        next step's quad in flight while this one is looked at.  Pass 1 keeps, per lane, the maximum, a NaN flag
//                        and the count of entries that come before the label's (whose logit one load fetched before the pass),
//                        and across the lanes the running top-k as a sorted list, lane j holding the j-th best: the k-th best is
//                        a wavefront-uniform threshold, a step's four columns are tested against it with one ballot, and only a
//                        hit is broadcast and shifted into the list with __shfl_up.  Pass 2 reads the row again -- it is 32 KB at
//                        V = 8,192 and measured to come from L2 -- for the sum of expf(x - m): four sums a lane, one
//                        per column of the quad, then (a0 + a1) + (a2 + a3) and a butterfly over the lanes, so that a term passes
//                        ceil(V / 256) + 8 additions at most (swt.h states the formula the tolerance of the tests is made of).
// Counts are stored per workgroup and summed by launch_counts_sum; there is no atomic and no scratch.
#include <cmath>

#include "swt_labels.h"

namespace swt {

constexpr uint32_t kFlStep = kBtCols;    // floats of a row one step of a wavefront covers: 64 lanes of one quad
constexpr uint32_t kFlPerBlock = kLbWaves;  // positions of one workgroup: a wavefront each
constexpr uint32_t kFlMaxK = 64;         // lane j holds the j-th best
constexpr uint32_t kFlCounts = 5;
constexpr uint32_t kFlTailLane = 4;      // the peel step: lanes 0 .. 2 hold the head, lanes 4 .. 6 the tail
constexpr unsigned long long kFlNoPos = ~0ull;

// ---- which cells

struct PosArgs {
  const void *ids;
  uint64_t cells;
  long long value;
  uint32_t differ;  // 1: the cells whose id is not the value
  unsigned long long *vals;  // per workgroup: its selected cells, then their exclusive sums; [grid]: the total
  unsigned long long *part;  // per workgroup: the cells it looked at
  unsigned long long *pos;
};

template <class T>
__device__ inline bool fill_selected(const PosArgs &A, uint64_t cell) {
  if (cell >= A.cells) return false;
  return ((long long)static_cast<const T *>(A.ids)[cell] == A.value) != (bool)A.differ;
}

template <class T>
__global__ __launch_bounds__(kLbThreads) void fill_count_kernel(PosArgs A) {
  __shared__ unsigned long long counts[kLbWaves][2];
  const uint64_t cell = (uint64_t)blockIdx.x * kLbThreads + threadIdx.x;
  const uint32_t n[2] = {fill_selected<T>(A, cell), cell < A.cells};
  const unsigned long long sum = bt_fold_counts(n, counts);
  if (threadIdx.x == 0) A.vals[blockIdx.x] = sum;
  if (threadIdx.x == 1) A.part[blockIdx.x] = sum;
}

template <class T>
__global__ __launch_bounds__(kLbThreads) void fill_scatter_kernel(PosArgs A) {
  __shared__ uint32_t wave_n[kLbWaves];
  const uint64_t cell = (uint64_t)blockIdx.x * kLbThreads + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool sel = fill_selected<T>(A, cell);
  const unsigned long long hits = __ballot(sel);
  if (!lane) wave_n[wave] = __popcll(hits);
  __syncthreads();
  if (sel) {
    uint64_t at = A.vals[blockIdx.x] + __popcll(hits & ((1ull << lane) - 1));
    for (uint32_t w = 0; w < wave; w++) at += wave_n[w];
    if (at < A.cells) A.pos[at] = cell;  // always: the ranks of the selected cells are below their number
  }
  if (cell < A.cells && cell >= A.vals[gridDim.x]) A.pos[cell] = kFlNoPos;
}

// ---- one pass over each selected row of logits

struct FillArgs {
  const float *logits;
  const unsigned long long *pos;
  const void *labels;  // null: no label outputs
  uint32_t labels64;
  uint64_t n, cells;
  uint32_t V, k;
  float *lse;
  int32_t *top_id;
  float *top_logit;
  int32_t *label_id;
  float *label_logit;
  int32_t *label_rank;
  unsigned long long *part;  // kFlCounts per workgroup; null: nobody asked for info
};

// (v, id) comes before (w, jd) in the order of the top-k and the rank: the greater logit, then the smaller id.  No NaN on either
// side that is to come first: a NaN v is before nothing.
__device__ inline bool fill_before(float v, int32_t id, float w, int32_t jd) { return v > w || (v == w && id < jd); }

// The sorted list over the lanes (lane j: the j-th best; id -1: an empty slot, all behind the filled ones) and its k-th entry, the
// uniform threshold.
struct FillList {
  float v, thr_v;
  int32_t id, thr_id;
};

// Column j of the step: every lane brings one entry (ok: it exists and is no NaN).  The lanes whose entry passes the threshold
// are served one after the other; an entry that an earlier one of the same ballot has pushed out of reach is dropped.
__device__ inline void fill_offer(FillList &L, uint32_t k, uint32_t lane, float v, int32_t id, bool ok) {
  unsigned long long hits = __ballot(ok && (L.thr_id < 0 || fill_before(v, id, L.thr_v, L.thr_id)));
  while (hits) {  // uniform
    const int src = __ffsll((long long)hits) - 1;
    hits &= hits - 1;
    const float cv = __shfl(v, src, 64);
    const int32_t cid = __shfl(id, src, 64);
    if (!(L.thr_id < 0 || fill_before(cv, cid, L.thr_v, L.thr_id))) continue;
    const uint32_t at = __popcll(__ballot(L.id >= 0 && fill_before(L.v, L.id, cv, cid)));  // the entries that stay in front
    const float up_v = __shfl_up(L.v, 1, 64);
    const int32_t up_id = __shfl_up(L.id, 1, 64);
    if (lane > at) {
      L.v = up_v;
      L.id = up_id;
    } else if (lane == at) {
      L.v = cv;
      L.id = cid;
    }
    L.thr_v = __shfl(L.v, k - 1, 64);
    L.thr_id = __shfl(L.id, k - 1, 64);
  }
}

// What pass 1 keeps in a lane.
struct FillLane {
  float m;        // the greatest entry that is no NaN, -inf without one
  uint32_t nan;   // an entry is a NaN
  uint32_t ahead;  // entries that come before the label's
};

__device__ inline void fill_look(FillLane &S, float v, int32_t id, bool have_label, float lab_v, int32_t lab_id) {
  if (v > S.m) S.m = v;
  S.nan |= !(v == v);
  if (have_label && fill_before(v, id, lab_v, lab_id)) S.ahead++;
}

// The row's geometry: `head` floats up to the first 16-byte boundary (all V where the row ends before it), `quads` whole quads,
// `tail` floats behind them.  peel_id: the entry of this lane in the peel step, -1 without one.
struct FillRow {
  const float *x;
  uint32_t head, quads, tail;
};

__device__ inline FillRow fill_row(const float *x, uint32_t V) {
  FillRow R;
  R.x = x;
  const uint32_t to_boundary = (uint32_t)((16 - (reinterpret_cast<uintptr_t>(x) & 15)) & 15) / 4;
  R.head = to_boundary < V ? to_boundary : V;
  R.quads = (V - R.head) / kBtQuad;
  R.tail = (V - R.head) % kBtQuad;
  return R;
}

__device__ inline int32_t fill_peel_id(const FillRow &R, uint32_t lane) {
  if (lane < R.head) return (int32_t)lane;
  if (lane >= kFlTailLane && lane - kFlTailLane < R.tail) return (int32_t)(R.head + R.quads * kBtQuad + (lane - kFlTailLane));
  return -1;
}

__device__ inline float4 fill_quad(const FillRow &R, uint32_t q) {
  return q < R.quads ? *reinterpret_cast<const float4 *>(R.x + R.head + (uint64_t)q * kBtQuad) : make_float4(0.f, 0.f, 0.f, 0.f);
}

__global__ __launch_bounds__(kLbThreads) void fill_predict_kernel(FillArgs A) {
  __shared__ unsigned long long counts[kLbWaves][kFlCounts];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t p = (uint64_t)blockIdx.x * kFlPerBlock + wave;  // uniform over the wavefront
  const uint32_t V = A.V, k = A.k;
  uint32_t n[kFlCounts] = {0, 0, 0, 0, 0};
  if (p < A.n) {
    const unsigned long long cell = A.pos[p];
    float lse = NAN, lab_v = NAN;
    int32_t lab_id = -1, rank = -1;
    FillList L{NAN, NAN, -1, -1};
    if (cell < A.cells) {
      const FillRow R = fill_row(A.logits + cell * V, V);
      bool range = true;
      if (A.labels) {
        const long long l = A.labels64 ? static_cast<const long long *>(A.labels)[cell] : (long long)static_cast<const int32_t *>(A.labels)[cell];
        range = l >= 0 && l < (long long)V;
        if (range) {
          lab_id = (int32_t)l;
          lab_v = R.x[l];
        }
      }
      const bool have_label = lab_v == lab_v;
      FillLane S{-INFINITY, 0, 0};
      {  // the peel step
        const int32_t id = fill_peel_id(R, lane);
        const float v = id >= 0 ? R.x[id] : -INFINITY;
        if (id >= 0) fill_look(S, v, id, have_label, lab_v, lab_id);
        if (k) fill_offer(L, k, lane, v, id, id >= 0 && v == v);
      }
      float4 next = fill_quad(R, lane);
      for (uint32_t q0 = 0; q0 < R.quads; q0 += 64) {  // uniform
        const uint32_t q = q0 + lane;
        const float4 cur = next;
        next = fill_quad(R, q + 64);
        const bool live = q < R.quads;
        const int32_t id0 = (int32_t)(R.head + q * kBtQuad);
        const float v[kBtQuad] = {cur.x, cur.y, cur.z, cur.w};
        bool hit = false;
#pragma unroll
        for (uint32_t j = 0; j < kBtQuad; j++) {
          if (live) fill_look(S, v[j], id0 + (int32_t)j, have_label, lab_v, lab_id);
          hit |= live && v[j] == v[j] && (L.thr_id < 0 || fill_before(v[j], id0 + (int32_t)j, L.thr_v, L.thr_id));
        }
        if (k && __ballot(hit)) {
#pragma unroll
          for (uint32_t j = 0; j < kBtQuad; j++) fill_offer(L, k, lane, v[j], id0 + (int32_t)j, live && v[j] == v[j]);
        }
      }
      float m = S.m;
      uint32_t ahead = S.ahead;
      for (int d = 32; d; d >>= 1) {
        const float o = __shfl_xor(m, d, 64);
        if (o > m) m = o;
        ahead += __shfl_xor(ahead, d, 64);
      }
      const bool any_nan = __ballot(S.nan) != 0;
      if (have_label) rank = (int32_t)ahead;
      if (any_nan) lse = NAN;
      else if (m == -INFINITY || m == INFINITY) lse = m;
      else if (A.lse) {  // pass 2
        float a[kBtQuad] = {0.f, 0.f, 0.f, 0.f};
        const int32_t id = fill_peel_id(R, lane);
        if (id >= 0) a[0] = expf(__fsub_rn(R.x[id], m));
        float4 nx = fill_quad(R, lane);
        for (uint32_t q0 = 0; q0 < R.quads; q0 += 64) {
          const uint32_t q = q0 + lane;
          const float4 cur = nx;
          nx = fill_quad(R, q + 64);
          if (q < R.quads) {
            a[0] = __fadd_rn(a[0], expf(__fsub_rn(cur.x, m)));
            a[1] = __fadd_rn(a[1], expf(__fsub_rn(cur.y, m)));
            a[2] = __fadd_rn(a[2], expf(__fsub_rn(cur.z, m)));
            a[3] = __fadd_rn(a[3], expf(__fsub_rn(cur.w, m)));
          }
        }
        float s = __fadd_rn(__fadd_rn(a[0], a[1]), __fadd_rn(a[2], a[3]));
        for (int d = 32; d; d >>= 1) s = __fadd_rn(s, __shfl_xor(s, d, 64));
        lse = __fadd_rn(m, logf(s));
      }
      if (!lane) {
        n[1] = rank == 0;
        n[2] = rank >= 0 && (uint32_t)rank < (k ? k : 1u);
        n[3] = any_nan;
        n[4] = !range;
      }
    }
    if (!lane) {
      n[0] = 1;
      if (A.lse) A.lse[p] = lse;
      if (A.label_id) A.label_id[p] = lab_id;
      if (A.label_logit) A.label_logit[p] = lab_v;
      if (A.label_rank) A.label_rank[p] = rank;
    }
    if (lane < k) {
      if (A.top_id) A.top_id[p * k + lane] = L.id;
      if (A.top_logit) A.top_logit[p * k + lane] = L.id >= 0 ? L.v : NAN;
    }
  }
  if (!A.part) return;  // uniform over the launch
  const unsigned long long sum = bt_fold_counts(n, counts);
  if (threadIdx.x < kFlCounts) A.part[(uint64_t)blockIdx.x * kFlCounts + threadIdx.x] = sum;
}

// the workgroups' selected cells and counts between the launches of a call: grow-only and shared by all calls of the process, as
// the workspace of the label calls and under the same rule
static DevBuf g_fill_ws;

static unsigned fl_grid(uint64_t n, uint32_t per) { return (unsigned)((n + per - 1) / per); }

struct PositionsCall {
  const void *ids;
  uint64_t rows;
  uint32_t width;
  uint32_t mode, flags;
  uint64_t *pos, *info;
};

static int positions_check(const PositionsCall &c) {
  if (int rc = lb_check_null({{"ids", c.ids, 0, 4, true, false}, {"out_pos", c.pos, 0, 8, true, true}, {"info", c.info, 0, 8, true, true}}))
    return rc;
  if (int rc = bt_check_shape(c.rows, c.width)) return rc;
  if (c.mode != SWT_FILL_EQUAL && c.mode != SWT_FILL_NOT_EQUAL) return fail(SWT_ERR_INVALID, "mode: SWT_FILL_EQUAL or SWT_FILL_NOT_EQUAL");
  if (c.flags & ~SWT_FILL_IDS64) return fail(SWT_ERR_INVALID, "flags: unknown flag");
  if (c.rows * c.width >> 32) return fail(SWT_ERR_INVALID, "rows * width: 2^32 cells or more");
  const size_t cells = (size_t)c.rows * c.width, id_bytes = (c.flags & SWT_FILL_IDS64) ? 8 : 4;
  return lb_check_layout({{"ids", c.ids, cells * id_bytes, id_bytes, true, false}, {"out_pos", c.pos, cells * 8, 8, true, true},
                          {"info", c.info, 16, 8, true, true}});
}

struct FillCall {
  const float *logits;
  uint64_t rows;
  uint32_t width;
  uint64_t V;
  const uint64_t *pos;
  uint64_t n;
  const void *labels;
  uint32_t flags, k;
  float *lse;
  int32_t *top_id;
  float *top_logit;
  int32_t *label_id;
  float *label_logit;
  int32_t *label_rank;
  uint64_t *info;
};

static int fill_check(const FillCall &c) {
  if (int rc = lb_check_null({{"logits", c.logits, 0, 4, true, false}, {"pos", c.pos, 0, 8, true, false}})) return rc;
  if (int rc = bt_check_shape(c.rows, c.width)) return rc;
  if (c.flags & ~SWT_FILL_IDS64) return fail(SWT_ERR_INVALID, "flags: unknown flag");
  if (!c.V) return fail(SWT_ERR_INVALID, "n_vocab: logits of no entry");
  if (c.V >> 31) return fail(SWT_ERR_INVALID, "n_vocab: 2^31 entries or more");
  if (c.k > kFlMaxK) return fail(SWT_ERR_INVALID, "k is above %u", kFlMaxK);
  if (!c.k && (c.top_id || c.top_logit)) return fail(SWT_ERR_INVALID, "k: out_top_id and out_top_logit are NULL with k == 0");
  if (!c.labels && (c.label_id || c.label_logit || c.label_rank))
    return fail(SWT_ERR_INVALID, "labels: out_label_id, out_label_logit and out_label_rank are NULL without labels");
  const uint64_t all_cells = c.rows * c.width;  // below 2^63: what bt_check_shape let through
  if (all_cells > ((1ull << 62) - 1) / c.V) return fail(SWT_ERR_INVALID, "logits: 2^62 elements or more");
  if (c.n >> 32) return fail(SWT_ERR_INVALID, "n_pos: 2^32 positions or more");
  const size_t cells = (size_t)all_cells, np = (size_t)c.n * 4, id_bytes = (c.flags & SWT_FILL_IDS64) ? 8 : 4;
  return lb_check_layout({{"logits", c.logits, cells * c.V * 4, 4, true, false}, {"pos", c.pos, (size_t)c.n * 8, 8, true, false},
                          {"labels", c.labels, cells * id_bytes, id_bytes, false, false}, {"out_lse", c.lse, np, 4, false, true},
                          {"out_top_id", c.top_id, np * c.k, 4, false, true}, {"out_top_logit", c.top_logit, np * c.k, 4, false, true},
                          {"out_label_id", c.label_id, np, 4, false, true}, {"out_label_logit", c.label_logit, np, 4, false, true},
                          {"out_label_rank", c.label_rank, np, 4, false, true}, {"info", c.info, kFlCounts * 8, 8, false, true}});
}

}  // namespace swt

using namespace swt;

extern "C" {

int swt_fill_capacity(uint32_t *floats_per_step, uint32_t *positions_per_workgroup, uint32_t *k_max, uint32_t *scan_cells) try {
  if (floats_per_step) *floats_per_step = kFlStep;
  if (positions_per_workgroup) *positions_per_workgroup = kFlPerBlock;
  if (k_max) *k_max = kFlMaxK;
  if (scan_cells) *scan_cells = kLbThreads * kBtScanGroup;
  return SWT_OK;
} SWT_API_CATCH

int swt_mlm_positions_dev(const void *d_ids, uint64_t rows, uint32_t width, int64_t value, uint32_t mode, uint32_t flags, uint64_t *d_out_pos,
                          uint64_t *d_info, void *stream) try {
  int rc = positions_check({d_ids, rows, width, mode, flags, d_out_pos, d_info});
  if (rc) return rc;
  if ((rc = ensure_device())) return rc;
  hipStream_t st = (hipStream_t)stream;
  SWT_HIP(hipMemsetAsync(d_info, 0, 16, st));
  const uint64_t cells = rows * width;
  if (!cells) return SWT_OK;
  const unsigned grid = fl_grid(cells, kLbThreads);
  const size_t val_bytes = lb_round(((size_t)grid + 1) * 8);
  if ((rc = g_batch_ws.reserve(grid))) return rc;
  if ((rc = g_fill_ws.reserve(val_bytes + (size_t)grid * 8))) return rc;
  PosArgs A{d_ids, cells, (long long)value, mode == SWT_FILL_NOT_EQUAL, g_fill_ws.as<unsigned long long>(),
            reinterpret_cast<unsigned long long *>(g_fill_ws.as<uint8_t>() + val_bytes), reinterpret_cast<unsigned long long *>(d_out_pos)};
  const bool ids64 = flags & SWT_FILL_IDS64;
  if (ids64) hipLaunchKernelGGL(fill_count_kernel<int64_t>, dim3(grid), dim3(kLbThreads), 0, st, A);
  else hipLaunchKernelGGL(fill_count_kernel<int32_t>, dim3(grid), dim3(kLbThreads), 0, st, A);
  launch_scan_bases(grid, A.vals, d_info, st);
  if (ids64) hipLaunchKernelGGL(fill_scatter_kernel<int64_t>, dim3(grid), dim3(kLbThreads), 0, st, A);
  else hipLaunchKernelGGL(fill_scatter_kernel<int32_t>, dim3(grid), dim3(kLbThreads), 0, st, A);
  launch_counts_sum(A.part, grid, 1, reinterpret_cast<unsigned long long *>(d_info) + 1, st);
  SWT_HIP(hipGetLastError());
  return SWT_OK;
} SWT_API_CATCH

int swt_mlm_positions(const void *ids, uint64_t rows, uint32_t width, int64_t value, uint32_t mode, uint32_t flags, uint64_t *out_pos,
                      uint64_t *info) try {
  int rc = positions_check({ids, rows, width, mode, flags, out_pos, info});
  if (rc) return rc;
  info[0] = info[1] = 0;
  const size_t cells = (size_t)rows * width;
  if (!cells) return SWT_OK;
  if ((rc = ensure_device())) return rc;
  BatchStage s;
  const void *d_ids = s.in(static_cast<const uint8_t *>(ids), cells * ((flags & SWT_FILL_IDS64) ? 8 : 4));
  uint64_t *d_pos = s.out(out_pos, cells * 8), *d_info = s.out(info, 16);
  if (s.rc) return s.rc;
  if ((rc = swt_mlm_positions_dev(d_ids, rows, width, value, mode, flags, d_pos, d_info, nullptr))) return rc;
  return s.fetch();
} SWT_API_CATCH

int swt_mlm_predict_dev(const float *d_logits, uint64_t rows, uint32_t width, uint64_t n_vocab, const uint64_t *d_pos, uint64_t n_pos,
                        const void *d_labels, uint32_t flags, uint32_t k, float *d_out_lse, int32_t *d_out_top_id, float *d_out_top_logit,
                        int32_t *d_out_label_id, float *d_out_label_logit, int32_t *d_out_label_rank, uint64_t *d_info, void *stream) try {
  int rc = fill_check({d_logits, rows, width, n_vocab, d_pos, n_pos, d_labels, flags, k, d_out_lse, d_out_top_id, d_out_top_logit,
                       d_out_label_id, d_out_label_logit, d_out_label_rank, d_info});
  if (rc) return rc;
  if ((rc = ensure_device())) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (d_info) SWT_HIP(hipMemsetAsync(d_info, 0, kFlCounts * 8, st));
  if (!n_pos) return SWT_OK;
  FillArgs A{d_logits, reinterpret_cast<const unsigned long long *>(d_pos), d_labels, (flags & SWT_FILL_IDS64) ? 1u : 0u, n_pos, rows * width,
             (uint32_t)n_vocab, k, d_out_lse, d_out_top_id, d_out_top_logit, d_out_label_id, d_out_label_logit, d_out_label_rank, nullptr};
  const unsigned grid = fl_grid(n_pos, kFlPerBlock);
  if (d_info) {
    if ((rc = g_fill_ws.reserve((size_t)grid * kFlCounts * 8))) return rc;
    A.part = g_fill_ws.as<unsigned long long>();
  }
  prof_begin(st);
  hipLaunchKernelGGL(fill_predict_kernel, dim3(grid), dim3(kLbThreads), 0, st, A);
  prof_end(st);
  if (d_info) launch_counts_sum(A.part, grid, kFlCounts, reinterpret_cast<unsigned long long *>(d_info), st);
  SWT_HIP(hipGetLastError());
  return SWT_OK;
} SWT_API_CATCH

int swt_mlm_predict(const float *logits, uint64_t rows, uint32_t width, uint64_t n_vocab, const uint64_t *pos, uint64_t n_pos, const void *labels,
                    uint32_t flags, uint32_t k, float *out_lse, int32_t *out_top_id, float *out_top_logit, int32_t *out_label_id,
                    float *out_label_logit, int32_t *out_label_rank, uint64_t *info) try {
  int rc = fill_check({logits, rows, width, n_vocab, pos, n_pos, labels, flags, k, out_lse, out_top_id, out_top_logit, out_label_id,
                       out_label_logit, out_label_rank, info});
  if (rc) return rc;
  const size_t cells = (size_t)rows * width;
  for (uint64_t p = 0; p < n_pos; p++)
    if (pos[p] >= cells) return fail(SWT_ERR_INVALID, "pos: position %llu is no cell of the rows", (unsigned long long)p);
  if (info)
    for (uint32_t i = 0; i < kFlCounts; i++) info[i] = 0;
  if (!n_pos) return SWT_OK;
  if ((rc = ensure_device())) return rc;
  const size_t np = (size_t)n_pos * 4;
  BatchStage s;
  const float *d_logits = s.in(logits, cells * n_vocab * 4);
  const uint64_t *d_pos = s.in(pos, (size_t)n_pos * 8);
  const void *d_labels = s.in(static_cast<const uint8_t *>(labels), cells * ((flags & SWT_FILL_IDS64) ? 8 : 4));
  float *d_lse = s.out(out_lse, np), *d_tl = s.out(out_top_logit, np * k), *d_ll = s.out(out_label_logit, np);
  int32_t *d_ti = s.out(out_top_id, np * k), *d_li = s.out(out_label_id, np), *d_lr = s.out(out_label_rank, np);
  uint64_t *d_info = s.out(info, kFlCounts * 8);
  if (s.rc) return s.rc;
  if ((rc = swt_mlm_predict_dev(d_logits, rows, width, n_vocab, d_pos, n_pos, d_labels, flags, k, d_lse, d_ti, d_tl, d_li, d_ll, d_lr, d_info,
                                nullptr)))
    return rc;
  return s.fetch();
} SWT_API_CATCH

}  // extern "C"
