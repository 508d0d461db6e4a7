// swt_mlm.hip -- masked-LM batches on the device: over finished rows of dense ids (any input_ids of the batch calls), which
// columns the objective selects, what stands in their place and the labels.  Semantics: include/swt.h; tests/mlm_cases.py holds
// them in NumPy; the design and its measurements: DESIGN.md 4.12.
//
// mlm_kernel<T>: ROW-major -- a group of g lanes per row (swt_rows.h), so that narrow rows share a wavefront; a row wider than
// 4 g columns takes several steps.  A step:
//   load    the lane's quad (bt_load_quad when the width is a multiple of four and the pointers are aligned; else column by
//           column)
//   class   from cls_tab, an id outside [0, n_class) is class 2
//   heads   a column is a head by its class and its left neighbour's -- the quad's first column asks the lane to its left, the
//           group's first lane the carry of the step before.  "head ? column : none" is max-scanned inside the quad, then over
//           the lanes of the group (__shfl_up, a lane taking nothing from below its group), then joined with the carry: the
//           last head of the steps before
//   draws   Philox4x32-10 at (head, row) decides the word, at (column, row) what a selected column becomes; consecutive columns
//           of one word share the head's draw, a head's own draw is its head's, and nothing is drawn for class 2
//   stores  ids, labels, selected
// The loop over the steps and the sets is uniform over the wavefront (the width and the sets are the launch's), a row beyond
// `rows` is masked, not skipped: every lane meets every shuffle.  The five counts are stored per workgroup; launch_counts_sum
// sums them into info.
#include "swt_batch.h"
#include "swt_philox.h"

namespace swt {

constexpr int kMlThreads = 256;
constexpr int kMlWaves = kMlThreads / 64;
constexpr uint32_t kMlFlags = SWT_MLM_WHOLE_WORD | SWT_MLM_IDS64;
constexpr uint32_t kMlCounts = 5;
constexpr int32_t kMlNoHead = -1;

// (Philox, philox4x32_10: swt_philox.h, which the BPE-dropout draws share)

struct MlmArgs {
  const void *ids;
  uint64_t rows;
  uint32_t width;
  const uint8_t *cls_tab;
  uint32_t n_class;
  const uint32_t *rand_ids;
  uint32_t n_rand;
  uint32_t key0, key1, epoch, whole_word, mask_id;
  unsigned long long select_below, mask_below, random_below;
  void *out_ids, *out_labels;
  uint8_t *out_selected;
  unsigned long long *part;  // the counts of every workgroup, kMlCounts each; null: nobody asked for info
  int vec;         // every array takes the wide loads and stores: the width is a multiple of four and the pointers are aligned
  uint32_t group;  // lanes per row: a power of two, 1 .. 64
  uint32_t sets;   // sets of rows a wavefront walks
};

template <class T> __device__ inline void ml_store_quad(T *p, const T (&v)[kBtQuad]);
template <> __device__ inline void ml_store_quad<int32_t>(int32_t *p, const int32_t (&v)[kBtQuad]) {
  *reinterpret_cast<int4 *>(p) = make_int4(v[0], v[1], v[2], v[3]);
}
template <> __device__ inline void ml_store_quad<int64_t>(int64_t *p, const int64_t (&v)[kBtQuad]) {
  reinterpret_cast<longlong2 *>(p)[0] = make_longlong2(v[0], v[1]);
  reinterpret_cast<longlong2 *>(p)[1] = make_longlong2(v[2], v[3]);
}

template <class T>
__global__ __launch_bounds__(kMlThreads) void mlm_kernel(MlmArgs A) {
  __shared__ unsigned long long counts[kMlWaves][kMlCounts];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t g = A.group, sub = lane & (g - 1), per_wave = 64 / g;
  const uint32_t group_last = lane | (g - 1);  // the last lane of this lane's group
  const T *ids = reinterpret_cast<const T *>(A.ids);
  T *out_ids = reinterpret_cast<T *>(A.out_ids), *out_labels = reinterpret_cast<T *>(A.out_labels);
  uint32_t n[kMlCounts] = {0, 0, 0, 0, 0};  // eligible, selected, masked, random, kept
  const uint64_t b0 = ((uint64_t)blockIdx.x * kMlWaves + wave) * per_wave * A.sets + lane / g;
  for (uint32_t it = 0; it < A.sets; it++) {
    const uint64_t b = b0 + (uint64_t)it * per_wave;
    const bool live = b < A.rows;
    const uint64_t at = live ? b * A.width : 0;
    int32_t carry_head = kMlNoHead;  // the last head of the steps before
    uint32_t carry_cls = 2;          // the class of the last column of the step before; none: as class 2
    // uniform over the wavefront: a row's columns past the width, and the rows past the last, are class 2 and store nothing.
    // A column is below 2^31 (mlm_check), so kMlNoHead lies below every head
    for (uint64_t base = 0; base < A.width; base += (uint64_t)g * kBtQuad) {
      const uint64_t c0 = base + (uint64_t)sub * kBtQuad;
      const bool whole = live && c0 + kBtQuad <= A.width;
      T v[kBtQuad];
      uint32_t cls[kBtQuad];
      if (A.vec) {
        if (whole) bt_load_quad<T>(ids + at + c0, v);
      } else {
#pragma unroll
        for (uint32_t j = 0; j < kBtQuad; j++)
          if (live && c0 + j < A.width) v[j] = ids[at + c0 + j];
      }
#pragma unroll
      for (uint32_t j = 0; j < kBtQuad; j++) {
        cls[j] = 2;
        if (!live || c0 + j >= A.width) { v[j] = 0; continue; }
        const int64_t id = (int64_t)v[j];
        if (id >= 0 && id < (int64_t)A.n_class) cls[j] = A.cls_tab[id];
        if (cls[j] > 2) cls[j] = 2;
      }
      // the class to the left of the quad: the lane before, and for the group's first lane the step before
      const uint32_t before = __shfl_up(cls[kBtQuad - 1], 1, 64);
      const uint32_t left = sub ? before : carry_cls;
      int32_t h[kBtQuad];
#pragma unroll
      for (uint32_t j = 0; j < kBtQuad; j++) {
        const uint32_t l = j ? cls[j - 1] : left;
        const bool head = A.whole_word ? cls[j] == 0 || (cls[j] == 1 && l == 2) : cls[j] < 2;
        h[j] = head ? (int32_t)(uint32_t)(c0 + j) : (j ? h[j - 1] : kMlNoHead);
      }
      // the last head up to and including each lane's quad, over the lanes of the group
      int32_t run = h[kBtQuad - 1];
      for (uint32_t d = 1; d < g; d <<= 1) {
        const int32_t o = __shfl_up(run, d, 64);
        if (sub >= d && o > run) run = o;
      }
      int32_t prev = __shfl_up(run, 1, 64);
      if (!sub || prev < carry_head) prev = carry_head;  // heads of earlier steps lie below every column of this one
      const int32_t step_head = __shfl(run, group_last, 64);
      carry_cls = __shfl(cls[kBtQuad - 1], group_last, 64);
      if (step_head > carry_head) carry_head = step_head;

      T lab[kBtQuad];
      uint32_t sel = 0;
      int32_t drawn = kMlNoHead;  // the head whose draw `word` holds
      bool word = false;
#pragma unroll
      for (uint32_t j = 0; j < kBtQuad; j++) {
        lab[j] = (T)-100;
        if (cls[j] >= 2) continue;
        n[0]++;
        const uint32_t c = (uint32_t)(c0 + j);
        Philox own;
        const int32_t head = h[j] != kMlNoHead ? h[j] : prev;
        bool have_own = false;
        if (head != drawn) {
          own = philox4x32_10((uint32_t)head, (uint32_t)b, A.epoch, 0, A.key0, A.key1);
          have_own = (uint32_t)head == c;
          word = own.x[0] < A.select_below;
          drawn = head;
        }
        if (!word) continue;
        if (!have_own) own = philox4x32_10(c, (uint32_t)b, A.epoch, 0, A.key0, A.key1);
        n[1]++;
        sel |= 1u << (8 * j);
        lab[j] = v[j];
        if (own.x[1] < A.mask_below) {
          v[j] = (T)A.mask_id; n[2]++;
        } else if (own.x[1] < A.random_below) {
          v[j] = (T)A.rand_ids[(uint32_t)(((uint64_t)own.x[2] * A.n_rand) >> 32)]; n[3]++;
        } else {
          n[4]++;
        }
      }
      if (A.vec) {
        if (whole) {
          ml_store_quad<T>(out_ids + at + c0, v);
          ml_store_quad<T>(out_labels + at + c0, lab);
          if (A.out_selected) *reinterpret_cast<uint32_t *>(A.out_selected + at + c0) = sel;
        }
      } else {
#pragma unroll
        for (uint32_t j = 0; j < kBtQuad; j++) {
          if (!live || c0 + j >= A.width) continue;
          out_ids[at + c0 + j] = v[j];
          out_labels[at + c0 + j] = lab[j];
          if (A.out_selected) A.out_selected[at + c0 + j] = (uint8_t)((sel >> (8 * j)) & 1u);
        }
      }
    }
  }
  if (!A.part) return;  // uniform over the workgroup
  const unsigned long long sum = bt_fold_counts(n, counts);
  if (threadIdx.x < kMlCounts) A.part[(uint64_t)blockIdx.x * kMlCounts + threadIdx.x] = sum;
}

// the workgroups' counts between the two launches: grow-only and shared by all calls of the process (the calls carry no
// handle), as the scan workspace of the plans and under the same rule
static DevBuf g_mlm_ws;

// the byte ranges [a, a + na) and [b, b + nb) share a byte
static bool ml_overlap(const void *a, size_t na, const void *b, size_t nb) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return a && b && na && nb && x < y + nb && y < x + na;
}

// What both forms refuse, from the arguments alone.
static int mlm_check(const void *ids, uint64_t rows, uint32_t width, const uint8_t *cls_tab, const uint32_t *rand_ids, uint32_t n_rand,
                     const swt_mlm_spec *spec, const void *out_ids, const void *out_labels, const uint8_t *out_selected) {
  if (!spec) return fail(SWT_ERR_INVALID, "null argument: spec");
  if (!ids) return fail(SWT_ERR_INVALID, "null argument: ids");
  if (!out_ids) return fail(SWT_ERR_INVALID, "null argument: out_ids");
  if (!out_labels) return fail(SWT_ERR_INVALID, "null argument: out_labels");
  if (!cls_tab) return fail(SWT_ERR_INVALID, "null argument: cls_tab");
  if (int rc = bt_check_shape(rows, width)) return rc;
  if (spec->flags & ~kMlFlags) return fail(SWT_ERR_INVALID, "flags: unknown flag");
  const uint64_t one = 1ull << 32;
  if (spec->select_below > one) return fail(SWT_ERR_INVALID, "select_below is above 2^32");
  if (spec->mask_below > one) return fail(SWT_ERR_INVALID, "mask_below is above 2^32");
  if (spec->random_below > one) return fail(SWT_ERR_INVALID, "random_below is above 2^32");
  if (spec->mask_below > spec->random_below) return fail(SWT_ERR_INVALID, "mask_below is above random_below");
  if (!spec->n_class) return fail(SWT_ERR_INVALID, "n_class: a class table of no entry");
  if (spec->mask_below != spec->random_below) {
    if (!rand_ids) return fail(SWT_ERR_INVALID, "null argument: rand_ids, with a share of random replacements");
    if (!n_rand) return fail(SWT_ERR_INVALID, "n_rand: no id to draw a random replacement from");
  }
  const size_t id_bytes = (spec->flags & SWT_MLM_IDS64) ? 8 : 4, cells = (size_t)rows * width;
  if (ml_overlap(ids, cells * id_bytes, out_ids, cells * id_bytes)) return fail(SWT_ERR_INVALID, "out_ids overlaps ids: not in place");
  if (ml_overlap(ids, cells * id_bytes, out_labels, cells * id_bytes)) return fail(SWT_ERR_INVALID, "out_labels overlaps ids: not in place");
  if (ml_overlap(ids, cells * id_bytes, out_selected, cells)) return fail(SWT_ERR_INVALID, "out_selected overlaps ids: not in place");
  return SWT_OK;
}

}  // namespace swt

using namespace swt;

extern "C" {

int swt_mlm_capacity(uint32_t *cols_per_step, uint32_t *rows_per_wave_max) try {
  if (cols_per_step) *cols_per_step = kBtCols;
  if (rows_per_wave_max) *rows_per_wave_max = 64;
  return SWT_OK;
} SWT_API_CATCH

int swt_mlm_mask_dev(const void *d_ids, uint64_t rows, uint32_t width, const uint8_t *d_cls_tab, const uint32_t *d_rand_ids, uint32_t n_rand,
                     const swt_mlm_spec *spec, void *d_out_ids, void *d_out_labels, uint8_t *d_out_selected, uint64_t *d_info,
                     void *stream) try {
  int rc = mlm_check(d_ids, rows, width, d_cls_tab, d_rand_ids, n_rand, spec, d_out_ids, d_out_labels, d_out_selected);
  if (rc) return rc;
  const uintptr_t id_bytes = (spec->flags & SWT_MLM_IDS64) ? 8 : 4;
  if (!bt_aligned(id_bytes, {d_ids, d_out_ids, d_out_labels}) || !bt_aligned(4, {d_rand_ids}) || !bt_aligned(8, {d_info}))
    return fail(SWT_ERR_INVALID, "an array is not aligned to its element type");
  if ((rc = ensure_device())) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (!rows) {
    if (d_info) SWT_HIP(hipMemsetAsync(d_info, 0, kMlCounts * 8, st));
    return SWT_OK;
  }
  MlmArgs A{d_ids, rows, width, d_cls_tab, spec->n_class, d_rand_ids, n_rand, (uint32_t)spec->seed, (uint32_t)(spec->seed >> 32), spec->epoch,
            (spec->flags & SWT_MLM_WHOLE_WORD) ? 1u : 0u, spec->mask_id, spec->select_below, spec->mask_below, spec->random_below,
            d_out_ids, d_out_labels, d_out_selected, nullptr, 0, 1, 1};
  A.vec = width % kBtQuad == 0 && bt_aligned(16, {d_ids, d_out_ids, d_out_labels}) && bt_aligned(4, {d_out_selected});
  A.group = bt_group(width);
  const RowShape shape = bt_shape(rows, A.group, kMlWaves);
  A.sets = (uint32_t)shape.sets;
  const unsigned grid = shape.grid;
  if (d_info) {
    if ((rc = g_mlm_ws.reserve((size_t)grid * kMlCounts * 8))) return rc;
    A.part = g_mlm_ws.as<unsigned long long>();
  }
  prof_begin(st);
  if (spec->flags & SWT_MLM_IDS64) hipLaunchKernelGGL(mlm_kernel<int64_t>, dim3(grid), dim3(kMlThreads), 0, st, A);
  else hipLaunchKernelGGL(mlm_kernel<int32_t>, dim3(grid), dim3(kMlThreads), 0, st, A);
  prof_end(st);
  if (d_info) launch_counts_sum(A.part, grid, kMlCounts, reinterpret_cast<unsigned long long *>(d_info), st);
  SWT_HIP(hipGetLastError());
  return SWT_OK;
} SWT_API_CATCH

int swt_mlm_mask(const void *ids, uint64_t rows, uint32_t width, const uint8_t *cls_tab, const uint32_t *rand_ids, uint32_t n_rand,
                 const swt_mlm_spec *spec, void *out_ids, void *out_labels, uint8_t *out_selected, uint64_t *info) try {
  int rc = mlm_check(ids, rows, width, cls_tab, rand_ids, n_rand, spec, out_ids, out_labels, out_selected);
  if (rc) return rc;
  if (info)
    for (uint32_t k = 0; k < kMlCounts; k++) info[k] = 0;
  if (!rows) return SWT_OK;
  if ((rc = ensure_device())) return rc;
  const size_t id_bytes = (spec->flags & SWT_MLM_IDS64) ? 8 : 4, cells = (size_t)rows * width;
  BatchStage s;
  const void *d_ids = s.in(static_cast<const uint8_t *>(ids), cells * id_bytes);
  const uint8_t *d_cls = s.in(cls_tab, spec->n_class);
  const uint32_t *d_rand = spec->mask_below != spec->random_below ? s.in(rand_ids, (size_t)n_rand * 4) : nullptr;
  void *d_out = s.out(static_cast<uint8_t *>(out_ids), cells * id_bytes), *d_lab = s.out(static_cast<uint8_t *>(out_labels), cells * id_bytes);
  uint8_t *d_sel = s.out(out_selected, cells);
  uint64_t *d_info = s.out(info, kMlCounts * 8);
  if (s.rc) return s.rc;
  if ((rc = swt_mlm_mask_dev(d_ids, rows, width, d_cls, d_rand, n_rand, spec, d_out, d_lab, d_sel, d_info, nullptr))) return rc;
  return s.fetch();
} SWT_API_CATCH

}  // extern "C"
