// swt_denoise.hip -- span-corruption batches on the device: over finished rows of dense ids, the span noise of SpanBERT (masked in
// place), T5 (every run of noise one sentinel in the row, the runs listed behind their sentinels in the labels) and BART (every
// run one [MASK]).  Semantics: include/swt.h; tests/denoise_cases.py holds them in plain Python; the design: DESIGN.md 4.19.
//
// denoise_kernel<T, kRows>: ROW-major as mlm_kernel -- a group of g lanes per row (swt_rows.h), a quad of four columns per lane
// and step, a row wider than 4 g columns in several steps.  kRows = false is the plan: the same walk, counts only.  A step:
//   load    the lane's quad, its classes and heads (as mlm_kernel)
//   units   an add-scan of the heads: the unit of a column is the number of heads up to it, less one
//   reach   Philox4x32-10 at (head, row, epoch, 1) says whether the unit starts a span and how long it is; "unit + length" of
//           the starts is max-scanned: a column is noise when the reach before or at it lies above its unit
//   runs    a noise column whose left neighbour is none starts a run; an add-scan of the run starts numbers the runs, and a run
//           past the sentinels (SENTINEL mode) is given back
//   places  an add-scan of "columns that stay + run starts" (the row) and of "noise columns + run starts" (the labels), both in
//           one 32-bit word: a step makes at most 4 g and 8 g of them
//   stores  MASK mode stores quads as mlm_kernel does.  The other two stage the step's ids in LDS at "place - first place of
//           the step" and the group stores the range, consecutive lanes on consecutive elements: at most 4 g ids of the row
//           and 8 g of the labels
// Every scan runs inside the quad, then over the lanes of the group (__shfl_up, a lane taking nothing from below its group), then
// joins the carry of the steps before: units, reach, whether the last column was noise, runs, both places.  The loops over the
// steps and the sets are uniform over the wavefront, a row beyond `rows` is masked, not skipped: every lane meets every shuffle.
// Behind a row's last step the group fills the tail (pad_id, mask 0, -100) and sets the closing sentinel.  The five counts and
// two maxima are stored per workgroup; info_kernel joins them.
#include "swt_batch.h"
#include "swt_philox.h"

namespace swt {

constexpr int kDnThreads = 256;
constexpr int kDnWaves = kDnThreads / 64;
constexpr uint32_t kDnFlags = SWT_DENOISE_WHOLE_WORD | SWT_DENOISE_IDS64;
constexpr uint32_t kDnSums = 5, kDnCounts = 7;  // info: five sums, then two maxima
constexpr uint32_t kDnLenMax = 31;
constexpr uint32_t kDnNoCap = 0xFFFFFFFFu;

struct DenoiseArgs {
  const void *ids;
  uint64_t rows;
  uint32_t width;
  const uint8_t *cls_tab;
  uint32_t n_class;
  const uint32_t *sentinel_ids;
  uint32_t key0, key1, epoch, whole_word, mode, mask_id, pad_id, n_len;
  uint32_t cap;  // the runs that stay noise: n_sentinel - 1 in SENTINEL mode, else all
  uint32_t label_width;
  unsigned long long start_below;
  unsigned long long len_below[kDnLenMax];
  void *out_ids, *out_labels;
  uint8_t *out_mask;
  uint32_t *out_len, *out_label_len;
  unsigned long long *part;  // the counts of every workgroup, kDnCounts each; null: nobody asked for info
  int vec_in, vec_out;  // the wide loads of ids; the wide stores of MASK mode
  uint32_t group;       // lanes per row: a power of two, 1 .. 64
  uint32_t sets;        // sets of rows a wavefront walks
};

template <class T> __device__ inline void dn_store_quad(T *p, const T (&v)[kBtQuad]);
template <> __device__ inline void dn_store_quad<int32_t>(int32_t *p, const int32_t (&v)[kBtQuad]) {
  *reinterpret_cast<int4 *>(p) = make_int4(v[0], v[1], v[2], v[3]);
}
template <> __device__ inline void dn_store_quad<int64_t>(int64_t *p, const int64_t (&v)[kBtQuad]) {
  reinterpret_cast<longlong2 *>(p)[0] = make_longlong2(v[0], v[1]);
  reinterpret_cast<longlong2 *>(p)[1] = make_longlong2(v[2], v[3]);
}

// the inclusive scan of x over the lanes of a group: a lane takes nothing from below its group
__device__ inline uint32_t dn_scan_add(uint32_t x, uint32_t sub, uint32_t g) {
  for (uint32_t d = 1; d < g; d <<= 1) {
    const uint32_t o = __shfl_up(x, d, 64);
    if (sub >= d) x += o;
  }
  return x;
}
__device__ inline uint32_t dn_scan_max(uint32_t x, uint32_t sub, uint32_t g) {
  for (uint32_t d = 1; d < g; d <<= 1) {
    const uint32_t o = __shfl_up(x, d, 64);
    if (sub >= d && o > x) x = o;
  }
  return x;
}

// what the lanes of a wavefront wrote to LDS, the others may read behind this
__device__ inline void dn_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <class T, bool kRows>
__global__ __launch_bounds__(kDnThreads) void denoise_kernel(DenoiseArgs A) {
  __shared__ unsigned long long counts[kDnWaves][kDnSums];
  __shared__ uint32_t most[kDnWaves][kDnCounts - kDnSums];
  // the stage of a wavefront: a group's 4 g ids of the row start at four times its first lane, its 8 g of the labels at eight times
  __shared__ T stage_ids[kRows ? kDnWaves * kBtCols : 1];
  __shared__ T stage_lab[kRows ? kDnWaves * 2 * kBtCols : 1];
  __shared__ uint8_t stage_mask[kRows ? kDnWaves * kBtCols : 4];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t g = A.group, sub = lane & (g - 1), per_wave = 64 / g;
  const uint32_t group_last = lane | (g - 1);  // the last lane of this lane's group
  const bool squeeze = A.mode != SWT_DENOISE_MASK, sentinel = A.mode == SWT_DENOISE_SENTINEL;
  const T *ids = reinterpret_cast<const T *>(A.ids);
  T *out_ids = reinterpret_cast<T *>(A.out_ids), *out_labels = reinterpret_cast<T *>(A.out_labels);
  T *sid = stage_ids + (kRows ? wave * kBtCols + (lane - sub) * kBtQuad : 0);
  T *slab = stage_lab + (kRows ? wave * 2 * kBtCols + (lane - sub) * 2 * kBtQuad : 0);
  uint8_t *smask = stage_mask + (kRows ? wave * kBtCols + (lane - sub) * kBtQuad : 0);
  uint32_t n[kDnSums] = {0, 0, 0, 0, 0};  // eligible, noise, runs, runs given back, rows cut
  uint32_t most_len = 0, most_lab = 0;
  const uint64_t b0 = ((uint64_t)blockIdx.x * kDnWaves + wave) * per_wave * A.sets + lane / g;
  for (uint32_t it = 0; it < A.sets; it++) {
    const uint64_t b = b0 + (uint64_t)it * per_wave;
    const bool live = b < A.rows;
    const uint64_t at = live ? b * A.width : 0;
    // the carries of the steps before: the class and the noise of the last column, units, reach, runs, both places
    uint32_t carry_cls = 2, carry_noise = 0, carry_units = 0, carry_reach = 0, carry_runs = 0, carry_o = 0, carry_l = 0;
    for (uint64_t base = 0; base < A.width; base += (uint64_t)g * kBtQuad) {
      const uint64_t c0 = base + (uint64_t)sub * kBtQuad;
      const bool whole = live && c0 + kBtQuad <= A.width;
      T v[kBtQuad];
      uint32_t cls[kBtQuad];
      bool in[kBtQuad];
      if (A.vec_in) {
        if (whole) bt_load_quad<T>(ids + at + c0, v);
      } else {
#pragma unroll
        for (uint32_t j = 0; j < kBtQuad; j++)
          if (live && c0 + j < A.width) v[j] = ids[at + c0 + j];
      }
#pragma unroll
      for (uint32_t j = 0; j < kBtQuad; j++) {
        cls[j] = 2;
        in[j] = live && c0 + j < A.width;
        if (!in[j]) { v[j] = 0; continue; }
        const int64_t id = (int64_t)v[j];
        if (id >= 0 && id < (int64_t)A.n_class) cls[j] = A.cls_tab[id];
        if (cls[j] > 2) cls[j] = 2;
      }
      const uint32_t before = __shfl_up(cls[kBtQuad - 1], 1, 64);
      const uint32_t left = sub ? before : carry_cls;
      carry_cls = __shfl(cls[kBtQuad - 1], group_last, 64);

      // units: the heads up to and including each column
      bool hd[kBtQuad];
      uint32_t hq[kBtQuad];
#pragma unroll
      for (uint32_t j = 0; j < kBtQuad; j++) {
        const uint32_t l = j ? cls[j - 1] : left;
        hd[j] = A.whole_word ? cls[j] == 0 || (cls[j] == 1 && l == 2) : cls[j] < 2;
        hq[j] = (j ? hq[j - 1] : 0) + (hd[j] ? 1u : 0u);
      }
      const uint32_t hs = dn_scan_add(hq[kBtQuad - 1], sub, g);
      uint32_t h_before = __shfl_up(hs, 1, 64);
      h_before = (sub ? h_before : 0) + carry_units;
      carry_units += __shfl(hs, group_last, 64);

      // reach: the greatest "unit + length" over the starts up to and including each column; 0: none
      uint32_t rq[kBtQuad];
#pragma unroll
      for (uint32_t j = 0; j < kBtQuad; j++) {
        uint32_t r = 0;
        if (hd[j]) {
          const Philox x = philox4x32_10((uint32_t)(c0 + j), (uint32_t)b, A.epoch, 1, A.key0, A.key1);
          if (x.x[0] < A.start_below) {
            r = h_before + hq[j];  // unit + 1
            for (uint32_t k = 0; k < A.n_len; k++) r += x.x[1] >= A.len_below[k] ? 1u : 0u;
          }
        }
        rq[j] = j && rq[j - 1] > r ? rq[j - 1] : r;
      }
      const uint32_t rs = dn_scan_max(rq[kBtQuad - 1], sub, g);
      uint32_t r_before = __shfl_up(rs, 1, 64);
      if (!sub || r_before < carry_reach) r_before = carry_reach;
      const uint32_t step_reach = __shfl(rs, group_last, 64);
      if (step_reach > carry_reach) carry_reach = step_reach;

      // noise, and the run starts up to and including each column
      bool nz[kBtQuad], st[kBtQuad];
      uint32_t kq[kBtQuad];
#pragma unroll
      for (uint32_t j = 0; j < kBtQuad; j++) {
        const uint32_t reach = rq[j] > r_before ? rq[j] : r_before;
        nz[j] = cls[j] < 2 && reach > h_before + hq[j] - 1;
      }
      const uint32_t noise_before = __shfl_up((uint32_t)nz[kBtQuad - 1], 1, 64);
      const bool left_noise = sub ? noise_before != 0 : carry_noise != 0;
      carry_noise = __shfl((uint32_t)nz[kBtQuad - 1], group_last, 64);
#pragma unroll
      for (uint32_t j = 0; j < kBtQuad; j++) {
        st[j] = nz[j] && !(j ? nz[j - 1] : left_noise);
        kq[j] = (j ? kq[j - 1] : 0) + (st[j] ? 1u : 0u);
      }
      const uint32_t ks = dn_scan_add(kq[kBtQuad - 1], sub, g);
      uint32_t k_before = __shfl_up(ks, 1, 64);
      k_before = (sub ? k_before : 0) + carry_runs;
      carry_runs += __shfl(ks, group_last, 64);

      // a run past the cap is given back; the places of what the row and the labels take, the labels' in the high half
      uint32_t run[kBtQuad], pq[kBtQuad];
#pragma unroll
      for (uint32_t j = 0; j < kBtQuad; j++) {
        run[j] = k_before + kq[j] - 1;  // of a noise column: the number of its run
        if (cls[j] < 2) n[0]++;
        if (st[j]) n[2]++;
        if (st[j] && run[j] >= A.cap) n[3]++;
        if (nz[j] && run[j] >= A.cap) nz[j] = st[j] = false;
        if (nz[j]) n[1]++;
        const uint32_t row_takes = in[j] && (!squeeze || !nz[j] || st[j]) ? 1u : 0u;
        const uint32_t lab_takes = sentinel ? (nz[j] ? 1u : 0u) + (st[j] ? 1u : 0u) : 0u;
        pq[j] = (j ? pq[j - 1] : 0) + (row_takes | lab_takes << 16);
      }
      const uint32_t ps = dn_scan_add(pq[kBtQuad - 1], sub, g);
      uint32_t p_before = __shfl_up(ps, 1, 64);
      if (!sub) p_before = 0;
      const uint32_t step_places = __shfl(ps, group_last, 64);
      const uint32_t step_o = step_places & 0xFFFFu, step_l = step_places >> 16;

      if (kRows && !squeeze) {
        T lab[kBtQuad];
#pragma unroll
        for (uint32_t j = 0; j < kBtQuad; j++) {
          lab[j] = nz[j] ? v[j] : (T)-100;
          if (nz[j]) v[j] = (T)A.mask_id;
        }
        if (A.vec_out) {
          if (whole) {
            dn_store_quad<T>(out_ids + at + c0, v);
            dn_store_quad<T>(out_labels + at + c0, lab);
          }
        } else {
#pragma unroll
          for (uint32_t j = 0; j < kBtQuad; j++) {
            if (!in[j]) continue;
            out_ids[at + c0 + j] = v[j];
            out_labels[at + c0 + j] = lab[j];
          }
        }
      }
      if (kRows && squeeze) {
        uint32_t o = p_before & 0xFFFFu, l = p_before >> 16;
#pragma unroll
        for (uint32_t j = 0; j < kBtQuad; j++) {
          if (!in[j]) continue;
          if (st[j]) {
            const T s = (T)(sentinel ? A.sentinel_ids[run[j]] : A.mask_id);  // run[j] < cap = n_sentinel - 1
            sid[o] = s; smask[o] = 1; o++;
            if (sentinel) slab[l++] = s;
          }
          if (nz[j]) {
            if (sentinel) slab[l++] = v[j];
          } else {
            sid[o] = v[j]; smask[o] = v[j] != (T)A.pad_id ? 1 : 0; o++;
          }
        }
        dn_wave_sync();
        // carry_o + step_o <= the columns walked so far <= width: a column gives the row one id at most
        if (live) {
          for (uint32_t i = sub; i < step_o; i += g) {
            out_ids[at + carry_o + i] = sid[i];
            if (A.out_mask) A.out_mask[at + carry_o + i] = smask[i];
          }
          if (sentinel)
            for (uint32_t i = sub; i < step_l; i += g)
              if ((uint64_t)carry_l + i < A.label_width) out_labels[b * A.label_width + carry_l + i] = slab[i];
        }
        dn_wave_sync();  // the reads are done before the next step stages
      }
      carry_o += step_o;
      carry_l += step_l;
    }
    // behind the row's last step: the closing sentinel, the fill and the lengths
    const uint32_t closing = carry_runs < A.cap ? carry_runs : A.cap;
    const uint32_t lab_len = sentinel ? carry_l + 1 : 0;
    if (live && !sub) {
      if (sentinel && lab_len > A.label_width) n[4]++;
      if (carry_o > most_len) most_len = carry_o;
      if (lab_len > most_lab) most_lab = lab_len;
    }
    if (kRows && squeeze && live) {
      for (uint64_t i = (uint64_t)carry_o + sub; i < A.width; i += g) {
        out_ids[at + i] = (T)A.pad_id;
        if (A.out_mask) A.out_mask[at + i] = 0;
      }
      if (sentinel) {
        if (!sub && carry_l < A.label_width) out_labels[b * A.label_width + carry_l] = (T)A.sentinel_ids[closing];
        for (uint64_t i = (uint64_t)lab_len + sub; i < A.label_width; i += g) out_labels[b * A.label_width + i] = (T)-100;
      }
      if (!sub) {
        if (A.out_len) A.out_len[b] = carry_o;
        if (A.out_label_len) A.out_label_len[b] = lab_len;
      }
    }
  }
  if (!A.part) return;  // uniform over the workgroup
  // the two maxima over the wavefront; the fold's barrier stands behind their stores too
  uint32_t m0 = most_len, m1 = most_lab;
  for (int d = 32; d; d >>= 1) {
    const uint32_t o0 = __shfl_xor(m0, d, 64), o1 = __shfl_xor(m1, d, 64);
    if (o0 > m0) m0 = o0;
    if (o1 > m1) m1 = o1;
  }
  if (lane == 0) { most[wave][0] = m0; most[wave][1] = m1; }
  unsigned long long sum = bt_fold_counts(n, counts);
  if (threadIdx.x >= kDnSums && threadIdx.x < kDnCounts)
    for (uint32_t w = 0; w < kDnWaves; w++)
      if (most[w][threadIdx.x - kDnSums] > sum) sum = most[w][threadIdx.x - kDnSums];
  if (threadIdx.x < kDnCounts) A.part[(uint64_t)blockIdx.x * kDnCounts + threadIdx.x] = sum;
}

// info[k] over the workgroups' counts: workgroup k sums (k < kDnSums) or takes the greatest; one workgroup per counter and no
// atomic, as counts_sum_kernel
__global__ __launch_bounds__(kDnThreads) void denoise_info_kernel(const unsigned long long *__restrict__ part, uint64_t n_blocks,
                                                                  unsigned long long *__restrict__ out) {
  __shared__ unsigned long long waves[kDnWaves];
  const uint32_t k = blockIdx.x;
  const bool most = k >= kDnSums;
  unsigned long long s = 0;
  for (uint64_t i = threadIdx.x; i < n_blocks; i += kDnThreads) {
    const unsigned long long x = part[i * kDnCounts + k];
    s = most ? (x > s ? x : s) : s + x;
  }
  for (int d = 32; d; d >>= 1) {
    const unsigned long long o = __shfl_xor(s, d, 64);
    s = most ? (o > s ? o : s) : s + o;
  }
  if ((threadIdx.x & 63) == 0) waves[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x) return;
  s = 0;
  for (uint32_t w = 0; w < kDnWaves; w++) s = most ? (waves[w] > s ? waves[w] : s) : s + waves[w];
  out[k] = s;
}

// the workgroups' counts between the two launches: grow-only and shared by all calls of the process, under swt_mlm_mask_dev's rule
static DevBuf g_denoise_ws;

static bool dn_overlap(const void *a, size_t na, const void *b, size_t nb) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return a && b && na && nb && x < y + nb && y < x + na;
}

struct DenoiseOut {
  void *ids, *labels;
  uint8_t *mask;
  uint32_t *len, *label_len;
};

// What all forms refuse, from the arguments alone; out: null for a plan.
static int dn_check(const void *ids, uint64_t rows, uint32_t width, const uint8_t *cls_tab, const uint32_t *sentinel_ids,
                    const swt_denoise_spec *spec, const DenoiseOut *out) {
  if (!spec) return fail(SWT_ERR_INVALID, "null argument: spec");
  if (!ids) return fail(SWT_ERR_INVALID, "null argument: ids");
  if (!cls_tab) return fail(SWT_ERR_INVALID, "null argument: cls_tab");
  if (int rc = bt_check_shape(rows, width)) return rc;
  if (spec->flags & ~kDnFlags) return fail(SWT_ERR_INVALID, "flags: unknown flag");
  if (spec->mode > SWT_DENOISE_INFILL) return fail(SWT_ERR_INVALID, "mode: unknown mode");
  const uint64_t one = 1ull << 32;
  if (spec->start_below > one) return fail(SWT_ERR_INVALID, "start_below is above 2^32");
  if (spec->n_len > kDnLenMax) return fail(SWT_ERR_INVALID, "n_len: more than 31 thresholds");
  for (uint32_t k = 0; k < spec->n_len; k++) {
    if (spec->len_below[k] > one) return fail(SWT_ERR_INVALID, "len_below: an entry is above 2^32");
    if (k && spec->len_below[k] < spec->len_below[k - 1]) return fail(SWT_ERR_INVALID, "len_below decreases");
  }
  if (!spec->n_class) return fail(SWT_ERR_INVALID, "n_class: a class table of no entry");
  const bool sentinel = spec->mode == SWT_DENOISE_SENTINEL, squeeze = spec->mode != SWT_DENOISE_MASK;
  if (sentinel && spec->n_sentinel < 2) return fail(SWT_ERR_INVALID, "n_sentinel: SENTINEL mode takes two sentinels or more");
  if (!out) return SWT_OK;
  if (sentinel && !sentinel_ids) return fail(SWT_ERR_INVALID, "null argument: sentinel_ids");
  if (!out->ids) return fail(SWT_ERR_INVALID, "null argument: out_ids");
  if (spec->mode != SWT_DENOISE_INFILL && !out->labels) return fail(SWT_ERR_INVALID, "null argument: out_labels");
  if (spec->mode == SWT_DENOISE_INFILL && out->labels) return fail(SWT_ERR_INVALID, "out_labels: INFILL mode has no label output");
  if (!sentinel && out->label_len) return fail(SWT_ERR_INVALID, "out_label_len: only SENTINEL mode has label lengths");
  if (!squeeze && (out->mask || out->len)) return fail(SWT_ERR_INVALID, "out_mask, out_len: MASK mode has neither");
  const size_t idb = (spec->flags & SWT_DENOISE_IDS64) ? 8 : 4, cells = (size_t)rows * width;
  const size_t lab_cells = sentinel ? (size_t)rows * spec->label_width : cells;
  if (dn_overlap(ids, cells * idb, out->ids, cells * idb)) return fail(SWT_ERR_INVALID, "out_ids overlaps ids: not in place");
  if (dn_overlap(ids, cells * idb, out->labels, lab_cells * idb)) return fail(SWT_ERR_INVALID, "out_labels overlaps ids: not in place");
  if (dn_overlap(ids, cells * idb, out->mask, cells)) return fail(SWT_ERR_INVALID, "out_mask overlaps ids: not in place");
  if (dn_overlap(ids, cells * idb, out->len, (size_t)rows * 4)) return fail(SWT_ERR_INVALID, "out_len overlaps ids: not in place");
  if (dn_overlap(ids, cells * idb, out->label_len, (size_t)rows * 4)) return fail(SWT_ERR_INVALID, "out_label_len overlaps ids: not in place");
  return SWT_OK;
}

// Both `_dev` forms behind their checks: the walk (the plan with out == null), then the counts into d_info.
static int dn_launch(const void *d_ids, uint64_t rows, uint32_t width, const uint8_t *d_cls_tab, const uint32_t *d_sentinel_ids,
                     const swt_denoise_spec *spec, const DenoiseOut *out, uint64_t *d_info, hipStream_t st) {
  int rc;
  const uintptr_t idb = (spec->flags & SWT_DENOISE_IDS64) ? 8 : 4;
  const DenoiseOut none{nullptr, nullptr, nullptr, nullptr, nullptr};
  const DenoiseOut &o = out ? *out : none;
  if (!bt_aligned(idb, {d_ids, o.ids, o.labels}) || !bt_aligned(4, {d_sentinel_ids, o.len, o.label_len}) || !bt_aligned(8, {d_info}))
    return fail(SWT_ERR_INVALID, "an array is not aligned to its element type");
  if ((rc = ensure_device())) return rc;
  if (!rows) {
    if (d_info) SWT_HIP(hipMemsetAsync(d_info, 0, kDnCounts * 8, st));
    return SWT_OK;
  }
  DenoiseArgs A{};
  A.ids = d_ids; A.rows = rows; A.width = width; A.cls_tab = d_cls_tab; A.n_class = spec->n_class; A.sentinel_ids = d_sentinel_ids;
  A.key0 = (uint32_t)spec->seed; A.key1 = (uint32_t)(spec->seed >> 32); A.epoch = spec->epoch;
  A.whole_word = (spec->flags & SWT_DENOISE_WHOLE_WORD) ? 1u : 0u;
  A.mode = spec->mode; A.mask_id = spec->mask_id; A.pad_id = spec->pad_id; A.n_len = spec->n_len;
  A.cap = spec->mode == SWT_DENOISE_SENTINEL ? spec->n_sentinel - 1 : kDnNoCap;
  A.label_width = spec->label_width; A.start_below = spec->start_below;
  for (uint32_t k = 0; k < spec->n_len; k++) A.len_below[k] = spec->len_below[k];
  A.out_ids = o.ids; A.out_labels = o.labels; A.out_mask = o.mask; A.out_len = o.len; A.out_label_len = o.label_len;
  A.vec_in = width % kBtQuad == 0 && bt_aligned(16, {d_ids});
  A.vec_out = A.vec_in && bt_aligned(16, {o.ids, o.labels});
  A.group = bt_group(width);
  const RowShape shape = bt_shape(rows, A.group, kDnWaves);
  A.sets = (uint32_t)shape.sets;
  const unsigned grid = shape.grid;
  if (d_info) {
    if ((rc = g_denoise_ws.reserve((size_t)grid * kDnCounts * 8))) return rc;
    A.part = g_denoise_ws.as<unsigned long long>();
  }
  const bool ids64 = spec->flags & SWT_DENOISE_IDS64;
  prof_begin(st);
  if (out) {
    if (ids64) hipLaunchKernelGGL((denoise_kernel<int64_t, true>), dim3(grid), dim3(kDnThreads), 0, st, A);
    else hipLaunchKernelGGL((denoise_kernel<int32_t, true>), dim3(grid), dim3(kDnThreads), 0, st, A);
  } else {
    if (ids64) hipLaunchKernelGGL((denoise_kernel<int64_t, false>), dim3(grid), dim3(kDnThreads), 0, st, A);
    else hipLaunchKernelGGL((denoise_kernel<int32_t, false>), dim3(grid), dim3(kDnThreads), 0, st, A);
  }
  prof_end(st);
  if (d_info)
    hipLaunchKernelGGL(denoise_info_kernel, dim3(kDnCounts), dim3(kDnThreads), 0, st, A.part, (uint64_t)grid,
                       reinterpret_cast<unsigned long long *>(d_info));
  SWT_HIP(hipGetLastError());
  return SWT_OK;
}

}  // namespace swt

using namespace swt;

extern "C" {

int swt_denoise_capacity(uint32_t *cols_per_step, uint32_t *stage_labels, uint32_t *n_len_max) try {
  if (cols_per_step) *cols_per_step = kBtCols;
  if (stage_labels) *stage_labels = 2 * kBtCols;
  if (n_len_max) *n_len_max = kDnLenMax;
  return SWT_OK;
} SWT_API_CATCH

int swt_denoise_plan_dev(const void *d_ids, uint64_t rows, uint32_t width, const uint8_t *d_cls_tab, const swt_denoise_spec *spec,
                         uint64_t *d_info, void *stream) try {
  int rc = dn_check(d_ids, rows, width, d_cls_tab, nullptr, spec, nullptr);
  if (rc) return rc;
  if (!d_info) return fail(SWT_ERR_INVALID, "null argument: info");
  return dn_launch(d_ids, rows, width, d_cls_tab, nullptr, spec, nullptr, d_info, (hipStream_t)stream);
} SWT_API_CATCH

int swt_denoise_plan(const void *ids, uint64_t rows, uint32_t width, const uint8_t *cls_tab, const swt_denoise_spec *spec,
                     uint64_t *info) try {
  int rc = dn_check(ids, rows, width, cls_tab, nullptr, spec, nullptr);
  if (rc) return rc;
  if (!info) return fail(SWT_ERR_INVALID, "null argument: info");
  for (uint32_t k = 0; k < kDnCounts; k++) info[k] = 0;
  if (!rows) return SWT_OK;
  if ((rc = ensure_device())) return rc;
  const size_t idb = (spec->flags & SWT_DENOISE_IDS64) ? 8 : 4;
  BatchStage s;
  const void *d_ids = s.in(static_cast<const uint8_t *>(ids), (size_t)rows * width * idb);
  const uint8_t *d_cls = s.in(cls_tab, spec->n_class);
  uint64_t *d_info = s.out(info, kDnCounts * 8);
  if (s.rc) return s.rc;
  if ((rc = swt_denoise_plan_dev(d_ids, rows, width, d_cls, spec, d_info, nullptr))) return rc;
  return s.fetch();
} SWT_API_CATCH

int swt_denoise_rows_dev(const void *d_ids, uint64_t rows, uint32_t width, const uint8_t *d_cls_tab, const uint32_t *d_sentinel_ids,
                         const swt_denoise_spec *spec, void *d_out_ids, uint8_t *d_out_mask, uint32_t *d_out_len, void *d_out_labels,
                         uint32_t *d_out_label_len, uint64_t *d_info, void *stream) try {
  const DenoiseOut out{d_out_ids, d_out_labels, d_out_mask, d_out_len, d_out_label_len};
  int rc = dn_check(d_ids, rows, width, d_cls_tab, d_sentinel_ids, spec, &out);
  if (rc) return rc;
  return dn_launch(d_ids, rows, width, d_cls_tab, d_sentinel_ids, spec, &out, d_info, (hipStream_t)stream);
} SWT_API_CATCH

int swt_denoise_rows(const void *ids, uint64_t rows, uint32_t width, const uint8_t *cls_tab, const uint32_t *sentinel_ids,
                     const swt_denoise_spec *spec, void *out_ids, uint8_t *out_mask, uint32_t *out_len, void *out_labels,
                     uint32_t *out_label_len, uint64_t *info) try {
  const DenoiseOut out{out_ids, out_labels, out_mask, out_len, out_label_len};
  int rc = dn_check(ids, rows, width, cls_tab, sentinel_ids, spec, &out);
  if (rc) return rc;
  if (info)
    for (uint32_t k = 0; k < kDnCounts; k++) info[k] = 0;
  if (!rows) return SWT_OK;
  if ((rc = ensure_device())) return rc;
  const bool sentinel = spec->mode == SWT_DENOISE_SENTINEL;
  const size_t idb = (spec->flags & SWT_DENOISE_IDS64) ? 8 : 4, cells = (size_t)rows * width;
  const size_t lab_cells = sentinel ? (size_t)rows * spec->label_width : cells;
  BatchStage s;
  const void *d_ids = s.in(static_cast<const uint8_t *>(ids), cells * idb);
  const uint8_t *d_cls = s.in(cls_tab, spec->n_class);
  const uint32_t *d_sent = sentinel ? s.in(sentinel_ids, (size_t)spec->n_sentinel * 4) : nullptr;
  void *d_out = s.out(static_cast<uint8_t *>(out_ids), cells * idb), *d_lab = s.out(static_cast<uint8_t *>(out_labels), lab_cells * idb);
  uint8_t *d_mask = s.out(out_mask, cells);
  uint32_t *d_len = s.out(out_len, (size_t)rows * 4), *d_lab_len = s.out(out_label_len, (size_t)rows * 4);
  uint64_t *d_info = s.out(info, kDnCounts * 8);
  if (s.rc) return s.rc;
  if ((rc = swt_denoise_rows_dev(d_ids, rows, width, d_cls, d_sent, spec, d_out, d_mask, d_len, d_lab, d_lab_len, d_info, nullptr))) return rc;
  return s.fetch();
} SWT_API_CATCH

}  // extern "C"
