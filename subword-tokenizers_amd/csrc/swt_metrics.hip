// swt_metrics.hip -- token-id histogram on the device: what the reference's benchmark suite counts with a Python Counter
// over token STRINGS (/root/reference/source/benchmarks.py:240-253, zipf_distribution) counted over token IDS, which are
// in bijection with the strings (a token with the '##' prefix and the same token without it are different strings and
// different ids: SWT_BPE_CONT).  SURVEY.md section 8f-3: so that the quality metrics run on 10 M-sentence outputs that never
// leave the device as strings.
//
// Token frequencies are Zipfian, so a global atomicAdd per token would serialise on the few hot ids.  Every wave stages its
// counters in LDS (a 1,024-slot table per wave, linear probing, the same pattern as the trainer's hist_build_kernel) and
// only the distinct ids of a wave's stretch reach the global array, one atomicAdd each.
//
// Second half: token-sequence equivalence of two tokenizers (/root/reference/source/benchmarks.py:113-183) over two id
// streams, row by row.  The reference compares token STRINGS after stripping a leading '##'; the caller gives each stream a
// map from its ids to canonical ids (one id per stripped string, shared by both tokenizers) and the kernels compare those.
#include "swt_common.h"

namespace swt {

constexpr int kMhThreads = 256;
constexpr int kMhSlots = 1024;
constexpr int kMhPerLane = 64;  // ids per lane: a wave flushes after 4,096 ids

__global__ __launch_bounds__(kMhThreads) void token_hist_kernel(const uint32_t *__restrict__ ids, uint64_t n, uint32_t id_cap,
                                                                unsigned long long *__restrict__ counts, unsigned long long *__restrict__ oor) {
  __shared__ uint32_t lk[kMhThreads / 64][kMhSlots];
  __shared__ uint32_t lc[kMhThreads / 64][kMhSlots];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t wave_id = (uint64_t)blockIdx.x * (kMhThreads / 64) + wave, n_waves = (uint64_t)gridDim.x * (kMhThreads / 64);
  for (uint64_t base = wave_id * 64 * kMhPerLane; base < n; base += n_waves * 64 * kMhPerLane) {
    for (int i = lane; i < kMhSlots; i += 64) { lk[wave][i] = 0xFFFFFFFFu; lc[wave][i] = 0; }
    __builtin_amdgcn_wave_barrier();
    for (int u = 0; u < kMhPerLane; u++) {
      const uint64_t i = base + (uint64_t)u * 64 + lane;  // coalesced: the wave reads 256 contiguous bytes per step
      if (i >= n) break;
      const uint32_t id = ids[i];
      const uint32_t sym = id & 0x7FFFFFFFu;
      if (sym >= id_cap) { atomicAdd(oor, 1ull); continue; }
      const uint32_t idx = sym + ((id >> 31) ? id_cap : 0u);
      uint32_t h = (idx * 2654435761u) >> 22;  // 10 bits
      bool done = false;
      for (int probe = 0; probe < 8 && !done; probe++) {
        uint32_t k = lk[wave][h];
        if (k == 0xFFFFFFFFu) {
          k = atomicCAS(&lk[wave][h], 0xFFFFFFFFu, idx);
          if (k == 0xFFFFFFFFu) k = idx;
        }
        if (k == idx) { atomicAdd(&lc[wave][h], 1u); done = true; }
        h = (h + 1) & (kMhSlots - 1);
      }
      if (!done) atomicAdd(&counts[idx], 1ull);  // the wave's table is crowded: straight to global
    }
    __builtin_amdgcn_wave_barrier();
    for (int i = lane; i < kMhSlots; i += 64)
      if (lk[wave][i] != 0xFFFFFFFFu) atomicAdd(&counts[lk[wave][i]], (unsigned long long)lc[wave][i]);
    __builtin_amdgcn_wave_barrier();
  }
}

// ---- token-sequence equivalence -----------------------------------------------------------------------------------------
// Per row (a sentence, or a word): positions = min(len a, len b); pos_matches = positions with the same canonical id on both
// sides; unordered = the multiset intersection, sum over tokens of min(count a, count b); has_common = the token SETS meet.
// The last two come from a hash table keyed by canonical id with TWO counters per slot: the shorter side is inserted
// (counter A), the longer side probes (counter B; a miss contributes nothing), and the row's values are read off the slots --
// min() is symmetric, so it does not matter which side is inserted, and nothing is ever decremented.
//
//   token_equiv_wave_kernel    one wavefront per row, a 512-slot table per wave in LDS; takes the rows whose shorter side has
//                              at most kTeWaveCap = 256 tokens.  The table is never more than half full, so plain linear
//                              probing always ends at the key or at an empty slot: there is no bounded probe that could fail.
//   token_equiv_block_kernel   one 1,024-thread workgroup per remaining row, a 4,096-slot table in LDS that takes at most
//                              kTeBlockCap = 2,048 distinct keys.  A row with more is counted in PASSES over a partition of
//                              the key space: pass (d, q) takes the tokens whose hash has the top d bits q.  The first d is the
//                              smallest with shorter length <= kTeBlockCap << d; a pass that still meets more than
//                              kTeBlockCap distinct keys is abandoned and replaced by its two halves (d + 1, 2q), (d + 1, 2q + 1).
//                              The hash is a bijection of the 32-bit ids, so a part at depth 21 cannot hold more than 2,048
//                              keys and the splitting ends.  Exact for any row, no scratch memory, nothing left to the host.
constexpr int kTeThreads = 256;
constexpr int kTeWaveSlots = 512;
constexpr uint32_t kTeWaveCap = 256;
constexpr int kTeBlockThreads = 1024;
constexpr int kTeBlockSlots = 4096;
constexpr uint32_t kTeBlockCap = 2048;
constexpr int kTeMaxDepth0 = 20;
constexpr int kTeSplitDepthMax = 21;  // 2^(32 - 21) = 2,048 possible keys in a part: never more than kTeBlockCap distinct ones
constexpr int kTeStackPairs = kTeSplitDepthMax + 2;  // one pair per depth 0..21 is the most a depth-first walk holds, and one spare
static_assert((1ull << (32 - kTeSplitDepthMax)) <= kTeBlockCap && kTeMaxDepth0 <= kTeSplitDepthMax, "the splitting must end within the stack");
constexpr uint32_t kTeNone = 0xFFFFFFFFu;  // no canonical id (an id beyond its map); also the empty slot

struct TeSide {
  const uint32_t *ids;
  const uint64_t *off;
  const uint32_t *map;
  uint32_t map_base, n_map;
  int flagged;
};

__device__ __forceinline__ uint32_t te_canon(const TeSide &s, uint64_t i) {
  const uint32_t id = s.ids[i], sym = id & 0x7FFFFFFFu;
  if (sym < s.map_base) return sym;
  const uint32_t k = sym - s.map_base;
  if (k >= s.n_map) return kTeNone;
  return s.map[k + ((s.flagged && (id >> 31)) ? s.n_map : 0u)];
}

__device__ __forceinline__ uint32_t te_hash(uint32_t c) { return c * 2654435761u; }  // odd multiplier: a bijection

__device__ __forceinline__ unsigned long long te_wave_sum(unsigned long long v) {
  for (int d = 32; d; d >>= 1) v += __shfl_down(v, d, 64);
  return v;  // lane 0 holds the sum
}

// find the slot of key c, claiming an empty one when `insert`; -1: not there (probe only).  The caller guarantees an empty slot.
template <int Slots>
__device__ __forceinline__ int te_slot(uint32_t *keys, uint32_t c, uint32_t h, bool insert, bool *claimed) {
  for (;;) {
    uint32_t k = keys[h];
    if (k == kTeNone) {
      if (!insert) return -1;
      k = atomicCAS(&keys[h], kTeNone, c);
      if (k == kTeNone) { *claimed = true; return (int)h; }
    }
    if (k == c) return (int)h;
    h = (h + 1) & (Slots - 1);
  }
}

__global__ __launch_bounds__(kTeThreads) void token_equiv_wave_kernel(TeSide A, TeSide B, uint64_t n_rows, const uint32_t *__restrict__ weight,
                                                                      unsigned long long *__restrict__ totals, uint32_t *__restrict__ per_row) {
  __shared__ uint32_t tk[kTeThreads / 64][kTeWaveSlots];
  __shared__ uint32_t ta[kTeThreads / 64][kTeWaveSlots];
  __shared__ uint32_t tb[kTeThreads / 64][kTeWaveSlots];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t wave_id = (uint64_t)blockIdx.x * (kTeThreads / 64) + wave, n_waves = (uint64_t)gridDim.x * (kTeThreads / 64);
  unsigned long long t_pos = 0, t_pm = 0, t_un = 0, t_cm = 0, t_oor = 0;  // lane 0's: this wave's share of totals[0..5)
  for (uint64_t row = wave_id; row < n_rows; row += n_waves) {
    const uint64_t a0 = A.off[row], b0 = B.off[row];
    const uint64_t la = A.off[row + 1] - a0, lb = B.off[row + 1] - b0;
    const uint64_t m = la < lb ? la : lb, mx = la < lb ? lb : la;
    if (m > kTeWaveCap) continue;  // token_equiv_block_kernel's
    unsigned long long pm = 0, oor = 0, un = 0, cm = 0;
    for (uint64_t i = lane; i < mx; i += 64) {  // positional matches; every token is looked at once here: ids beyond the maps
      const uint32_t ca = i < la ? te_canon(A, a0 + i) : kTeNone, cb = i < lb ? te_canon(B, b0 + i) : kTeNone;
      oor += (i < la && ca == kTeNone) + (i < lb && cb == kTeNone);
      pm += (ca != kTeNone && ca == cb);
    }
    if (m) {
      const TeSide &S = la <= lb ? A : B, &L = la <= lb ? B : A;
      const uint64_t s0 = la <= lb ? a0 : b0, l0 = la <= lb ? b0 : a0;
      for (int i = lane; i < kTeWaveSlots; i += 64) { tk[wave][i] = kTeNone; ta[wave][i] = 0; tb[wave][i] = 0; }
      __builtin_amdgcn_wave_barrier();
      for (uint64_t i = lane; i < m; i += 64) {
        const uint32_t c = te_canon(S, s0 + i);
        if (c == kTeNone) continue;
        bool claimed = false;
        atomicAdd(&ta[wave][te_slot<kTeWaveSlots>(tk[wave], c, te_hash(c) >> 23, true, &claimed)], 1u);
      }
      __builtin_amdgcn_wave_barrier();
      for (uint64_t i = lane; i < mx; i += 64) {
        const uint32_t c = te_canon(L, l0 + i);
        if (c == kTeNone) continue;
        bool claimed = false;
        const int h = te_slot<kTeWaveSlots>(tk[wave], c, te_hash(c) >> 23, false, &claimed);
        if (h >= 0) atomicAdd(&tb[wave][h], 1u);
      }
      __builtin_amdgcn_wave_barrier();
      for (int i = lane; i < kTeWaveSlots; i += 64) {
        const uint32_t a = ta[wave][i], b = tb[wave][i];
        un += a < b ? a : b;
        cm |= (a && b);
      }
      __builtin_amdgcn_wave_barrier();
    }
    pm = te_wave_sum(pm);
    oor = te_wave_sum(oor);
    un = te_wave_sum(un);
    cm = te_wave_sum(cm) ? 1 : 0;
    if (lane == 0) {
      if (per_row) {
        per_row[4 * row] = (uint32_t)m;
        per_row[4 * row + 1] = (uint32_t)pm;
        per_row[4 * row + 2] = (uint32_t)un;
        per_row[4 * row + 3] = (uint32_t)cm;
      }
      const unsigned long long w = weight ? weight[row] : 1u;
      t_pos += m * w;
      t_pm += pm * w;
      t_un += un * w;
      t_cm += cm * w;
      t_oor += oor;
    }
  }
  if (lane == 0) {  // one atomic per wave and counter
    if (t_pos) atomicAdd(&totals[0], t_pos);
    if (t_pm) atomicAdd(&totals[1], t_pm);
    if (t_un) atomicAdd(&totals[2], t_un);
    if (t_cm) atomicAdd(&totals[3], t_cm);
    if (t_oor) atomicAdd(&totals[4], t_oor);
  }
}

__global__ __launch_bounds__(kTeBlockThreads) void token_equiv_block_kernel(TeSide A, TeSide B, uint64_t n_rows, const uint32_t *__restrict__ weight,
                                                                        unsigned long long *__restrict__ totals, uint32_t *__restrict__ per_row) {
  __shared__ uint32_t tk[kTeBlockSlots], ta[kTeBlockSlots], tb[kTeBlockSlots];
  __shared__ uint32_t queue[kTeBlockThreads];  // the long rows among the 1,024 this workgroup is looking at
  __shared__ uint32_t n_queue, n_keys;
  // (depth, part) of the passes still to do.  A split replaces the top pair by two of the next depth, so the stack grows by one
  // per depth below the first; depths run from d0 <= kTeMaxDepth0 to kTeSplitDepthMax, where a part cannot overflow any more
  __shared__ uint32_t stack[2 * kTeStackPairs];
  __shared__ int sp;
  __shared__ unsigned long long acc[4];  // the row's pos_matches, unordered, has_common, ids beyond the maps
  const int tid = threadIdx.x, lane = threadIdx.x & 63;
  unsigned long long t_pos = 0, t_pm = 0, t_un = 0, t_cm = 0, t_oor = 0;  // thread 0's
  for (uint64_t tile = blockIdx.x; tile * kTeBlockThreads < n_rows; tile += gridDim.x) {
    if (tid == 0) n_queue = 0;
    __syncthreads();
    {
      const uint64_t r = tile * kTeBlockThreads + tid;
      if (r < n_rows) {
        const uint64_t la = A.off[r + 1] - A.off[r], lb = B.off[r + 1] - B.off[r];
        if ((la < lb ? la : lb) > kTeWaveCap) queue[atomicAdd(&n_queue, 1u)] = (uint32_t)tid;
      }
    }
    __syncthreads();
    const uint32_t nq = n_queue;
    for (uint32_t qi = 0; qi < nq; qi++) {
      const uint64_t row = tile * kTeBlockThreads + queue[qi];
      const uint64_t a0 = A.off[row], b0 = B.off[row];
      const uint64_t la = A.off[row + 1] - a0, lb = B.off[row + 1] - b0;
      const uint64_t m = la < lb ? la : lb, mx = la < lb ? lb : la;
      const TeSide &S = la <= lb ? A : B, &L = la <= lb ? B : A;
      const uint64_t s0 = la <= lb ? a0 : b0, l0 = la <= lb ? b0 : a0;
      if (tid < 4) acc[tid] = 0;
      __syncthreads();
      {
        unsigned long long pm = 0, oor = 0;
        for (uint64_t i = tid; i < mx; i += kTeBlockThreads) {
          const uint32_t ca = i < la ? te_canon(A, a0 + i) : kTeNone, cb = i < lb ? te_canon(B, b0 + i) : kTeNone;
          oor += (i < la && ca == kTeNone) + (i < lb && cb == kTeNone);
          pm += (ca != kTeNone && ca == cb);
        }
        pm = te_wave_sum(pm);
        oor = te_wave_sum(oor);
        if (lane == 0 && pm) atomicAdd(&acc[0], pm);
        if (lane == 0 && oor) atomicAdd(&acc[3], oor);
      }
      int d0 = 0;
      while (d0 < kTeMaxDepth0 && m > ((uint64_t)kTeBlockCap << d0)) d0++;
      for (uint32_t part0 = 0; part0 < (1u << d0); part0++) {
        __syncthreads();  // everybody has seen the last part's stack run empty
        if (tid == 0) { stack[0] = (uint32_t)d0; stack[1] = part0; sp = 1; }
        for (;;) {
          __syncthreads();  // thread 0's stack writes (and the last pass's table reads) are done
          const int top = sp;
          if (top == 0) break;
          const uint32_t d = stack[2 * (top - 1)], q = stack[2 * (top - 1) + 1];
          __syncthreads();  // everybody has read the top before thread 0 pops it
          if (tid == 0) { sp = top - 1; n_keys = 0; }
          for (int i = tid; i < kTeBlockSlots; i += kTeBlockThreads) { tk[i] = kTeNone; ta[i] = 0; tb[i] = 0; }
          __syncthreads();
          for (uint64_t i = tid; i < m; i += kTeBlockThreads) {
            // at most kTeBlockCap + 1 claims before this is seen, and one more per thread after it: 3,073 < 4,096 slots
            if (*(volatile uint32_t *)&n_keys > kTeBlockCap) break;
            const uint32_t c = te_canon(S, s0 + i);
            if (c == kTeNone) continue;
            const uint32_t h = te_hash(c);
            if (d && (h >> (32 - d)) != q) continue;
            bool claimed = false;
            const int slot = te_slot<kTeBlockSlots>(tk, c, (h << d) >> 20, true, &claimed);
            if (claimed) atomicAdd(&n_keys, 1u);
            atomicAdd(&ta[slot], 1u);
          }
          __syncthreads();
          if (n_keys > kTeBlockCap) {  // too many distinct keys for one table: the two halves of this part instead
            if (tid == 0) {
              stack[2 * (top - 1)] = d + 1; stack[2 * (top - 1) + 1] = 2 * q;
              stack[2 * top] = d + 1; stack[2 * top + 1] = 2 * q + 1;
              sp = top + 1;
            }
            continue;
          }
          for (uint64_t i = tid; i < mx; i += kTeBlockThreads) {
            const uint32_t c = te_canon(L, l0 + i);
            if (c == kTeNone) continue;
            const uint32_t h = te_hash(c);
            if (d && (h >> (32 - d)) != q) continue;
            bool claimed = false;
            const int slot = te_slot<kTeBlockSlots>(tk, c, (h << d) >> 20, false, &claimed);
            if (slot >= 0) atomicAdd(&tb[slot], 1u);
          }
          __syncthreads();
          unsigned long long un = 0, cm = 0;
          for (int i = tid; i < kTeBlockSlots; i += kTeBlockThreads) {
            const uint32_t a = ta[i], b = tb[i];
            un += a < b ? a : b;
            cm |= (a && b);
          }
          un = te_wave_sum(un);
          cm = te_wave_sum(cm);
          if (lane == 0 && un) atomicAdd(&acc[1], un);
          if (lane == 0 && cm) atomicMax(&acc[2], 1ull);
        }
      }
      __syncthreads();
      if (tid == 0) {
        if (per_row) {
          per_row[4 * row] = (uint32_t)m;
          per_row[4 * row + 1] = (uint32_t)acc[0];
          per_row[4 * row + 2] = (uint32_t)acc[1];
          per_row[4 * row + 3] = (uint32_t)acc[2];
        }
        const unsigned long long w = weight ? weight[row] : 1u;
        t_pos += m * w;
        t_pm += acc[0] * w;
        t_un += acc[1] * w;
        t_cm += acc[2] * w;
        t_oor += acc[3];
      }
      __syncthreads();
    }
  }
  if (tid == 0) {
    if (t_pos) atomicAdd(&totals[0], t_pos);
    if (t_pm) atomicAdd(&totals[1], t_pm);
    if (t_un) atomicAdd(&totals[2], t_un);
    if (t_cm) atomicAdd(&totals[3], t_cm);
    if (t_oor) atomicAdd(&totals[4], t_oor);
  }
}

}  // namespace swt

using namespace swt;

extern "C" {

int swt_token_histogram_dev(const uint32_t *d_ids, uint64_t n, uint32_t id_cap, uint64_t *d_counts, uint64_t *d_out_of_range, void *stream) try {
  if ((n && !d_ids) || !d_counts || !d_out_of_range || !id_cap) return fail(SWT_ERR_INVALID, "null argument");
  int rc = ensure_device();
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  SWT_HIP(hipMemsetAsync(d_counts, 0, (size_t)2 * id_cap * 8, st));
  SWT_HIP(hipMemsetAsync(d_out_of_range, 0, 8, st));
  if (!n) return SWT_OK;
  uint64_t blocks = (n + (uint64_t)kMhThreads * kMhPerLane - 1) / ((uint64_t)kMhThreads * kMhPerLane);
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(token_hist_kernel, dim3((unsigned)blocks), dim3(kMhThreads), 0, st, d_ids, n, id_cap,
                     reinterpret_cast<unsigned long long *>(d_counts), reinterpret_cast<unsigned long long *>(d_out_of_range));
  SWT_HIP(hipGetLastError());
  return SWT_OK;
} SWT_API_CATCH

int swt_token_histogram(const uint32_t *ids, uint64_t n, uint32_t id_cap, uint64_t *counts, uint64_t *out_of_range) try {
  if ((n && !ids) || !counts || !out_of_range || !id_cap) return fail(SWT_ERR_INVALID, "null argument");
  int rc = ensure_device();
  if (rc) return rc;
  DevBuf d_ids, d_counts;
  struct Guard { DevBuf &a, &b; ~Guard() { a.release(); b.release(); } } guard{d_ids, d_counts};
  if ((rc = d_ids.reserve(n * 4 + 16)) || (rc = d_counts.reserve((size_t)2 * id_cap * 8 + 16))) return rc;
  if (n) SWT_HIP(hipMemcpy(d_ids.p, ids, n * 4, hipMemcpyHostToDevice));
  uint64_t *d_c = d_counts.as<uint64_t>();
  if ((rc = swt_token_histogram_dev(d_ids.as<uint32_t>(), n, id_cap, d_c + 1, d_c, nullptr))) return rc;
  SWT_HIP(hipStreamSynchronize(nullptr));
  SWT_HIP(hipMemcpy(out_of_range, d_c, 8, hipMemcpyDeviceToHost));
  SWT_HIP(hipMemcpy(counts, d_c + 1, (size_t)2 * id_cap * 8, hipMemcpyDeviceToHost));
  return SWT_OK;
} SWT_API_CATCH

int swt_token_equivalence_capacity(uint32_t *wave_cap, uint32_t *block_cap) try {
  if (wave_cap) *wave_cap = kTeWaveCap;
  if (block_cap) *block_cap = kTeBlockCap;
  return SWT_OK;
} SWT_API_CATCH

int swt_token_equivalence_dev(const uint32_t *d_ids_a, const uint64_t *d_off_a, const uint32_t *d_map_a, uint32_t map_base_a, uint32_t n_map_a, int flagged_a,
                              const uint32_t *d_ids_b, const uint64_t *d_off_b, const uint32_t *d_map_b, uint32_t map_base_b, uint32_t n_map_b, int flagged_b,
                              uint64_t n_rows, const uint32_t *d_weight, uint64_t *d_totals, uint32_t *d_per_row, void *stream) try {
  if (!d_totals || (n_rows && (!d_off_a || !d_off_b)) || (n_map_a && !d_map_a) || (n_map_b && !d_map_b)) return fail(SWT_ERR_INVALID, "null argument");
  if (n_rows >= (1ull << 61)) return fail(SWT_ERR_INVALID, "too many rows");
  int rc = ensure_device();
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  SWT_HIP(hipMemsetAsync(d_totals, 0, 5 * 8, st));
  if (!n_rows) return SWT_OK;
  if (d_per_row) SWT_HIP(hipMemsetAsync(d_per_row, 0, (size_t)n_rows * 16, st));
  const TeSide A{d_ids_a, d_off_a, d_map_a, map_base_a, n_map_a, flagged_a}, B{d_ids_b, d_off_b, d_map_b, map_base_b, n_map_b, flagged_b};
  unsigned long long *tot = reinterpret_cast<unsigned long long *>(d_totals);
  uint64_t blocks = (n_rows + kTeThreads / 64 - 1) / (kTeThreads / 64), cap = (uint64_t)device_cus() * 8;
  if (blocks > cap) blocks = cap;
  prof_begin(st, 2);  // both kernels: which of them dominates depends on the rows, so there is no level-1 bracket here
  hipLaunchKernelGGL(token_equiv_wave_kernel, dim3((unsigned)blocks), dim3(kTeThreads), 0, st, A, B, n_rows, d_weight, tot, d_per_row);
  SWT_HIP(hipGetLastError());
  // the rows the wave kernel left out; a workgroup whose 1,024-row tiles hold none of them only reads their offsets
  blocks = (n_rows + kTeBlockThreads - 1) / kTeBlockThreads;
  cap = (uint64_t)device_cus();
  if (blocks > cap) blocks = cap;
  hipLaunchKernelGGL(token_equiv_block_kernel, dim3((unsigned)blocks), dim3(kTeBlockThreads), 0, st, A, B, n_rows, d_weight, tot, d_per_row);
  prof_end(st, 2);
  SWT_HIP(hipGetLastError());
  return SWT_OK;
} SWT_API_CATCH

int swt_token_equivalence(const uint32_t *ids_a, const uint64_t *off_a, const uint32_t *map_a, uint32_t map_base_a, uint32_t n_map_a, int flagged_a,
                          const uint32_t *ids_b, const uint64_t *off_b, const uint32_t *map_b, uint32_t map_base_b, uint32_t n_map_b, int flagged_b,
                          uint64_t n_rows, const uint32_t *weight, uint64_t *totals, uint32_t *per_row) try {
  if (!totals || (n_rows && (!off_a || !off_b)) || (n_map_a && !map_a) || (n_map_b && !map_b)) return fail(SWT_ERR_INVALID, "null argument");
  if (n_rows >= (1ull << 61)) return fail(SWT_ERR_INVALID, "too many rows");
  const uint64_t na = n_rows ? off_a[n_rows] : 0, nb = n_rows ? off_b[n_rows] : 0;
  if ((na && !ids_a) || (nb && !ids_b)) return fail(SWT_ERR_INVALID, "null argument");
  for (uint64_t r = 0; r < n_rows; r++)
    if (off_a[r] > off_a[r + 1] || off_b[r] > off_b[r + 1]) return fail(SWT_ERR_INVALID, "row offsets must not decrease");
  int rc = ensure_device();
  if (rc) return rc;
  const size_t ma = (size_t)n_map_a * (flagged_a ? 2 : 1), mb = (size_t)n_map_b * (flagged_b ? 2 : 1);
  DevBuf d[9];  // ids, offsets, map of a; of b; weight; totals; per_row
  struct Guard { DevBuf *d; ~Guard() { for (int i = 0; i < 9; i++) d[i].release(); } } guard{d};
  const void *src[7] = {ids_a, off_a, map_a, ids_b, off_b, map_b, weight};
  const size_t bytes[7] = {(size_t)na * 4, (size_t)(n_rows + 1) * 8, ma * 4, (size_t)nb * 4, (size_t)(n_rows + 1) * 8, mb * 4, (size_t)n_rows * 4};
  for (int i = 0; i < 7; i++) {
    if (!src[i] || !bytes[i] || (!n_rows && i != 2 && i != 5)) continue;
    if ((rc = d[i].reserve(bytes[i] + 16))) return rc;
    SWT_HIP(hipMemcpy(d[i].p, src[i], bytes[i], hipMemcpyHostToDevice));
  }
  if ((rc = d[7].reserve(5 * 8)) || (per_row && n_rows && (rc = d[8].reserve((size_t)n_rows * 16)))) return rc;
  if ((rc = swt_token_equivalence_dev(d[0].as<uint32_t>(), d[1].as<uint64_t>(), d[2].as<uint32_t>(), map_base_a, n_map_a, flagged_a,
                                      d[3].as<uint32_t>(), d[4].as<uint64_t>(), d[5].as<uint32_t>(), map_base_b, n_map_b, flagged_b,
                                      n_rows, weight ? d[6].as<uint32_t>() : nullptr, d[7].as<uint64_t>(), per_row ? d[8].as<uint32_t>() : nullptr, nullptr)))
    return rc;
  SWT_HIP(hipStreamSynchronize(nullptr));
  SWT_HIP(hipMemcpy(totals, d[7].p, 5 * 8, hipMemcpyDeviceToHost));
  if (per_row && n_rows) SWT_HIP(hipMemcpy(per_row, d[8].p, (size_t)n_rows * 16, hipMemcpyDeviceToHost));
  return SWT_OK;
} SWT_API_CATCH

}  // extern "C"
