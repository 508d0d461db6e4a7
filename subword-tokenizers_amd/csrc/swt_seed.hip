// swt_seed.hip -- the substring census behind UnigramWP.seed_substrings (include/swt.h, swt_substring_counts).
//
// Kudo 2018 seeds the unigram trainer with the corpus's most frequent substrings.  Over the unique words of swt_words.hip
// (code points, CSR offsets, frequencies) every (word, start i, length l in 2..L) is one insertion of the key
// (i > 0, c[i..i+l)) with the word's frequency:
//   count    one wave per tile of kSeedTile consecutive START positions of the symbol stream, whatever words they lie in.
//            The tile's code points and the kSeedHalo behind them go to LDS with a bitmap of the word starts and, at every
//            start, the word's frequency (0 for a word longer than max_word).  A lane takes one start per step, finds its
//            word's start (the boundary bit at or below it) and end (the next bit above it), and extends a 64-bit rolling
//            hash one code point at a time: one multiply-add, one mix and one find-or-insert per length.
//   table    global, open addressing, linear probing.  A slot is one 64-bit word [tag:16 | flag:1 | length-1:5 | offset of
//            a representative occurrence in sym:42], claimed with one atomicCAS; a hit is confirmed by comparing the code
//            points with the representative's (sym is input: the compare races with nothing).  Counts are a separate
//            uint64 array under atomicAdd.
//   compact  select: the slots with count >= min_count draw their entry numbers from one cursor per wave (ballot + one
//            atomicAdd) and write length, flag and count; rocPRIM scans the lengths into offsets; emit copies the code points.
#include <rocprim/device/device_scan.hpp>

#include "swt_words.h"

namespace swt {

constexpr int kSeedTile = 1024;                      // start positions of one wavefront
constexpr int kSeedMaxChars = 32;                    // the largest L
constexpr int kSeedHalo = kSeedMaxChars - 1;         // positions staged behind a tile: its last start reaches that far
constexpr int kSeedStage = kSeedTile + kSeedHalo;
constexpr int kSeedMaskWords = (kSeedStage + 63) / 64;
constexpr unsigned long long kSeedEmpty = ~0ull;
constexpr int kSeedOffBits = 42;
constexpr unsigned long long kSeedOffMask = (1ull << kSeedOffBits) - 1ull;
constexpr unsigned long long kSeedMul = 0x9E3779B97F4A7C15ull;  // odd: the rolling hash is h * kSeedMul + (code point + 1)
constexpr uint64_t kSeedMaxSyms = 1ull << 40;                   // far below the offset field: no slot equals kSeedEmpty
enum { kCtlInsertions = 0, kCtlClaimed = 1, kCtlFull = 2, kCtlEntries = 3, kCtlCps = 4, kCtlWords = 8 };

struct SeedTable {
  unsigned long long *slot;  // tag:16 | flag:1 | length-1:5 | representative offset:42
  unsigned long long *cnt;   // sum of the frequencies
  unsigned long long *ctl;   // kCtl*
  uint32_t bits;
};

// find-or-insert one (start, length): `mine` = its code points in LDS, gpos = its offset in sym, h = the rolling hash.
// -> 2: this occurrence became the representative, 1: found, 0: the table is full (kCtlFull is set)
__device__ int seed_insert(const SeedTable &T, const uint32_t *__restrict__ sym, const uint32_t *mine, uint32_t len, bool inner,
                           uint64_t gpos, unsigned long long h, uint32_t f) {
  h ^= h >> 29; h *= 0xBF58476D1CE4E5B9ull; h ^= h >> 32;
  const uint32_t mask = (1u << T.bits) - 1u;
  const unsigned long long head = ((h >> 48) << 48) | ((unsigned long long)inner << 47) | ((unsigned long long)(len - 1u) << kSeedOffBits);
  const unsigned long long packed = head | gpos;
  uint32_t idx = (uint32_t)h & mask;
  for (uint32_t probes = 0; probes <= mask; probes++) {
    unsigned long long v = __hip_atomic_load(&T.slot[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (v == kSeedEmpty) {
      v = atomicCAS(&T.slot[idx], kSeedEmpty, packed);
      if (v == kSeedEmpty) {
        atomicAdd(&T.cnt[idx], (unsigned long long)f);
        return 2;
      }
    }
    // an occupied slot, or the value that won the race for it: the same key only after the exact compare
    if ((v & ~kSeedOffMask) == head) {
      const uint32_t *rep = sym + (v & kSeedOffMask);
      bool same = true;
      for (uint32_t i = 0; i < len; i++)
        if (rep[i] != mine[i]) { same = false; break; }
      if (same) {
        atomicAdd(&T.cnt[idx], (unsigned long long)f);
        return 1;
      }
    }
    idx = (idx + 1) & mask;
    // a full table was found by another lane: the call fails whatever this one does
    if ((probes & 63u) == 63u && __hip_atomic_load(&T.ctl[kCtlFull], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return 0;
  }
  atomicOr(&T.ctl[kCtlFull], 1ull);  // every slot holds another key
  return 0;
}

struct SeedLds {
  uint32_t cp[kSeedStage + 1];
  uint32_t wfreq[kSeedStage + 1];                  // at a word start: the word's frequency, 0 when the word is barred
  unsigned long long bound[kSeedMaskWords + 1];    // bit r: a (non-empty) word starts at staged position r
};

// count_only: tally the insertions (sizes the table); otherwise make them
__global__ __launch_bounds__(64) void seed_count_kernel(const uint32_t *__restrict__ sym, const uint64_t *__restrict__ word_off,
                                                        const uint32_t *__restrict__ freq, uint64_t n_words, uint64_t n_syms,
                                                        uint32_t max_chars, uint32_t max_word, SeedTable T, bool count_only) {
  __shared__ SeedLds L;
  const int lane = threadIdx.x;
  const uint64_t base = (uint64_t)blockIdx.x * kSeedTile;
  if (base >= n_syms) return;
  if (!count_only && __hip_atomic_load(&T.ctl[kCtlFull], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
  const uint64_t lim = base + kSeedStage < n_syms ? base + kSeedStage : n_syms;
  const uint32_t staged = (uint32_t)(lim - base);
  const uint32_t tile_n = staged < (uint32_t)kSeedTile ? staged : (uint32_t)kSeedTile;
  for (uint32_t c = lane; c < staged; c += 64) L.cp[c] = sym[base + c];
  if (lane <= kSeedMaskWords) L.bound[lane] = 0ull;
  // the word that holds `base`: the last one whose offset is <= base (so it is not empty); word_off[0] = 0 <= base < word_off[n_words]
  uint64_t w_lo = 0, w_hi = n_words;
  while (w_hi - w_lo > 1) {
    const uint64_t mid = w_lo + ((w_hi - w_lo) >> 1);
    if (word_off[mid] <= base) w_lo = mid; else w_hi = mid;
  }
  const uint64_t o_lo = word_off[w_lo], e_lo = word_off[w_lo + 1];
  const uint32_t f_lo = (max_word && e_lo - o_lo > max_word) ? 0u : freq[w_lo];
  __syncthreads();
  // the words that start inside the staged range, one lane each
  for (uint64_t w = w_lo + lane; w < n_words; w += 64) {
    const uint64_t o = word_off[w];
    if (o >= lim) break;
    const uint64_t o1 = word_off[w + 1];
    if (o1 <= o || o < base) continue;  // an empty word, or the one that began before the tile (f_lo speaks for it)
    const uint32_t r = (uint32_t)(o - base);
    atomicOr(&L.bound[r >> 6], 1ull << (r & 63));
    L.wfreq[r] = (max_word && o1 - o > max_word) ? 0u : freq[w];
  }
  __syncthreads();

  unsigned long long tally = 0;  // insertions (count_only) or slots claimed
  for (uint32_t r0 = 0; r0 < tile_n; r0 += 64) {
    const uint32_t r = r0 + lane;
    if (r >= tile_n) continue;
    // the start of r's word: the boundary bit at or below r; none: the word began before the tile
    uint32_t wq = r >> 6;
    unsigned long long m = L.bound[wq] & (~0ull >> (63 - (r & 63)));
    while (!m && wq > 0) m = L.bound[--wq];
    const uint32_t s = m ? wq * 64 + 63 - (uint32_t)__builtin_clzll(m) : 0xFFFFFFFFu;
    const uint32_t f = m ? L.wfreq[s] : f_lo;
    const bool inner = s != r;  // i > 0: the '##' of the WordPiece spelling
    // its end, as far as a piece can reach: the next boundary bit above r (within max_chars it lies in this mask word or the next)
    uint32_t e = r + max_chars < staged ? r + max_chars : staged;
    if (r + 1 < staged) {
      wq = (r + 1) >> 6;
      m = L.bound[wq] & (~0ull << ((r + 1) & 63));
      if (!m) m = L.bound[++wq];
      if (m) {
        const uint32_t nb = wq * 64 + (uint32_t)__builtin_ctzll(m);
        if (nb < e) e = nb;
      }
    }
    const uint32_t lmax = e - r;
    if (!f || lmax < 2) continue;
    if (count_only) {
      tally += lmax - 1;
      continue;
    }
    unsigned long long h = (inner ? 0x2545F4914F6CDD1Dull : 0xD6E8FEB86659FD93ull) * kSeedMul + (L.cp[r] + 1u);
    for (uint32_t l = 2; l <= lmax; l++) {
      h = h * kSeedMul + (L.cp[r + l - 1] + 1u);
      const int got = seed_insert(T, sym, &L.cp[r], l, inner, base + r, h, f);
      if (!got) break;
      tally += got == 2;
    }
  }
  for (int d = 32; d >= 1; d >>= 1) tally += __shfl_xor(tally, d);
  if (lane == 0 && tally) atomicAdd(&T.ctl[count_only ? kCtlInsertions : kCtlClaimed], tally);
}

__global__ void seed_fill_kernel(unsigned long long *slot, unsigned long long *cnt, uint64_t n) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    slot[i] = kSeedEmpty;
    cnt[i] = 0ull;
  }
}

// the slots with count >= min_count, in no particular order: entry k gets its slot (sel), length (in out_len, scanned into the
// offsets afterwards), flag and count; nothing is written at or past out_cap, the cursors count on
__global__ __launch_bounds__(256) void seed_select_kernel(SeedTable T, unsigned long long min_count, uint32_t *__restrict__ sel,
                                                          uint64_t *__restrict__ out_len, uint8_t *__restrict__ out_flag,
                                                          uint64_t *__restrict__ out_count, uint64_t out_cap) {
  const uint64_t cap = 1ull << T.bits;
  const int lane = threadIdx.x & 63;
  const unsigned long long lt = (1ull << lane) - 1ull;
  const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
  for (uint64_t i0 = wave * 64; i0 < cap; i0 += n_waves * 64) {
    const uint64_t i = i0 + lane;
    const unsigned long long v = i < cap ? T.slot[i] : kSeedEmpty;
    const unsigned long long c = v != kSeedEmpty ? T.cnt[i] : 0ull;
    const bool keep = v != kSeedEmpty && c >= min_count;
    const uint32_t len = keep ? (uint32_t)((v >> kSeedOffBits) & 31u) + 1u : 0u;
    const unsigned long long KEEP = __ballot(keep);
    if (!KEEP) continue;
    uint32_t cps = len;
    for (int d = 32; d >= 1; d >>= 1) cps += __shfl_xor(cps, d);
    unsigned long long k0 = 0;
    if (lane == 0) {
      k0 = atomicAdd(&T.ctl[kCtlEntries], (unsigned long long)__popcll(KEEP));
      atomicAdd(&T.ctl[kCtlCps], (unsigned long long)cps);
    }
    k0 = __shfl(k0, 0);
    const uint64_t k = k0 + __popcll(KEEP & lt);
    if (keep && k < out_cap) {
      sel[k] = (uint32_t)i;
      out_len[k] = len;
      out_flag[k] = (uint8_t)((v >> 47) & 1u);
      out_count[k] = c;
    }
  }
}

__global__ void seed_emit_kernel(const uint32_t *__restrict__ sym, SeedTable T, const uint32_t *__restrict__ sel, uint64_t n,
                                 const uint64_t *__restrict__ out_off, uint32_t *__restrict__ out_cps) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const unsigned long long v = T.slot[sel[k]];
  const uint32_t *rep = sym + (v & kSeedOffMask);
  const uint32_t len = (uint32_t)((v >> kSeedOffBits) & 31u) + 1u;
  uint32_t *o = out_cps + out_off[k];
  for (uint32_t i = 0; i < len; i++) o[i] = rep[i];
}

struct SeedArgs {
  uint32_t max_chars;
  uint64_t min_count;
  uint32_t max_word, table_bits;
};
struct SeedOut {  // device pointers
  uint64_t *off;
  uint32_t *cps;
  uint8_t *flag;
  uint64_t *count;
  uint64_t out_cap, cps_cap;
};

static int seed_check(const SeedArgs &A, const void *off, const void *cps, const void *flag, const void *count, uint64_t out_cap,
                      uint64_t cps_cap, const uint64_t *n_out, const uint64_t *n_cps) {
  if (!n_out || !n_cps) return fail(SWT_ERR_INVALID, "null argument");
  if (A.max_chars < 2 || A.max_chars > (uint32_t)kSeedMaxChars) return fail(SWT_ERR_INVALID, "max_chars lies in 2..%d", kSeedMaxChars);
  if (A.min_count < 1) return fail(SWT_ERR_INVALID, "min_count is at least 1");
  if (A.max_word > 1024) return fail(SWT_ERR_INVALID, "max_word is 0 or lies in 1..1024");
  if (A.table_bits && (A.table_bits < 4 || A.table_bits > 30)) return fail(SWT_ERR_INVALID, "table_bits is 0 or lies in 4..30");
  if (out_cap && (!off || !flag || !count)) return fail(SWT_ERR_INVALID, "null output with a capacity of %llu", (unsigned long long)out_cap);
  if (cps_cap && !cps) return fail(SWT_ERR_INVALID, "null out_cps with a capacity of %llu", (unsigned long long)cps_cap);
  return SWT_OK;
}

struct DevOwner {  // device allocations of one call
  std::vector<void *> held;
  ~DevOwner() {
    for (void *p : held) (void)hipFree(p);
  }
  template <class P> hipError_t alloc(P **out, size_t bytes) {
    void *p = nullptr;
    const hipError_t e = hipMalloc(&p, bytes ? bytes : 8);
    if (e == hipSuccess) held.push_back(p);
    *out = reinterpret_cast<P *>(p);
    return e;
  }
};

static unsigned seed_grid(uint64_t n, unsigned threads, unsigned cap) {
  uint64_t g = (n + threads - 1) / threads;
  return (unsigned)(g < 1 ? 1 : (g > cap ? cap : g));
}

// the census over device arrays; synchronises `st` (the numbers come back to the host)
static int seed_run(const uint32_t *d_sym, const uint64_t *d_woff, const uint32_t *d_freq, uint64_t n_words, uint64_t n_syms,
                    const SeedArgs &A, const SeedOut &O, uint64_t *n_out, uint64_t *n_cps, hipStream_t st) {
  *n_out = 0;
  *n_cps = 0;
  if (n_syms >= kSeedMaxSyms) return fail(SWT_ERR_UNSUPPORTED, "word list of %llu code points (the limit is 2^40)", (unsigned long long)n_syms);
  if (O.off) SWT_HIP(hipMemsetAsync(O.off, 0, 8, st));
  if (!n_words || !n_syms) {
    SWT_HIP(hipStreamSynchronize(st));
    return SWT_OK;
  }
  DevOwner own;
  SeedTable T{nullptr, nullptr, nullptr, 0};
  unsigned long long ctl[kCtlWords];
  SWT_HIP(own.alloc(&T.ctl, sizeof ctl));
  SWT_HIP(hipMemsetAsync(T.ctl, 0, sizeof ctl, st));
  const unsigned n_tiles = (unsigned)((n_syms + kSeedTile - 1) / kSeedTile);
  prof_begin(st, 2);
  uint32_t bits = A.table_bits;
  if (!bits) {
    // the library's own size: twice the insertions, so that distinct keys <= insertions never fill it
    hipLaunchKernelGGL(seed_count_kernel, dim3(n_tiles), dim3(64), 0, st, d_sym, d_woff, d_freq, n_words, n_syms, A.max_chars, A.max_word, T, true);
    SWT_HIP(hipMemcpyAsync(ctl, T.ctl, 8, hipMemcpyDeviceToHost, st));
    SWT_HIP(hipStreamSynchronize(st));
    if (!ctl[kCtlInsertions]) {
      prof_end(st, 2);
      return SWT_OK;
    }
    bits = 10;
    while (bits <= 30 && (1ull << bits) < 2 * ctl[kCtlInsertions] + 16) bits++;
    if (bits > 30) prof_end(st, 2);
    if (bits > 30)
      return fail(SWT_ERR_UNSUPPORTED, "%llu insertions need a table of more than 2^30 slots", (unsigned long long)ctl[kCtlInsertions]);
  }
  T.bits = bits;
  const uint64_t cap = 1ull << bits;
  SWT_HIP(own.alloc(&T.slot, cap * 8));
  SWT_HIP(own.alloc(&T.cnt, cap * 8));
  hipLaunchKernelGGL(seed_fill_kernel, dim3(seed_grid(cap, 256, 8192)), dim3(256), 0, st, T.slot, T.cnt, cap);
  prof_begin(st);
  hipLaunchKernelGGL(seed_count_kernel, dim3(n_tiles), dim3(64), 0, st, d_sym, d_woff, d_freq, n_words, n_syms, A.max_chars, A.max_word, T, false);
  prof_end(st);
  SWT_HIP(hipMemcpyAsync(ctl, T.ctl, sizeof ctl, hipMemcpyDeviceToHost, st));
  SWT_HIP(hipStreamSynchronize(st));
  // one slot stays empty in a table that is not full, so every probe ended at its key or at an empty slot
  if (ctl[kCtlFull] || ctl[kCtlClaimed] >= cap) {
    prof_end(st, 2);
    return fail(SWT_ERR_NOMEM, "the substring table of 2^%u slots is full: it must keep one slot more than the distinct keys (table_bits = 0 sizes it)", bits);
  }
  uint32_t *d_sel = nullptr;
  const uint64_t sel_n = O.out_cap < cap ? O.out_cap : cap;
  SWT_HIP(own.alloc(&d_sel, sel_n * 4));
  hipLaunchKernelGGL(seed_select_kernel, dim3(seed_grid(cap, 256, 4096)), dim3(256), 0, st, T, (unsigned long long)A.min_count, d_sel, O.off, O.flag,
                     O.count, O.out_cap);
  SWT_HIP(hipMemcpyAsync(ctl, T.ctl, sizeof ctl, hipMemcpyDeviceToHost, st));
  SWT_HIP(hipStreamSynchronize(st));
  *n_out = ctl[kCtlEntries];
  *n_cps = ctl[kCtlCps];
  if (*n_out > O.out_cap || *n_cps > O.cps_cap) {
    prof_end(st, 2);
    return fail(SWT_ERR_CAPACITY, "%llu entries of %llu code points", (unsigned long long)*n_out, (unsigned long long)*n_cps);
  }
  if (*n_out) {
    const size_t n = (size_t)*n_out;
    SWT_HIP(hipMemsetAsync(O.off + n, 0, 8, st));
    size_t tmp_bytes = 0;
    void *d_tmp = nullptr;
    SWT_HIP(rocprim::exclusive_scan(nullptr, tmp_bytes, O.off, O.off, (uint64_t)0, n + 1, rocprim::plus<uint64_t>(), st));
    SWT_HIP(own.alloc(&d_tmp, tmp_bytes + 16));
    SWT_HIP(rocprim::exclusive_scan(d_tmp, tmp_bytes, O.off, O.off, (uint64_t)0, n + 1, rocprim::plus<uint64_t>(), st));
    hipLaunchKernelGGL(seed_emit_kernel, dim3(seed_grid(n, 256, 1u << 22)), dim3(256), 0, st, d_sym, T, d_sel, (uint64_t)n, O.off, O.cps);
  }
  prof_end(st, 2);
  SWT_HIP(hipGetLastError());
  SWT_HIP(hipStreamSynchronize(st));
  return SWT_OK;
}

}  // namespace swt

using namespace swt;

extern "C" {

int swt_substring_counts_capacity(uint32_t *tile, uint32_t *halo, uint32_t *max_chars) try {
  if (tile) *tile = kSeedTile;
  if (halo) *halo = kSeedHalo;
  if (max_chars) *max_chars = kSeedMaxChars;
  return SWT_OK;
} SWT_API_CATCH

int swt_substring_counts_dev(const uint32_t *d_sym, const uint64_t *d_word_off, const uint32_t *d_freq, uint64_t n_words, uint32_t max_chars,
                             uint64_t min_count, uint32_t max_word, uint32_t table_bits, uint64_t *d_out_off, uint32_t *d_out_cps,
                             uint8_t *d_out_flag, uint64_t *d_out_count, uint64_t out_cap, uint64_t cps_cap, uint64_t *n_out, uint64_t *n_cps,
                             void *stream) try {
  const SeedArgs A{max_chars, min_count, max_word, table_bits};
  if (int rc = seed_check(A, d_out_off, d_out_cps, d_out_flag, d_out_count, out_cap, cps_cap, n_out, n_cps)) return rc;
  if (n_words && (!d_word_off || !d_freq)) return fail(SWT_ERR_INVALID, "null argument");
  if (int rc = ensure_device()) return rc;
  hipStream_t st = (hipStream_t)stream;
  uint64_t first = 0, n_syms = 0;
  if (n_words) {
    SWT_HIP(hipMemcpyAsync(&first, d_word_off, 8, hipMemcpyDeviceToHost, st));
    SWT_HIP(hipMemcpyAsync(&n_syms, d_word_off + n_words, 8, hipMemcpyDeviceToHost, st));
    SWT_HIP(hipStreamSynchronize(st));
    if (first != 0) return fail(SWT_ERR_INVALID, "word_off[0] must be 0");
    if (n_syms && !d_sym) return fail(SWT_ERR_INVALID, "null argument");
  }
  return seed_run(d_sym, d_word_off, d_freq, n_words, n_syms, A, SeedOut{d_out_off, d_out_cps, d_out_flag, d_out_count, out_cap, cps_cap}, n_out,
                  n_cps, st);
} SWT_API_CATCH

int swt_substring_counts(const uint32_t *sym, const uint64_t *word_off, const uint32_t *freq, uint64_t n_words, uint32_t max_chars,
                         uint64_t min_count, uint32_t max_word, uint32_t table_bits, uint64_t *out_off, uint32_t *out_cps, uint8_t *out_flag,
                         uint64_t *out_count, uint64_t out_cap, uint64_t cps_cap, uint64_t *n_out, uint64_t *n_cps) try {
  const SeedArgs A{max_chars, min_count, max_word, table_bits};
  if (int rc = seed_check(A, out_off, out_cps, out_flag, out_count, out_cap, cps_cap, n_out, n_cps)) return rc;
  if (n_words && (!word_off || !freq)) return fail(SWT_ERR_INVALID, "null argument");
  uint64_t n_syms = 0;
  if (n_words) {
    if (word_off[0] != 0) return fail(SWT_ERR_INVALID, "word_off[0] must be 0");
    for (uint64_t w = 0; w < n_words; w++)
      if (word_off[w] > word_off[w + 1]) return fail(SWT_ERR_INVALID, "word offsets must be non-decreasing (at %llu)", (unsigned long long)w);
    n_syms = word_off[n_words];
    if (n_syms && !sym) return fail(SWT_ERR_INVALID, "null argument");
  }
  if (int rc = ensure_device()) return rc;
  DevOwner own;
  uint32_t *d_sym = nullptr, *d_freq = nullptr;
  uint64_t *d_woff = nullptr;
  SeedOut O{nullptr, nullptr, nullptr, nullptr, out_cap, cps_cap};
  SWT_HIP(own.alloc(&d_sym, n_syms * 4));
  SWT_HIP(own.alloc(&d_woff, (n_words + 1) * 8));
  SWT_HIP(own.alloc(&d_freq, n_words * 4));
  SWT_HIP(own.alloc(&O.off, (out_cap + 1) * 8));
  SWT_HIP(own.alloc(&O.cps, cps_cap * 4));
  SWT_HIP(own.alloc(&O.flag, out_cap));
  SWT_HIP(own.alloc(&O.count, out_cap * 8));
  if (n_syms) SWT_HIP(hipMemcpy(d_sym, sym, n_syms * 4, hipMemcpyHostToDevice));
  if (n_words) {
    SWT_HIP(hipMemcpy(d_woff, word_off, (n_words + 1) * 8, hipMemcpyHostToDevice));
    SWT_HIP(hipMemcpy(d_freq, freq, n_words * 4, hipMemcpyHostToDevice));
  }
  if (int rc = seed_run(d_sym, d_woff, d_freq, n_words, n_syms, A, O, n_out, n_cps, nullptr)) return rc;
  const uint64_t n = *n_out;
  if (out_off) SWT_HIP(hipMemcpy(out_off, O.off, (n + 1) * 8, hipMemcpyDeviceToHost));
  if (n) {
    SWT_HIP(hipMemcpy(out_cps, O.cps, *n_cps * 4, hipMemcpyDeviceToHost));
    SWT_HIP(hipMemcpy(out_flag, O.flag, n, hipMemcpyDeviceToHost));
    SWT_HIP(hipMemcpy(out_count, O.count, n * 8, hipMemcpyDeviceToHost));
  }
  return SWT_OK;
} SWT_API_CATCH

int swt_substring_counts_text_dev(const uint8_t *d_text, uint64_t n_bytes, const uint64_t *d_sent_off, uint64_t n_sent, uint32_t max_chars,
                                  uint64_t min_count, uint32_t max_word, uint32_t table_bits, uint64_t *d_out_off, uint32_t *d_out_cps,
                                  uint8_t *d_out_flag, uint64_t *d_out_count, uint64_t out_cap, uint64_t cps_cap, uint64_t *n_out,
                                  uint64_t *n_cps, uint32_t *base_out, uint32_t base_cap, uint32_t *n_base, void *stream) try {
  const SeedArgs A{max_chars, min_count, max_word, table_bits};
  if (int rc = seed_check(A, d_out_off, d_out_cps, d_out_flag, d_out_count, out_cap, cps_cap, n_out, n_cps)) return rc;
  if (!d_sent_off || (n_bytes && !d_text) || (base_cap && !base_out)) return fail(SWT_ERR_INVALID, "null argument");
  if (int rc = ensure_device()) return rc;
  hipStream_t st = (hipStream_t)stream;
  SWT_HIP(hipStreamSynchronize(st));  // the census runs on the default stream: what filled the text has to be over
  DeviceWords dw;
  if (int rc = device_words_from_text(d_text, n_bytes, d_sent_off, n_sent, &dw)) return rc;
  DevOwner own;
  own.held = {(void *)dw.d_sym, (void *)dw.d_woff, (void *)dw.d_freq};
  if (n_base) *n_base = (uint32_t)dw.base_syms.size();
  for (size_t i = 0; i < dw.base_syms.size() && i < base_cap; i++) base_out[i] = dw.base_syms[i];
  return seed_run(dw.d_sym, dw.d_woff, dw.d_freq, dw.n_words, dw.n_syms, A, SeedOut{d_out_off, d_out_cps, d_out_flag, d_out_count, out_cap, cps_cap},
                  n_out, n_cps, st);
} SWT_API_CATCH

}  // extern "C"
