// swt_pack.hip -- packed batches on the device: several short rows of the CSR pair (ids, tok_off) share one model row, with the
// position of every column inside its segment and the segment / source-row numbers a model needs to keep attention inside a
// sentence.  Semantics: include/swt.h; the design and its measurements: DESIGN.md 4.11.
//
// A source row r gives a segment [cls?] body [sep?] of L(r) columns; P = the exclusive sum of L.
//
// plan   pack_len_kernel leaves L(r) in the workspace and the longest source row in info[1] (one atomicMax per wavefront);
//        launch_scan_u64 (swt_tile.h) scans it in groups of kBtScanGroup and pack_base_kernel makes P[n_rows + 1] of it -- in
//        SPLIT straight into slot, which P is.
//   SPLIT  pack_base_kernel also writes row_first: a segment owns the packed rows whose column 0 it holds.
//   WHOLE  next(r) = the largest q with P[q] - P[r] <= width (a search in P); the packed rows are the orbit of 0 under next.
//          pack_orbit_kernel, one workgroup per group of kPkGroup consecutive rows: pointer doubling in LDS gives every row of
//          the group (the row at which its path leaves the group, the packed rows started on the way, the last of them) in
//          log2 kPkGroup rounds.  pack_walk_kernel, one lane: one step per GROUP, not per row -- where the orbit enters each
//          group, the packed rows before it and the packed row that is open when the group begins (a packed row can span
//          many groups: the exit is a row number); its workgroup fetches the heads of sixteen groups ahead in one round trip.  pack_mark_kernel, per group again: the rows the orbit visits from the
//          entry, marked through the doubling tables from the longest jump down; a count scan and a max scan over the marks
//          give every row its packed row and that row's first source row, hence slot and row_first.
// rows   pack_rows_kernel<kSplit>: PACKED-row-major -- a group of lanes per packed row (swt_rows.h).  A lane finds the segment
//        of its column by a galloping search in slot from the packed row's first source row (one probe while it stays in a
//        segment).  One writer per output row, the aligned 16-byte stores kept, no atomics on the data path, and no store
//        depends on what slot or row_first hold: a group writes the columns of its own row b < min(rows, rows_cap) and nothing
//        else.  The counters of info are added once per workgroup.
#include "swt_batch.h"

namespace swt {

constexpr int kPkThreads = 256;
constexpr int kPkWaves = kPkThreads / 64;
constexpr uint32_t kPkGroup = 1024;     // rows of one group of the orbit step: one workgroup, one row per thread
constexpr uint32_t kPkRounds = 10;      // log2 kPkGroup
constexpr uint32_t kPkNone = 0xFFFFFFFFu;
constexpr uint32_t kPkKinds = SWT_PACK_WHOLE | SWT_PACK_SPLIT;  // the bits of a mode that say which packing
constexpr uint32_t kPkFlags = SWT_BATCH_IDS64;

// The columns of a segment of n tokens.
__host__ __device__ inline uint64_t pk_len(uint64_t n, bool split, uint32_t cap, uint32_t n_special) {
  return (split || n < cap ? n : cap) + n_special;
}

// The largest r in [lo, hi) with a[r] <= x, for an array that does not decrease and a[lo] <= x; lo < hi.  It gallops away from
// lo, so a hit next to lo costs one probe.  Whatever a holds, the result lies in [lo, hi).
__device__ inline uint64_t pk_find(const unsigned long long *__restrict__ a, uint64_t lo, uint64_t hi, unsigned long long x) {
  uint64_t step = 1;
  while (step < hi - lo && a[lo + step] <= x) { lo += step; step <<= 1; }
  uint64_t top = step < hi - lo ? lo + step : hi;  // a[top] > x, or top == hi
  while (top - lo > 1) {
    const uint64_t mid = lo + (top - lo) / 2;
    if (a[mid] <= x) lo = mid; else top = mid;
  }
  return lo;
}

// The packed rows of a plan whose last segment ends at flat position `end`.
__host__ __device__ inline uint64_t pk_rows(unsigned long long end, uint32_t width, uint32_t mode, uint64_t n_rows) {
  if (!n_rows) return 0;
  if (mode & SWT_PACK_SPLIT) return (mode & SWT_PACK_DROP_LAST) ? end / width : (end + width - 1) / width;
  const uint64_t rows = (end + width - 1) / width;
  return rows ? rows : 1;  // nothing but empty segments: one row of padding
}

// Plan, first pass: the segment lengths, and info[1] = the longest source row.
__global__ __launch_bounds__(kPkThreads) void pack_len_kernel(const uint64_t *__restrict__ tok_off, uint64_t n_rows, int split, uint32_t cap,
                                                              uint32_t n_special, unsigned long long *__restrict__ len,
                                                              unsigned long long *__restrict__ info) {
  const uint64_t i = (uint64_t)blockIdx.x * kPkThreads + threadIdx.x;
  unsigned long long n = 0;
  if (i < n_rows) {
    uint64_t first;
    n = bt_tokens(tok_off, i, first);
    len[i] = pk_len(n, split != 0, cap, n_special);
  }
  for (int d = 32; d; d >>= 1) {
    const unsigned long long o = __shfl_xor(n, d, 64);
    n = o > n ? o : n;
  }
  // most wavefronts find a row as long as theirs already there: a look before the atomic
  if ((threadIdx.x & 63) == 0 && n > __hip_atomic_load(&info[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&info[1], n);
}

// Plan, after the scan: P[i] = the group base on top of the scan inside the group; the total (info[3]) closes the array.  SPLIT
// (row_first given; P is slot): a segment also names itself the owner of every packed row whose column 0 it holds -- of the first
// n_rows + 1 packed rows: row_first has no more entries -- the entries from the last packed row on are n_rows, info[0] = the
// packed rows.
__global__ __launch_bounds__(kPkThreads) void pack_base_kernel(const unsigned long long *__restrict__ local,
                                                               const unsigned long long *__restrict__ blk_base,
                                                               const unsigned long long *__restrict__ len, uint64_t n_rows, uint32_t width,
                                                               uint32_t mode, unsigned long long *__restrict__ P,
                                                               unsigned long long *__restrict__ row_first, unsigned long long *__restrict__ info) {
  const uint64_t i = (uint64_t)blockIdx.x * kPkThreads + threadIdx.x;
  if (i > n_rows) return;
  const unsigned long long at = i < n_rows ? blk_base[i / kBtScanGroup] + local[i] : info[3];
  P[i] = at;
  if (!row_first) return;
  const uint64_t rows = pk_rows(info[3], width, mode, n_rows);
  if (i == 0) info[0] = rows;
  if (i >= rows) row_first[i] = n_rows;
  if (i == n_rows) return;
  const uint64_t top = rows < n_rows + 1 ? rows : n_rows + 1;
  for (uint64_t b = (at + width - 1) / width; b < top && b * width < at + len[i]; b++) row_first[b] = i;
}

// The doubling tables of one group of rows [g0, g1): jump[k][i] = the row of the group (its index) that 2^k steps of next lead
// to from row g0 + i, kPkGroup once the path has left the group.  With kFold also, per row: the row at which its path leaves
// the group, the packed rows it starts on the way (itself included) and the last of them.
struct OrbitLds {
  uint16_t jump[kPkRounds][kPkGroup];
};

template <bool kFold>
__device__ inline void pk_double(OrbitLds &S, const uint32_t *__restrict__ next, uint64_t g0, uint64_t g1, uint32_t (&fold)[3],
                                 uint32_t (*__restrict__ tab)[3]) {
  const uint32_t i = threadIdx.x;
  const bool have = g0 + i < g1;
  const uint32_t nx = have ? next[g0 + i] : 0;
  S.jump[0][i] = have && nx < g1 ? (uint16_t)(nx - g0) : (uint16_t)kPkGroup;
  if constexpr (kFold) {
    fold[0] = nx; fold[1] = 1; fold[2] = (uint32_t)(g0 + i);
    tab[i][0] = fold[0]; tab[i][1] = fold[1]; tab[i][2] = fold[2];
  }
  __syncthreads();
  for (uint32_t k = 0; k < kPkRounds; k++) {
    const uint32_t j = S.jump[k][i];
    uint32_t to = kPkGroup, f0 = 0, f1 = 0, f2 = 0;
    if (j < kPkGroup) {
      to = S.jump[k][j];
      if constexpr (kFold) { f0 = tab[j][0]; f1 = tab[j][1]; f2 = tab[j][2]; }
    }
    __syncthreads();  // every row has read what its jump's target held after k rounds
    if (k + 1 < kPkRounds) S.jump[k + 1][i] = (uint16_t)to;
    if constexpr (kFold) {
      if (j < kPkGroup) {
        fold[0] = f0; fold[1] += f1; fold[2] = f2;
        tab[i][0] = fold[0]; tab[i][1] = fold[1]; tab[i][2] = fold[2];
      }
    }
    __syncthreads();
  }
}

// WHOLE: next(r), and per row of the group where its path leaves the group.  After kPkRounds rounds a path has made kPkGroup
// steps, each to a later row: it has left.
__global__ __launch_bounds__(kPkGroup) void pack_orbit_kernel(const unsigned long long *__restrict__ P, uint64_t n_rows, uint32_t width,
                                                              uint32_t *__restrict__ next, uint32_t *__restrict__ exit_row,
                                                              uint32_t *__restrict__ started, uint32_t *__restrict__ last_start) {
  __shared__ OrbitLds S;
  __shared__ uint32_t tab[kPkGroup][3];
  const uint64_t g0 = (uint64_t)blockIdx.x * kPkGroup, r = g0 + threadIdx.x;
  const uint64_t g1 = g0 + kPkGroup < n_rows ? g0 + kPkGroup : n_rows;
  if (r < n_rows) next[r] = (uint32_t)pk_find(P, r, n_rows + 1, P[r] + width);  // > r: a segment is no longer than a row
  __syncthreads();  // the group reads the next of its own rows only: written by this workgroup
  uint32_t fold[3];
  pk_double<true>(S, next, g0, g1, fold, tab);
  if (r < n_rows) { exit_row[r] = fold[0]; started[r] = fold[1]; last_start[r] = fold[2]; }
}

// WHOLE: one step per group.  entry[g] = the row at which the orbit of 0 enters group g (kPkNone: it passes over the group),
// base[g] = the packed rows started before the group, carry[g] = the first source row of the packed row open at its start.
// One lane walks; a step needs what pack_orbit_kernel left for the entry row, a round trip to memory.  The orbit enters a group
// within a packed row's worth of rows of its start, so the workgroup brings the first kPkHead rows of the next kPkAhead groups
// into LDS in ONE round trip and the lane finds most entries there; an entry further in costs its own round trip, as before.
constexpr uint32_t kPkAhead = 16, kPkHead = 64;
__global__ __launch_bounds__(kPkAhead * kPkHead) void pack_walk_kernel(const uint32_t *__restrict__ exit_row, const uint32_t *__restrict__ started,
                                                                     const uint32_t *__restrict__ last_start, uint64_t n_rows,
                                                                     uint32_t *__restrict__ entry, uint32_t *__restrict__ base,
                                                                     uint32_t *__restrict__ carry, unsigned long long *__restrict__ info) {
  __shared__ uint32_t head[kPkAhead][kPkHead][3];
  const uint64_t n_groups = (n_rows + kPkGroup - 1) / kPkGroup;
  const uint32_t w = threadIdx.x / kPkHead, l = threadIdx.x % kPkHead;
  uint64_t e = 0;  // the walking lane's: the next entry, the packed rows so far, the open packed row's first source row
  uint32_t rows = 0, open = 0;
  for (uint64_t g0 = 0; g0 < n_groups; g0 += kPkAhead) {  // uniform: every lane meets every barrier
    const uint64_t row = (g0 + w) * kPkGroup + l;
    if (row < n_rows) { head[w][l][0] = exit_row[row]; head[w][l][1] = started[row]; head[w][l][2] = last_start[row]; }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (uint64_t g = g0; g < g0 + kPkAhead && g < n_groups; g++) {
        const bool enters = e < n_rows && e / kPkGroup == g;
        entry[g] = enters ? (uint32_t)e : kPkNone; base[g] = rows; carry[g] = open;
        if (!enters) continue;
        const uint64_t at = e - g * kPkGroup;
        const bool near = at < kPkHead;
        const uint32_t to = near ? head[g - g0][at][0] : exit_row[e];
        rows += near ? head[g - g0][at][1] : started[e];
        open = near ? head[g - g0][at][2] : last_start[e];
        e = to;
      }
    }
    __syncthreads();  // the next window overwrites head
  }
  if (threadIdx.x == 0) info[0] = rows;
}

// WHOLE: the orbit's rows inside each group, and from them slot and row_first.
__global__ __launch_bounds__(kPkGroup) void pack_mark_kernel(const unsigned long long *__restrict__ P, uint64_t n_rows, uint32_t width,
                                                             const uint32_t *__restrict__ next, const uint32_t *__restrict__ entry,
                                                             const uint32_t *__restrict__ base, const uint32_t *__restrict__ carry,
                                                             const unsigned long long *__restrict__ info,
                                                             unsigned long long *__restrict__ slot, unsigned long long *__restrict__ row_first) {
  __shared__ OrbitLds S;
  __shared__ uint8_t mark[kPkGroup];
  __shared__ uint32_t wave_n[kPkGroup / 64];
  __shared__ int32_t wave_top[kPkGroup / 64];
  const uint32_t i = threadIdx.x, lane = i & 63, wave = i >> 6;
  const uint64_t g0 = (uint64_t)blockIdx.x * kPkGroup, r = g0 + i;
  const uint64_t g1 = g0 + kPkGroup < n_rows ? g0 + kPkGroup : n_rows;
  const uint64_t rows = info[0];
  uint32_t none[3];
  pk_double<false>(S, next, g0, g1, none, nullptr);
  const uint32_t e = entry[blockIdx.x];
  mark[i] = e != kPkNone && e - g0 == i;
  __syncthreads();
  // what the entry reaches in any number of steps below kPkGroup: the jumps of 2^k steps, each taken or not
  for (int k = (int)kPkRounds - 1; k >= 0; k--) {
    const uint32_t j = S.jump[k][i];
    const bool hop = mark[i] && j < kPkGroup;
    __syncthreads();
    if (hop) mark[j] = 1;
    __syncthreads();
  }
  const bool mine = mark[i] != 0;
  const unsigned long long marks = __ballot(mine), upto = marks & (~0ull >> (63 - lane));
  if (lane == 0) {
    wave_n[wave] = (uint32_t)__popcll(marks);
    wave_top[wave] = marks ? (int32_t)(wave * 64 + 63 - __builtin_clzll(marks)) : -1;
  }
  __syncthreads();
  uint32_t k = (uint32_t)__popcll(upto);                                                // marked rows of the group up to this one
  int32_t top = upto ? (int32_t)(wave * 64 + 63 - __builtin_clzll(upto)) : -1;          // the last of them
  for (uint32_t w = 0; w < wave; w++) {
    k += wave_n[w];
    if (!upto && wave_top[w] >= 0) top = wave_top[w];  // none in this wavefront: the nearest one below that has one
  }
  if (r < n_rows) {
    const uint64_t bin = k ? (uint64_t)base[blockIdx.x] + k - 1 : (uint64_t)base[blockIdx.x] - 1;  // k == 0: the row open at the start
    const uint64_t start = k ? g0 + (uint32_t)top : carry[blockIdx.x];
    const unsigned long long at = bin * width + (P[r] - P[start]);
    slot[r] = at;
    if (r + 1 == n_rows) slot[n_rows] = at + (P[n_rows] - P[r]);
    if (mine && bin < n_rows) row_first[bin] = r;  // a packed row has a source row of its own: bin <= r
  }
  // from row_first[rows] on; the entries below are the marked rows'
  if (r < n_rows && r >= rows) row_first[r] = n_rows;
  if (r + 1 == n_rows) row_first[n_rows] = n_rows;
}

struct PackArgs {
  const uint32_t *ids;
  const uint64_t *tok_off;
  uint64_t n_rows;
  const uint32_t *map;
  uint32_t n_map;
  int flagged;
  uint32_t width, cap, flags, mode, pad_id, unk_id, cls_id, sep_id;
  const unsigned long long *slot, *row_first;
  uint64_t rows_cap;
  void *out_ids;
  uint8_t *out_mask;
  uint32_t *out_pos, *out_seg, *out_doc, *out_len;
  unsigned long long *info;
  int vec;         // every output takes the wide stores: the width is a multiple of four and the pointers are aligned
  uint32_t group;  // lanes per packed row: a power of two, 1 .. 64
  uint32_t sets;   // sets of packed rows a wavefront walks
};

template <bool kSplit>
__global__ __launch_bounds__(kPkThreads) void pack_rows_kernel(PackArgs A) {
  __shared__ unsigned long long counts[kPkWaves][2];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t sub = lane & (A.group - 1), per_wave = 64 / A.group;
  const bool ids64 = (A.flags & SWT_BATCH_IDS64) != 0;
  const uint32_t has_cls = A.cls_id != SWT_BATCH_NONE, has_sep = A.sep_id != SWT_BATCH_NONE, n_special = has_cls + has_sep;
  const uint64_t n = A.n_rows;  // >= 1
  uint64_t lim = pk_rows(A.slot[n], A.width, A.mode, n);
  lim = lim < A.rows_cap ? lim : A.rows_cap;
  if (blockIdx.x == 0 && threadIdx.x == 0 && A.info) A.info[0] = lim;
  uint32_t n_unk = 0, n_lost = 0;
  const uint64_t b0 = ((uint64_t)blockIdx.x * kPkWaves + wave) * per_wave * A.sets + lane / A.group;
  for (uint32_t it = 0; it < A.sets; it++) {
    const uint64_t b = b0 + (uint64_t)it * per_wave;
    const bool live = b < lim;
    uint32_t filled = 0;
    if (live) {
      // the source rows [first, last) among which the columns of this row find their segments
      uint64_t first, last = n;
      if constexpr (kSplit) {
        first = pk_find(A.slot, 0, n, (unsigned long long)b * A.width);
      } else {
        first = b < n ? A.row_first[b] : n;
        last = b < n ? A.row_first[b + 1] : n;
        last = last < n ? last : n;
      }
      first = first < last ? first : last;
      const bool any = first < last;
      const uint64_t slot0 = b * A.width;
      uint64_t r = first, tok0 = 0, body = 0;
      unsigned long long at = 0, len = 0;  // the segment of r: where it starts and its columns; len == 0: not loaded
      bool loaded = false, lost = false;
      for (uint32_t c0 = sub * kBtQuad; c0 < A.width; c0 += A.group * kBtQuad) {
        uint32_t id[kBtQuad], ps[kBtQuad], sg[kBtQuad], dc[kBtQuad], mask = 0;
#pragma unroll
        for (uint32_t j = 0; j < kBtQuad; j++) {
          id[j] = A.pad_id; ps[j] = 0; sg[j] = SWT_BATCH_NONE; dc[j] = SWT_BATCH_NONE;
          if (!any || c0 + j >= A.width) continue;
          const unsigned long long x = slot0 + c0 + j;
          const uint64_t q = pk_find(A.slot, r, last, x);
          if (q != r || !loaded) {
            r = q; loaded = true;
            at = A.slot[r];
            const uint64_t tokens = bt_tokens(A.tok_off, r, tok0);
            lost = !kSplit && tokens > A.cap;
            body = kSplit || tokens < A.cap ? tokens : A.cap;
            len = body + n_special;
          }
          const unsigned long long p = x - at;  // the column's position in its segment; wraps to a large value before it
          if (p >= len) continue;               // behind the row's last segment, or a plan that is not one: padding
          mask |= 1u << (8 * j);
          ps[j] = (uint32_t)p; sg[j] = (uint32_t)(r - first); dc[j] = (uint32_t)r;
          filled++;
          if (p == 0 && lost) n_lost++;  // a segment's first column is written once
          if (has_cls && p == 0) { id[j] = A.cls_id; continue; }
          if (has_sep && p == len - 1) { id[j] = A.sep_id; continue; }
          const uint64_t t = tok0 + (p - has_cls);  // p - has_cls < body
          id[j] = bt_dense_id(A.ids[t], A.map, A.n_map, A.flagged, A.unk_id, n_unk);
        }
        const uint64_t o = slot0 + c0;
        if (A.vec) {
          bt_store_quad(A.out_ids, o, ids64, id);
          *reinterpret_cast<uint32_t *>(A.out_mask + o) = mask;
          if (A.out_pos) *reinterpret_cast<uint4 *>(A.out_pos + o) = make_uint4(ps[0], ps[1], ps[2], ps[3]);
          if (A.out_seg) *reinterpret_cast<uint4 *>(A.out_seg + o) = make_uint4(sg[0], sg[1], sg[2], sg[3]);
          if (A.out_doc) *reinterpret_cast<uint4 *>(A.out_doc + o) = make_uint4(dc[0], dc[1], dc[2], dc[3]);
        } else {
#pragma unroll
          for (uint32_t j = 0; j < kBtQuad; j++) {
            if (c0 + j >= A.width) break;
            bt_store_one(A.out_ids, o + j, ids64, id[j]);
            A.out_mask[o + j] = (uint8_t)((mask >> (8 * j)) & 1u);
            if (A.out_pos) A.out_pos[o + j] = ps[j];
            if (A.out_seg) A.out_seg[o + j] = sg[j];
            if (A.out_doc) A.out_doc[o + j] = dc[j];
          }
        }
      }
    }
    for (uint32_t d = A.group >> 1; d; d >>= 1) filled += __shfl_xor(filled, d, 64);  // over the lanes of the row
    if (live && sub == 0 && A.out_len) A.out_len[b] = filled;
  }
  if (!A.info) return;  // uniform over the workgroup
  const uint32_t mine[2] = {n_lost, n_unk};  // info[1], info[2]
  const unsigned long long sum = bt_fold_counts(mine, counts);
  if (sum) atomicAdd(&A.info[1 + threadIdx.x], sum);  // threads 0 and 1 alone have one
}

// what the plan keeps between its launches, grow-only as the scan's workspace and under the same rule
struct PackWorkspace {
  DevBuf len, p, rows32, groups32;  // rows32: next, exit, started, last start; groups32: entry, base, carry
};
static PackWorkspace g_pack_ws;

// The spec and the mode of a call.  *cap_out = the tokens of a segment in WHOLE.
static int pack_check(const swt_batch_spec *spec, uint32_t mode, uint64_t n_rows, uint32_t *cap_out, uint32_t *n_special_out) {
  if (!spec) return fail(SWT_ERR_INVALID, "null argument");
  if (spec->flags & (SWT_BATCH_WINDOWS | SWT_BATCH_PAD_LEFT)) return fail(SWT_ERR_INVALID, "packed rows have no windows and no left padding");
  if (spec->flags & ~kPkFlags) return fail(SWT_ERR_INVALID, "unknown flag");
  if (spec->stride) return fail(SWT_ERR_INVALID, "packed rows have no stride");
  if ((mode & ~(kPkKinds | SWT_PACK_DROP_LAST)) || (mode & kPkKinds) == kPkKinds || !(mode & kPkKinds))
    return fail(SWT_ERR_INVALID, "the mode is SWT_PACK_WHOLE or SWT_PACK_SPLIT");
  if ((mode & SWT_PACK_DROP_LAST) && !(mode & SWT_PACK_SPLIT)) return fail(SWT_ERR_INVALID, "only split packing drops a last row");
  const uint32_t n_special = (spec->cls_id != SWT_BATCH_NONE) + (spec->sep_id != SWT_BATCH_NONE);
  if (spec->width <= n_special) return fail(SWT_ERR_INVALID, "the width leaves no room for a token");
  if (spec->pad_id == SWT_BATCH_NONE || spec->unk_id == SWT_BATCH_NONE) return fail(SWT_ERR_INVALID, "pad_id and unk_id must be ids");
  if (n_rows > 0xFFFFFFFFull) return fail(SWT_ERR_INVALID, "2^32 rows or more");
  *cap_out = spec->width - n_special;
  *n_special_out = n_special;
  return SWT_OK;
}

// The plan of a host form's offsets, row after row: what the device's plan must equal.  slot and row_first may be null.
static uint64_t pack_plan_host(const uint64_t *tok_off, uint64_t n_rows, uint32_t width, uint32_t cap, uint32_t n_special, uint32_t mode,
                               std::vector<uint64_t> *slot, std::vector<uint64_t> *row_first, uint64_t *total) {
  const bool split = (mode & SWT_PACK_SPLIT) != 0;
  if (slot) slot->assign(n_rows + 1, 0);
  if (row_first) row_first->assign(n_rows + 1, n_rows);
  uint64_t sum = 0, bin = 0, used = 0;
  for (uint64_t r = 0; r < n_rows; r++) {
    const uint64_t len = pk_len(tok_off[r + 1] - tok_off[r], split, cap, n_special);
    if (split) {
      if (slot) (*slot)[r] = sum;
      if (row_first && len)
        for (uint64_t b = (sum + width - 1) / width; b * width < sum + len && b <= n_rows; b++) (*row_first)[b] = r;
    } else {
      if (r == 0 || used + len > width) {
        if (r) bin++;
        used = 0;
        if (row_first) (*row_first)[bin] = r;
      }
      if (slot) (*slot)[r] = bin * width + used;
      used += len;
    }
    sum += len;
  }
  const uint64_t end = split ? sum : bin * width + used;
  if (slot) (*slot)[n_rows] = end;
  const uint64_t rows = pk_rows(end, width, mode, n_rows);
  if (row_first)
    for (uint64_t b = rows; b <= n_rows; b++) (*row_first)[b] = n_rows;  // a dropped last row had an owner
  if (total) *total = sum;
  return rows;
}

}  // namespace swt

using namespace swt;

extern "C" {

int swt_pack_capacity(uint32_t *cols_per_step, uint32_t *scan_group, uint32_t *orbit_group) try {
  if (cols_per_step) *cols_per_step = kBtCols;
  if (scan_group) *scan_group = kBtScanGroup;
  if (orbit_group) *orbit_group = kPkGroup;
  return SWT_OK;
} SWT_API_CATCH

int swt_pack_plan_dev(const uint64_t *d_tok_off, uint64_t n_rows, const swt_batch_spec *spec, uint32_t mode, uint64_t *d_slot,
                      uint64_t *d_row_first, uint64_t *d_info, void *stream) try {
  uint32_t cap = 0, n_special = 0;
  int rc = pack_check(spec, mode, n_rows, &cap, &n_special);
  if (rc) return rc;
  if (!d_tok_off || !d_slot || !d_row_first || !d_info) return fail(SWT_ERR_INVALID, "null argument");
  if ((rc = ensure_device())) return rc;
  hipStream_t st = (hipStream_t)stream;
  const bool split = (mode & SWT_PACK_SPLIT) != 0;
  unsigned long long *slot = reinterpret_cast<unsigned long long *>(d_slot), *first = reinterpret_cast<unsigned long long *>(d_row_first);
  unsigned long long *info = reinterpret_cast<unsigned long long *>(d_info);
  SWT_HIP(hipMemsetAsync(d_info, 0, 32, st));
  if (!n_rows) {
    SWT_HIP(hipMemsetAsync(d_slot, 0, 8, st));
    SWT_HIP(hipMemsetAsync(d_row_first, 0, 8, st));
    return SWT_OK;
  }
  PackWorkspace &ws = g_pack_ws;
  const uint64_t nb = (n_rows + kBtScanGroup - 1) / kBtScanGroup, n_groups = (n_rows + kPkGroup - 1) / kPkGroup;
  if ((rc = g_batch_ws.reserve(n_rows))) return rc;
  if ((rc = ws.len.reserve((size_t)n_rows * 8 + 16))) return rc;
  if (!split) {
    if ((rc = ws.p.reserve((size_t)(n_rows + 1) * 8))) return rc;
    if ((rc = ws.rows32.reserve((size_t)n_rows * 16))) return rc;
    if ((rc = ws.groups32.reserve((size_t)n_groups * 12))) return rc;
  }
  unsigned long long *len = ws.len.as<unsigned long long>(), *local = g_batch_ws.local.as<unsigned long long>();
  unsigned long long *blk = g_batch_ws.blk.as<unsigned long long>(), *P = split ? slot : ws.p.as<unsigned long long>();
  const unsigned grid = (unsigned)((n_rows + 1 + kPkThreads - 1) / kPkThreads);
  hipLaunchKernelGGL(pack_len_kernel, dim3(grid), dim3(kPkThreads), 0, st, d_tok_off, n_rows, split ? 1 : 0, cap, n_special, len, info);
  launch_scan_u64(n_rows, len, local, blk, d_info + 3, st);
  hipLaunchKernelGGL(pack_base_kernel, dim3(grid), dim3(kPkThreads), 0, st, local, blk + 1 + nb, len, n_rows, spec->width, mode, P,
                     split ? first : nullptr, info);
  if (!split) {
    uint32_t *next = ws.rows32.as<uint32_t>(), *exit_row = next + n_rows, *started = exit_row + n_rows, *last_start = started + n_rows;
    uint32_t *entry = ws.groups32.as<uint32_t>(), *base = entry + n_groups, *carry = base + n_groups;
    hipLaunchKernelGGL(pack_orbit_kernel, dim3((unsigned)n_groups), dim3(kPkGroup), 0, st, P, n_rows, spec->width, next, exit_row, started,
                       last_start);
    hipLaunchKernelGGL(pack_walk_kernel, dim3(1), dim3(kPkAhead * kPkHead), 0, st, exit_row, started, last_start, n_rows, entry, base, carry, info);
    hipLaunchKernelGGL(pack_mark_kernel, dim3((unsigned)n_groups), dim3(kPkGroup), 0, st, P, n_rows, spec->width, next, entry, base, carry,
                       info, slot, first);
  }
  SWT_HIP(hipGetLastError());
  return SWT_OK;
} SWT_API_CATCH

int swt_pack_plan(const uint64_t *tok_off, uint64_t n_rows, const swt_batch_spec *spec, uint32_t mode, uint64_t *slot, uint64_t *row_first,
                  uint64_t *info) try {
  uint32_t cap = 0, n_special = 0;
  int rc = pack_check(spec, mode, n_rows, &cap, &n_special);
  if (rc) return rc;
  if (!tok_off || !slot || !row_first || !info) return fail(SWT_ERR_INVALID, "null argument");
  for (uint64_t r = 0; r < n_rows; r++)
    if (tok_off[r] > tok_off[r + 1]) return fail(SWT_ERR_INVALID, "offsets must not decrease");
  if ((rc = ensure_device())) return rc;
  BatchStage s;
  const size_t off_bytes = (size_t)(n_rows + 1) * 8;
  const uint64_t *d_off = s.in(tok_off, off_bytes);
  uint64_t *d_slot = s.out(slot, off_bytes), *d_first = s.out(row_first, off_bytes), *d_info = s.out(info, 32);
  if (s.rc) return s.rc;
  if ((rc = swt_pack_plan_dev(d_off, n_rows, spec, mode, d_slot, d_first, d_info, nullptr))) return rc;
  return s.fetch();
} SWT_API_CATCH

int swt_pack_rows_dev(const uint32_t *d_ids, const uint64_t *d_tok_off, uint64_t n_rows, const uint32_t *d_map, uint32_t n_map, int flagged,
                      const swt_batch_spec *spec, uint32_t mode, const uint64_t *d_slot, const uint64_t *d_row_first, uint64_t rows_cap,
                      void *d_out_ids, uint8_t *d_out_mask, uint32_t *d_out_pos, uint32_t *d_out_seg, uint32_t *d_out_doc,
                      uint32_t *d_out_len, uint64_t *d_info, void *stream) try {
  uint32_t cap = 0, n_special = 0;
  int rc = pack_check(spec, mode, n_rows, &cap, &n_special);
  if (rc) return rc;
  if (!d_out_ids || !d_out_mask) return fail(SWT_ERR_INVALID, "null argument");
  if (flagged && !d_map) return fail(SWT_ERR_INVALID, "a flagged stream needs a map");
  if (n_rows && (!d_tok_off || !d_ids || !d_slot || !d_row_first)) return fail(SWT_ERR_INVALID, "null argument");
  const uintptr_t id_bytes = (spec->flags & SWT_BATCH_IDS64) ? 8 : 4;
  if (!bt_aligned(id_bytes, {d_out_ids}) || !bt_aligned(4, {d_out_pos, d_out_seg, d_out_doc, d_out_len}) || !bt_aligned(8, {d_info}))
    return fail(SWT_ERR_INVALID, "an output is not aligned to its element type");
  if ((rc = ensure_device())) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (d_info) SWT_HIP(hipMemsetAsync(d_info, 0, 24, st));
  if (!n_rows || !rows_cap) return SWT_OK;
  PackArgs A{d_ids, d_tok_off, n_rows, d_map, n_map, flagged ? 1 : 0, spec->width, cap, spec->flags, mode, spec->pad_id, spec->unk_id,
             spec->cls_id, spec->sep_id, reinterpret_cast<const unsigned long long *>(d_slot),
             reinterpret_cast<const unsigned long long *>(d_row_first), rows_cap, d_out_ids, d_out_mask, d_out_pos, d_out_seg, d_out_doc,
             d_out_len, reinterpret_cast<unsigned long long *>(d_info), 0, 1, 1};
  A.vec = A.width % kBtQuad == 0 && bt_aligned(16, {d_out_ids, d_out_pos, d_out_seg, d_out_doc}) && bt_aligned(4, {d_out_mask});
  A.group = bt_group(A.width);
  // the packed rows are known to the device alone: room for rows_cap of them, which nothing bounds: the sets must fit their field
  const RowShape shape = bt_shape(rows_cap, A.group, kPkWaves);
  if (shape.sets > 0xFFFFFFFFull) return fail(SWT_ERR_INVALID, "2^32 rows or more");
  A.sets = (uint32_t)shape.sets;
  prof_begin(st);
  if (mode & SWT_PACK_SPLIT) hipLaunchKernelGGL(pack_rows_kernel<true>, dim3(shape.grid), dim3(kPkThreads), 0, st, A);
  else hipLaunchKernelGGL(pack_rows_kernel<false>, dim3(shape.grid), dim3(kPkThreads), 0, st, A);
  prof_end(st);
  SWT_HIP(hipGetLastError());
  return SWT_OK;
} SWT_API_CATCH

int swt_pack_rows(const uint32_t *ids, const uint64_t *tok_off, uint64_t n_rows, const uint32_t *map, uint32_t n_map, int flagged,
                  const swt_batch_spec *spec, uint32_t mode, const uint64_t *slot, const uint64_t *row_first, uint64_t rows_cap, void *out_ids,
                  uint8_t *out_mask, uint32_t *out_pos, uint32_t *out_seg, uint32_t *out_doc, uint32_t *out_len, uint64_t *info) try {
  uint32_t cap = 0, n_special = 0;
  int rc = pack_check(spec, mode, n_rows, &cap, &n_special);
  if (rc) return rc;
  if (!out_ids || !out_mask) return fail(SWT_ERR_INVALID, "null argument");
  if (flagged && !map) return fail(SWT_ERR_INVALID, "a flagged stream needs a map");
  if (n_rows && (!tok_off || !slot || !row_first)) return fail(SWT_ERR_INVALID, "null argument");
  for (uint64_t r = 0; r < n_rows; r++)
    if (tok_off[r] > tok_off[r + 1]) return fail(SWT_ERR_INVALID, "offsets must not decrease");
  std::vector<uint64_t> want_slot, want_first;
  const uint64_t need = pack_plan_host(tok_off, n_rows, spec->width, cap, n_special, mode, &want_slot, &want_first, nullptr);
  for (uint64_t r = 0; n_rows && r <= n_rows; r++)
    if (slot[r] != want_slot[r] || row_first[r] != want_first[r]) return fail(SWT_ERR_INVALID, "slot and row_first are not the plan of these offsets");
  const uint64_t n_tok = n_rows ? tok_off[n_rows] : 0;
  if (n_tok && !ids) return fail(SWT_ERR_INVALID, "null argument");
  if (info) { info[0] = need; info[1] = 0; info[2] = 0; }
  if (need > rows_cap) return fail(SWT_ERR_CAPACITY, "%llu rows needed, room for %llu", (unsigned long long)need, (unsigned long long)rows_cap);
  if (!n_rows || !need) return SWT_OK;
  if ((rc = ensure_device())) return rc;
  const size_t slots = (size_t)need * spec->width, n_map_all = map ? (size_t)n_map * (flagged ? 2 : 1) : 0;
  const size_t id_bytes = (spec->flags & SWT_BATCH_IDS64) ? 8 : 4, off_bytes = (size_t)(n_rows + 1) * 8;
  BatchStage s;
  const uint32_t *d_ids = s.in(ids, n_tok * 4, true), *d_map = s.in(map, n_map_all * 4);
  const uint64_t *d_off = s.in(tok_off, off_bytes), *d_slot = s.in(slot, off_bytes), *d_first = s.in(row_first, off_bytes);
  void *d_out = s.out(out_ids, slots * id_bytes);
  uint8_t *d_mask = s.out(out_mask, slots);
  uint32_t *d_pos = s.out(out_pos, slots * 4), *d_seg = s.out(out_seg, slots * 4), *d_doc = s.out(out_doc, slots * 4);
  uint32_t *d_len = s.out(out_len, (size_t)need * 4);
  uint64_t *d_info = s.out(info, 24);
  if (s.rc) return s.rc;
  if ((rc = swt_pack_rows_dev(d_ids, d_off, n_rows, d_map, n_map, flagged, spec, mode, d_slot, d_first, need, d_out, d_mask, d_pos, d_seg,
                              d_doc, d_len, d_info, nullptr)))
    return rc;
  return s.fetch();
} SWT_API_CATCH

}  // extern "C"
