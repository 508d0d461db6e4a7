// swt_batch.h -- what the row kernels share (rows_kernel in swt_batch.hip, pack_rows_kernel in swt_pack.hip, mlm_kernel in
// swt_mlm.hip, decode_kernel in swt_decode.hip): the launch geometry (swt_rows.h), the loads and stores of a
// lane's four columns, the dense-id lookup, the fold of a kernel's counts, the scan with its bases and the sum of the
// workgroups' counts (both defined in swt_batch.hip), and the device side of a host form.
#pragma once

#include <deque>
#include <initializer_list>
#include <vector>

#include "swt_rows.h"
#include "swt_tile.h"

namespace swt {

constexpr uint32_t kBtScanGroup = 1024;   // rows of one scan group (launch_scan_u64)

// The tokens of row r of an offset array, and where they start.
__device__ inline uint64_t bt_tokens(const uint64_t *__restrict__ off, uint64_t r, uint64_t &first) {
  first = off[r];
  const uint64_t end = off[r + 1];
  return end > first ? end - first : 0;
}

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

__device__ inline void bt_store_one(void *out, uint64_t slot, bool ids64, uint32_t v) {
  if (ids64) reinterpret_cast<uint64_t *>(out)[slot] = v;
  else reinterpret_cast<uint32_t *>(out)[slot] = v;
}

// four ids of a row: one 16-byte load of int32, two of int64
template <class T> __device__ inline void bt_load_quad(const T *p, T (&v)[kBtQuad]);
template <> __device__ inline void bt_load_quad<int32_t>(const int32_t *p, int32_t (&v)[kBtQuad]) {
  const int4 q = *reinterpret_cast<const int4 *>(p);
  v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
}
template <> __device__ inline void bt_load_quad<int64_t>(const int64_t *p, int64_t (&v)[kBtQuad]) {
  const longlong2 a = reinterpret_cast<const longlong2 *>(p)[0], b = reinterpret_cast<const longlong2 *>(p)[1];
  v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
}

// The dense id of a token of the stream: raw = the encoder's id, bit 31 its flag; map[s + flagged-and-set * n_map] where a map
// is given, else the id itself.  An id outside the map, or one the map leaves out, is unk_id and is counted.
__device__ inline uint32_t bt_dense_id(uint32_t raw, const uint32_t *__restrict__ map, uint32_t n_map, int flagged, uint32_t unk_id,
                                       uint32_t &n_unk) {
  const uint32_t s = raw & 0x7FFFFFFFu;
  uint32_t d = SWT_BATCH_NONE;
  if (s < n_map) d = map ? map[(uint64_t)s + ((flagged && (raw >> 31)) ? (uint64_t)n_map : 0ull)] : s;
  if (d == SWT_BATCH_NONE) { d = unk_id; n_unk++; }
  return d;
}

// The K counts of a kernel, folded over the wavefront and then, through `waves` (LDS), over the workgroup: -> the workgroup's sum
// of counter k in thread k < K, 0 in every other thread.  Every thread of the workgroup calls it once: there is a barrier in it,
// behind which whatever else the wavefronts left in LDS before the call may be read as well.
template <class N, uint32_t K, uint32_t kWaves>
__device__ inline unsigned long long bt_fold_counts(const N (&n)[K], unsigned long long (&waves)[kWaves][K]) {
#pragma unroll
  for (uint32_t k = 0; k < K; k++) {
    unsigned long long s = n[k];
    for (int d = 32; d; d >>= 1) s += __shfl_xor(s, d, 64);
    if ((threadIdx.x & 63) == 0) waves[threadIdx.x >> 6][k] = s;
  }
  __syncthreads();
  unsigned long long s = 0;
  if (threadIdx.x < K)
    for (uint32_t w = 0; w < kWaves; w++) s += waves[w][threadIdx.x];
  return s;
}

// every pointer of the list is a multiple of a (a null pointer is)
inline bool bt_aligned(uintptr_t a, std::initializer_list<const void *> ps) {
  for (const void *p : ps)
    if (reinterpret_cast<uintptr_t>(p) & (a - 1)) return false;
  return true;
}

// The scan workspace of the plans: grow-only, shared by all calls of the process (the calls carry no handle); a plan uses it on
// its own stream, so plans on different streams must not overlap -- the header says so.  reserve: room for a scan over n_rows
// values (launch_scan_u64), the ticket zeroed when the buffer is new.
struct BatchWorkspace {
  DevBuf local, blk;
  int reserve(uint64_t n_rows);
};
extern BatchWorkspace g_batch_ws;

// Host launchers of the two kernels every plan of the family ends with (defined in swt_batch.hip).
// d_vals[0, n) -> their exclusive sums in place, the total in d_vals[n] and in *d_total: launch_scan_u64, then the group bases.
// n >= 1, and g_batch_ws.reserve(n) has been called: before the plan's first launch, so that a failed allocation touches nothing
void launch_scan_bases(uint64_t n, unsigned long long *d_vals, uint64_t *d_total, hipStream_t st);
// d_out[k] = the sum over the n_blocks workgroups of part[block * n_counts + k]: one workgroup per counter and no atomic --
// thousands of workgroups adding to a few words of one cache line cost more than the kernels themselves
void launch_counts_sum(const unsigned long long *d_part, uint64_t n_blocks, uint32_t n_counts, unsigned long long *d_out, hipStream_t st);

// What the calls over finished rows (masked-LM, decode) refuse of their shape.
inline int bt_check_shape(uint64_t rows, uint32_t width) {
  if (rows && !width) return fail(SWT_ERR_INVALID, "width: rows of no column");
  if (rows > 0xFFFFFFFFull) return fail(SWT_ERR_INVALID, "rows: 2^32 rows or more");
  if (width > 0x7FFFFFFFu) return fail(SWT_ERR_INVALID, "width: 2^31 columns or more");
  return SWT_OK;
}

// The device side of a host form.  in(): a host array goes up and its device copy comes back -- none for a null pointer, unless
// the call takes the array even when it is empty (always); out(): room for an output that was given; fetch(): after the call,
// the stream drained, every output back where it belongs.  A failure stays in rc and hands out null pointers from then on;
// whatever ends the call, the buffers are released.
struct BatchStage {
  struct Out { void *host; const void *dev; size_t bytes; };
  std::deque<DevBuf> bufs;
  std::vector<Out> outs;
  int rc = SWT_OK;
  ~BatchStage() { for (DevBuf &b : bufs) b.release(); }
  void *room(size_t bytes) {
    if (rc) return nullptr;
    bufs.emplace_back();
    rc = bufs.back().reserve(bytes + 16);
    return rc ? nullptr : bufs.back().p;
  }
  int copy(void *dst, const void *src, size_t bytes, hipMemcpyKind kind) {
    if (bytes) SWT_HIP(hipMemcpy(dst, src, bytes, kind));
    return SWT_OK;
  }
  template <class T> T *in(const T *host, size_t bytes, bool always = false) {
    void *d = host || always ? room(bytes) : nullptr;
    if (d && host) rc = copy(d, host, bytes, hipMemcpyHostToDevice);
    return rc ? nullptr : static_cast<T *>(d);
  }
  template <class T> T *out(T *host, size_t bytes) {
    void *d = host ? room(bytes) : nullptr;
    if (d) outs.push_back({host, d, bytes});
    return static_cast<T *>(d);
  }
  int fetch() {
    SWT_HIP(hipStreamSynchronize(nullptr));
    for (const Out &o : outs)
      if ((rc = copy(o.host, o.dev, o.bytes, hipMemcpyDeviceToHost))) return rc;
    return SWT_OK;
  }
};

}  // namespace swt
