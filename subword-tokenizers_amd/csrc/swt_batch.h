// swt_batch.h -- what the batch calls (swt_batch.hip: padded rows and pairs) and the packing calls (swt_pack.hip) share: the
// stores of a lane's four columns, the scan workspace of the plans and the device side of a host form.
#pragma once

#include <deque>
#include <initializer_list>
#include <vector>

#include "swt_tile.h"

namespace swt {

constexpr uint32_t kBtQuad = 4;           // columns of one lane per step
constexpr uint32_t kBtCols = 64 * kBtQuad;  // columns of one wavefront per step
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
