// swt_tile.hip -- the skeleton's own kernels: plan (tile -> first sentence), scan of tile totals, gather; and the host-call layer
// of the encoders (host_encode*).
#include "swt_tile.h"
#include "swt_words.h"

namespace swt {

// plan[t] = first sentence whose first byte is >= map.boundary(t)  (lower bound; plan[n_tiles] = n_sent).  Two forms, the same result:
// the search (one thread per tile, log2(n_sent) dependent loads) for texts of few long sentences, and the pass below.  The
// arithmetic of both is in swt_tilemap.h (plan_search, plan_range), where a CPU test runs it.
__global__ void plan_kernel(const uint64_t *__restrict__ sent_off, uint64_t n_sent, TileMap map, uint64_t *__restrict__ plan) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t > map.n_tiles) return;
  plan[t] = plan_search(map, sent_off, n_sent, t);
}

// The pass: one thread per sentence, no dependent load.  Sentence s is the answer for every tile boundary in
// (sent_off[s-1], sent_off[s]] (from 0 for s = 0; an empty sentence owns none, so the first of several at one offset wins), and
// "sentence" n_sent for the boundaries past the last sentence's start and for plan[n_tiles].  A thread writes up to four
// entries itself; a longer range (a sentence of many tiles) is written by its whole wave, so one giant sentence costs a wave
// n / 64 steps and not one thread n.
__global__ __launch_bounds__(256) void plan_pass_kernel(const uint64_t *__restrict__ sent_off, uint64_t n_sent, TileMap map,
                                                        uint64_t *__restrict__ plan) {
  const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63;
  uint64_t lo = 1, hi = 0;  // tiles [lo, hi] get s; empty for the threads past n_sent
  if (s <= n_sent) plan_range(map, sent_off, n_sent, s, lo, hi);
  const uint64_t cnt = hi + 1 > lo ? hi + 1 - lo : 0;
  if (cnt <= 4)
    for (uint64_t t = lo; t <= hi; t++) plan[t] = s;
  for (unsigned long long LONG = __ballot(cnt > 4); LONG; LONG &= LONG - 1ull) {
    const int src = __builtin_ctzll(LONG);
    const uint64_t l = __shfl(lo, src), h = __shfl(hi, src), v = __shfl(s, src);
    for (uint64_t t = l + lane; t <= h; t += 64) plan[t] = v;
  }
}

// Exclusive scan of the tile totals, one launch: every workgroup scans its 1024 tiles locally and publishes its total;
// the last one to arrive (ticket) scans the workgroup totals.  Global base of tile t = blk_base[t >> 10] + tile_base[t].
template <class T>
__global__ __launch_bounds__(1024) void tile_scan_kernel(const T *__restrict__ tile_tok, uint64_t n_tiles,
                                                         T *__restrict__ tile_base, unsigned long long *__restrict__ blk_tot,
                                                         unsigned long long *__restrict__ blk_base, unsigned int *__restrict__ ticket,
                                                         uint64_t *__restrict__ n_tokens) {
  __shared__ unsigned long long wsum[16];
  __shared__ unsigned long long carry_s;
  __shared__ bool is_last;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint64_t i = (uint64_t)blockIdx.x * 1024 + tid;
  const unsigned long long v = i < n_tiles ? tile_tok[i] : 0;
  unsigned long long x = v;
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long y = __shfl_up(x, d);
    if (lane >= d) x += y;
  }
  if (lane == 63) wsum[wave] = x;
  __syncthreads();
  unsigned long long wb = 0;
  for (int w = 0; w < wave; w++) wb += wsum[w];
  if (i < n_tiles) tile_base[i] = (T)(wb + x - v);
  if (tid == 1023) {
    // the total travels in a device-scope store and is read back by device-scope loads below, so the ticket only has to wait until
    // the store has been performed -- no device-scope FENCE (which writes the XCD's L2 back and invalidates it, once per workgroup)
    __hip_atomic_store(&blk_tot[blockIdx.x], wb + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    is_last = atomicAdd(ticket, 1u) == gridDim.x - 1;
  }
  __syncthreads();
  if (!is_last) return;
  if (tid == 0) carry_s = 0;
  __syncthreads();
  for (uint32_t base = 0; base < gridDim.x; base += 1024) {
    const uint32_t j = base + tid;
    const unsigned long long u = j < gridDim.x ? __hip_atomic_load(&blk_tot[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
    unsigned long long z = u;
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned long long y = __shfl_up(z, d);
      if (lane >= d) z += y;
    }
    if (lane == 63) wsum[wave] = z;
    __syncthreads();
    unsigned long long wb2 = 0;
    for (int w = 0; w < wave; w++) wb2 += wsum[w];
    const unsigned long long carry = carry_s;
    if (j < gridDim.x) blk_base[j] = carry + wb2 + z - u;
    __syncthreads();
    if (tid == 1023) carry_s = carry + wb2 + z;
    __syncthreads();
  }
  if (tid == 0) {
    *n_tokens = carry_s;
    *ticket = 0;  // ready for the next call
  }
}

// The same scan for up to kScanOne tiles in ONE workgroup: eight tiles per thread, nothing handed from workgroup to workgroup.
// It fills what the gather reads of the form above: tile_base[t] = the global base, blk_base[t >> 10] = 0.  32 bits hold the base:
// the tokens of a call are no more than its bytes, and those no more than 8,192 tiles (a few KiB each at most).
constexpr uint64_t kScanOne = 8192;
__global__ __launch_bounds__(1024) void tile_scan_one_kernel(const uint32_t *__restrict__ tile_tok, uint32_t n_tiles,
                                                             uint32_t *__restrict__ tile_base, unsigned long long *__restrict__ blk_base,
                                                             uint64_t *__restrict__ n_tokens) {
  __shared__ uint32_t wsum[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t i0 = (uint32_t)tid * 8;
  uint32_t v[8];
  if (i0 + 8 <= n_tiles) {  // tile_tok and tile_base come from hipMalloc: 32 bytes into them is 16-byte aligned
    const uint4 a = *reinterpret_cast<const uint4 *>(tile_tok + i0), b = *reinterpret_cast<const uint4 *>(tile_tok + i0 + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  } else {
    for (int k = 0; k < 8; k++) v[k] = i0 + k < n_tiles ? tile_tok[i0 + k] : 0u;
  }
  uint32_t mine = 0;
  for (int k = 0; k < 8; k++) mine += v[k];
  uint32_t x = mine;
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t y = __shfl_up(x, d);
    if (lane >= d) x += y;
  }
  if (lane == 63) wsum[wave] = x;
  __syncthreads();
  uint32_t wb = 0, all = 0;
  for (int w = 0; w < 16; w++) {
    if (w < wave) wb += wsum[w];
    all += wsum[w];
  }
  uint32_t run = wb + x - mine;
  for (int k = 0; k < 8; k++) {
    if (i0 + k < n_tiles) tile_base[i0 + k] = run;
    run += v[k];
  }
  if ((uint32_t)tid < ((n_tiles + 1023u) >> 10)) blk_base[tid] = 0ull;
  if (tid == 0) *n_tokens = all;
}

// A tile's tokens are contiguous in the output: copy its run and turn local sentence offsets into global ones.  A tile holds
// a few dozen tokens: one WAVE per tile (a workgroup per tile spent most of the launch on dispatching 66 k workgroups).
__global__ __launch_bounds__(kThreads) void gather_kernel(const uint64_t *__restrict__ sent_off, const uint64_t *__restrict__ plan,
                                                          uint64_t n_tiles, uint64_t n_sent, const uint32_t *__restrict__ scratch,
                                                          const uint32_t *__restrict__ sent_local, const uint32_t *__restrict__ tile_tok,
                                                          const uint32_t *__restrict__ tile_base, const unsigned long long *__restrict__ blk_base,
                                                          const uint64_t *__restrict__ n_tokens, uint32_t *__restrict__ out_ids,
                                                          uint64_t *__restrict__ out_off) {
  const int lane = threadIdx.x & 63;
  const uint64_t t = (uint64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (t >= n_tiles) return;
  const uint64_t s_lo = plan[t], s_hi = plan[t + 1];
  if (t == n_tiles - 1 && lane == 0) out_off[n_sent] = *n_tokens;
  if (s_lo == s_hi) return;
  const uint64_t base = blk_base[t >> 10] + tile_base[t];
  const uint32_t n = tile_tok[t];
  const uint32_t *src = scratch + sent_off[s_lo];
  for (uint32_t i = lane; i < n; i += 64) out_ids[base + i] = src[i];
  for (uint64_t s = s_lo + lane; s < s_hi; s += 64) out_off[s] = base + sent_local[s];
}

// The gather of what travels next to the ids (token spans and word indices): the same tiles, the same bases, the same slots.
__global__ __launch_bounds__(kThreads) void gather_spans_kernel(const uint64_t *__restrict__ sent_off, const uint64_t *__restrict__ plan,
                                                                uint64_t n_tiles, const uint32_t *__restrict__ sp_scratch,
                                                                const uint32_t *__restrict__ wd_scratch, const uint32_t *__restrict__ tile_tok,
                                                                const uint32_t *__restrict__ tile_base,
                                                                const unsigned long long *__restrict__ blk_base, uint32_t *__restrict__ out_spans,
                                                                uint32_t *__restrict__ out_word) {
  const int lane = threadIdx.x & 63;
  const uint64_t t = (uint64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (t >= n_tiles) return;
  const uint64_t s_lo = plan[t], s_hi = plan[t + 1];
  if (s_lo == s_hi) return;
  const uint64_t base = blk_base[t >> 10] + tile_base[t];
  const uint32_t n = tile_tok[t];
  const uint64_t src = sent_off[s_lo];
  for (uint32_t i = lane; i < n; i += 64) {
    out_spans[2 * (base + i)] = sp_scratch[2 * (src + i)];
    out_spans[2 * (base + i) + 1] = sp_scratch[2 * (src + i) + 1];
    if (out_word) out_word[base + i] = wd_scratch[src + i];
  }
}

int TileWorkspace::reserve(uint64_t n_bytes, uint64_t n_sent, uint64_t n_tiles) {
  int rc;
  if ((rc = plan.reserve((n_tiles + 1) * 8))) return rc;
  if ((rc = scratch.reserve((n_bytes + 64) * 4))) return rc;
  if ((rc = sent_local.reserve((n_sent + 1) * 4))) return rc;
  if ((rc = tile_tok.reserve((n_tiles + 1) * 4))) return rc;
  if ((rc = tile_base.reserve((n_tiles + 2) * 4))) return rc;
  const uint64_t nb = (n_tiles + 1023) / 1024;
  const void *before = blk.p;
  if ((rc = blk.reserve((2 * nb + 4) * 8))) return rc;
  if (blk.p != before) {  // a new buffer: zero the ticket once (the scan kernel resets it itself afterwards)
    SWT_HIP(hipMemset(blk.p, 0, 8));
    SWT_HIP(hipDeviceSynchronize());  // rare path; callers launch on streams that need not order with the null stream
  }
  return SWT_OK;
}

void TileWorkspace::release() {
  plan.release(); scratch.release(); sent_local.release(); tile_tok.release(); tile_base.release(); blk.release();
}

void launch_plan(const uint64_t *d_sent_off, uint64_t n_sent, const TileMap &map, uint64_t *d_plan, hipStream_t st) {
  const uint64_t n_tiles = map.n_tiles;
  // the pass reads every sentence offset once; the search is the better form only where sentences are few and tiles many
  if (n_sent / 256 <= n_tiles)
    hipLaunchKernelGGL(plan_pass_kernel, dim3((unsigned)((n_sent + 1 + 255) / 256)), dim3(256), 0, st, d_sent_off, n_sent, map, d_plan);
  else
    hipLaunchKernelGGL(plan_kernel, dim3((unsigned)((n_tiles + 1 + 255) / 256)), dim3(256), 0, st, d_sent_off, n_sent, map, d_plan);
}

void launch_plan(const uint64_t *d_sent_off, uint64_t n_sent, uint64_t n_tiles, uint32_t tile, uint64_t *d_plan, hipStream_t st) {
  TileMap map = tilemap_uniform(0, tile);
  map.n_tiles = n_tiles;  // the caller's count: the dedup path plans fewer tiles than its text would have
  launch_plan(d_sent_off, n_sent, map, d_plan, st);
}

void launch_scan_only(uint64_t n_tiles, const TileWorkspace &ws, uint64_t *d_n_tokens, hipStream_t st) {
  const uint64_t nb = (n_tiles + 1023) / 1024;
  unsigned long long *b = ws.blk.as<unsigned long long>();
  hipLaunchKernelGGL(tile_scan_kernel<uint32_t>, dim3((unsigned)nb), dim3(1024), 0, st, ws.tile_tok.as<uint32_t>(), n_tiles,
                     ws.tile_base.as<uint32_t>(), b + 1, b + 1 + nb, reinterpret_cast<unsigned int *>(b), d_n_tokens);
}

void launch_scan_u64(uint64_t n, const unsigned long long *d_in, unsigned long long *d_local, unsigned long long *blk,
                     uint64_t *d_total, hipStream_t st) {
  const uint64_t nb = (n + 1023) / 1024;
  hipLaunchKernelGGL(tile_scan_kernel<unsigned long long>, dim3((unsigned)nb), dim3(1024), 0, st, d_in, n, d_local, blk + 1,
                     blk + 1 + nb, reinterpret_cast<unsigned int *>(blk), d_total);
}

void launch_scan_gather(const uint64_t *d_sent_off, uint64_t n_sent, uint64_t n_tiles, const TileWorkspace &ws,
                        uint32_t *d_out_ids, uint64_t *d_out_off, uint64_t *d_n_tokens, hipStream_t st) {
  const uint64_t nb = (n_tiles + 1023) / 1024;
  // blk layout: [0] ticket (8 bytes), then blk_tot[nb], then blk_base[nb]
  unsigned long long *b = ws.blk.as<unsigned long long>();
  unsigned int *ticket = reinterpret_cast<unsigned int *>(b);
  unsigned long long *blk_tot = b + 1, *blk_base = b + 1 + nb;
  if (n_tiles <= kScanOne)
    hipLaunchKernelGGL(tile_scan_one_kernel, dim3(1), dim3(1024), 0, st, ws.tile_tok.as<uint32_t>(), (uint32_t)n_tiles,
                       ws.tile_base.as<uint32_t>(), blk_base, d_n_tokens);
  else
    hipLaunchKernelGGL(tile_scan_kernel<uint32_t>, dim3((unsigned)nb), dim3(1024), 0, st, ws.tile_tok.as<uint32_t>(), n_tiles,
                       ws.tile_base.as<uint32_t>(), blk_tot, blk_base, ticket, d_n_tokens);
  hipLaunchKernelGGL(gather_kernel, dim3((unsigned)((n_tiles + kThreads / 64 - 1) / (kThreads / 64))), dim3(kThreads), 0, st, d_sent_off, ws.plan.as<uint64_t>(), n_tiles,
                     n_sent, ws.scratch.as<uint32_t>(), ws.sent_local.as<uint32_t>(), ws.tile_tok.as<uint32_t>(),
                     ws.tile_base.as<uint32_t>(), blk_base, d_n_tokens, d_out_ids, d_out_off);
}

void launch_gather_spans(const uint64_t *d_sent_off, uint64_t n_tiles, const TileWorkspace &ws, const uint32_t *d_sp_scratch,
                         const uint32_t *d_wd_scratch, uint32_t *d_spans, uint32_t *d_word, hipStream_t st) {
  const uint64_t nb = (n_tiles + 1023) / 1024;
  const unsigned long long *blk_base = ws.blk.as<unsigned long long>() + 1 + nb;
  hipLaunchKernelGGL(gather_spans_kernel, dim3((unsigned)((n_tiles + kThreads / 64 - 1) / (kThreads / 64))), dim3(kThreads), 0, st, d_sent_off,
                     ws.plan.as<uint64_t>(), n_tiles, d_sp_scratch, d_wd_scratch, ws.tile_tok.as<uint32_t>(), ws.tile_base.as<uint32_t>(),
                     blk_base, d_spans, d_word);
}

// ---- the host-call layer --------------------------------------------------------------------------------------------

void HostStage::release() {
  for (DevBuf *b : {&in_text, &in_off, &out_ids, &out_off, &out_status, &n_tok, &small_in, &small_out, &out_spans, &out_word}) b->release();
  pin.release();
}

// A call's results to the caller's arrays: the count, the offsets and the statuses (st, null for none) first, the ids only if
// they fit.  device: the sources are device buffers (blocking copies); otherwise host memory the device has finished writing.
// extra with its sources sp and wd: the spans and word indices of the same token slots, copied when the ids are.
static int unpack(const void *count, const void *off, const void *st, const void *ids, bool device, uint64_t n_sent, uint32_t *out_ids,
                  uint64_t out_cap, uint64_t *out_off, uint8_t *status, uint64_t *n_tokens, const HostExtra *extra = nullptr,
                  const void *sp = nullptr, const void *wd = nullptr) {
  const auto get = [device](void *dst, const void *src, size_t n) {
    if (device) return hipMemcpy(dst, src, n, hipMemcpyDeviceToHost);
    memcpy(dst, src, n);
    return hipSuccess;
  };
  uint64_t nt = 0;
  SWT_HIP(get(&nt, count, 8));
  *n_tokens = nt;
  SWT_HIP(get(out_off, off, (n_sent + 1) * 8));
  if (st && n_sent) SWT_HIP(get(status, st, n_sent));
  if (nt > out_cap)
    return fail(SWT_ERR_CAPACITY, "out_ids too small: need %llu ids, have %llu", (unsigned long long)nt, (unsigned long long)out_cap);
  if (nt) SWT_HIP(get(out_ids, ids, nt * 4));
  if (nt && extra) {
    SWT_HIP(get(extra->spans, sp, nt * 8));
    if (extra->word) SWT_HIP(get(extra->word, wd, nt * 4));
  }
  return SWT_OK;
}

int host_encode_from_device(HostStage &hs, const HostEncoder &enc, const uint8_t *d_text, uint64_t n_bytes, const uint64_t *d_off,
                            uint64_t n_sent, uint32_t *out_ids, uint64_t out_cap, uint64_t *out_off, uint8_t *status, uint64_t *n_tokens,
                            const HostExtra *extra) {
  int rc;
  if ((rc = hs.out_ids.reserve((n_bytes + 64) * 4))) return rc;
  if ((rc = hs.out_off.reserve((n_sent + 1) * 8))) return rc;
  if (enc.has_status && (rc = hs.out_status.reserve(n_sent + 8))) return rc;
  if ((rc = hs.n_tok.reserve(8))) return rc;
  uint8_t *const d_status = enc.has_status ? hs.out_status.as<uint8_t>() : nullptr;
  if (extra) {
    if ((rc = hs.out_spans.reserve((n_bytes + 64) * 8)) || (rc = hs.out_word.reserve((n_bytes + 64) * 4))) return rc;
    if ((rc = enc.dev_extra(d_text, n_bytes, d_off, n_sent, hs.out_ids.as<uint32_t>(), hs.out_off.as<uint64_t>(), d_status,
                            hs.n_tok.as<uint64_t>(), hs.out_spans.as<uint32_t>(), hs.out_word.as<uint32_t>())))
      return rc;
    return unpack(hs.n_tok.p, hs.out_off.p, d_status, hs.out_ids.p, true, n_sent, out_ids, out_cap, out_off, status, n_tokens, extra,
                  hs.out_spans.p, hs.out_word.p);
  }
  if ((rc = enc.dev(d_text, n_bytes, d_off, n_sent, hs.out_ids.as<uint32_t>(), hs.out_off.as<uint64_t>(), d_status, hs.n_tok.as<uint64_t>())))
    return rc;
  return unpack(hs.n_tok.p, hs.out_off.p, d_status, hs.out_ids.p, true, n_sent, out_ids, out_cap, out_off, status, n_tokens);
}

int host_encode(HostStage &hs, const HostEncoder &enc, const uint8_t *text, const uint64_t *sent_off, uint64_t n_sent,
                uint32_t *out_ids, uint64_t out_cap, uint64_t *out_off, uint8_t *status, uint64_t *n_tokens, const HostExtra *extra) {
  if (!sent_off || !out_off || !n_tokens || (enc.has_status && n_sent && !status)) return fail(SWT_ERR_INVALID, "null argument");
  if (extra && (!extra->spans || !enc.dev_extra)) return fail(SWT_ERR_INVALID, "null spans");
  int rc = enc.upload();
  if (rc) return rc;
  const uint64_t n_bytes = sent_off[n_sent];
  if (sent_off[0] != 0) return fail(SWT_ERR_INVALID, "sent_off[0] must be 0");
  for (uint64_t s = 0; s < n_sent; s++)
    if (sent_off[s] > sent_off[s + 1])
      return fail(SWT_ERR_INVALID, "sentence offsets must be non-decreasing (at %llu)", (unsigned long long)s);
  if (n_bytes && !text) return fail(SWT_ERR_INVALID, "null text");
  // The two small paths move one block each way.  In: the offsets, then the text.  Out: the count at 0, the offsets at 16, the
  // statuses behind them, the ids last -- every part at a multiple of 16.
  const size_t off_bytes = ((n_sent + 1) * 8 + 15) & ~(size_t)15, st_bytes = enc.has_status ? (n_sent + 15) & ~(size_t)15 : 0;
  // With a HostExtra the spans and the word indices follow the ids.
  const size_t st_at = 16 + off_bytes, ids_at = st_at + st_bytes, sp_at = ids_at + (n_bytes + 64) * 4, wd_at = sp_at + (n_bytes + 64) * 8;
  const size_t out_bytes = extra ? wd_at + (n_bytes + 64) * 4 : sp_at;
  const auto encode = [&](const uint8_t *in, uint8_t *o) {
    if (extra)
      return enc.dev_extra(in + off_bytes, n_bytes, reinterpret_cast<const uint64_t *>(in), n_sent, reinterpret_cast<uint32_t *>(o + ids_at),
                           reinterpret_cast<uint64_t *>(o + 16), enc.has_status ? o + st_at : nullptr, reinterpret_cast<uint64_t *>(o),
                           reinterpret_cast<uint32_t *>(o + sp_at), reinterpret_cast<uint32_t *>(o + wd_at));
    return enc.dev(in + off_bytes, n_bytes, reinterpret_cast<const uint64_t *>(in), n_sent, reinterpret_cast<uint32_t *>(o + ids_at),
                   reinterpret_cast<uint64_t *>(o + 16), enc.has_status ? o + st_at : nullptr, reinterpret_cast<uint64_t *>(o));
  };
  const auto unpack_block = [&](const uint8_t *o) {
    return unpack(o, o + 16, enc.has_status ? o + st_at : nullptr, o + ids_at, false, n_sent, out_ids, out_cap, out_off, status, n_tokens,
                  extra, o + sp_at, o + wd_at);
  };
  if (n_bytes <= enc.direct_bytes && n_sent <= enc.direct_sents && n_sent > 0) {
    // tokenize(text) on one sentence, the reference's call: the single workgroup of the direct form reads the text and the
    // offsets from pinned host memory and writes the out block there -- one launch and one synchronisation, no copy call at all.
    // Measured (FastBPE): 43.1 -> 40.7 us per call from Python; a launch + hipStreamSynchronize is 11 us here, spinning on a host
    // word instead would save 4.5 of them (tools/micro/sync_probe.hip), the rest is the kernel's own latency chain and ctypes.
    // By size alone: FastWP under SWT_OPT_DEDUP = 2 runs its dedup pipeline over this pinned memory.
    const size_t out_at = off_bytes + ((n_bytes + 64 + 15) & ~(size_t)15);
    if ((rc = hs.pin.reserve(out_at + out_bytes))) return rc;
    uint8_t *h = hs.pin.as<uint8_t>();
    memcpy(h, sent_off, (n_sent + 1) * 8);
    if (n_bytes) memcpy(h + off_bytes, text, n_bytes);
    memset(h + off_bytes + n_bytes, ' ', 64);
    if ((rc = encode(h, h + out_at))) return rc;
    SWT_HIP(hipStreamSynchronize(0));
    return unpack_block(h + out_at);
  }
  if (n_bytes <= kSmallCallBytes && n_sent <= kSmallCallSents) {
    // A few sentences: five small copies and their synchronisations cost more than the kernels.  The in block goes up in ONE
    // copy from pinned memory, the out block comes back in ONE.
    const size_t in_bytes = off_bytes + n_bytes + 64;
    if ((rc = hs.pin.reserve(in_bytes > out_bytes ? in_bytes : out_bytes)) || (rc = hs.small_in.reserve(in_bytes)) ||
        (rc = hs.small_out.reserve(out_bytes)))
      return rc;
    uint8_t *h = hs.pin.as<uint8_t>();
    memcpy(h, sent_off, (n_sent + 1) * 8);
    if (n_bytes) memcpy(h + off_bytes, text, n_bytes);
    SWT_HIP(hipMemcpyAsync(hs.small_in.p, h, off_bytes + n_bytes, hipMemcpyHostToDevice, 0));
    if ((rc = encode(hs.small_in.as<uint8_t>(), hs.small_out.as<uint8_t>()))) return rc;
    SWT_HIP(hipMemcpyAsync(h, hs.small_out.p, out_bytes, hipMemcpyDeviceToHost, 0));
    SWT_HIP(hipStreamSynchronize(0));
    return unpack_block(h);
  }
  if ((rc = hs.in_text.reserve(n_bytes + 64))) return rc;
  if ((rc = hs.in_off.reserve((n_sent + 1) * 8))) return rc;
  if (n_bytes) SWT_HIP(hipMemcpyAsync(hs.in_text.p, text, n_bytes, hipMemcpyHostToDevice, 0));
  SWT_HIP(hipMemcpyAsync(hs.in_off.p, sent_off, (n_sent + 1) * 8, hipMemcpyHostToDevice, 0));
  return host_encode_from_device(hs, enc, hs.in_text.as<uint8_t>(), n_bytes, hs.in_off.as<uint64_t>(), n_sent, out_ids, out_cap, out_off,
                                 status, n_tokens, extra);
}

int host_encode_joined(HostStage &hs, const HostEncoder &enc, const uint8_t *joined, uint64_t n_joined, uint64_t n_sent,
                       uint32_t *out_ids, uint64_t out_cap, uint64_t *out_off, uint8_t *status, uint64_t *n_tokens, uint8_t *need_host) {
  if (!out_off || !n_tokens || (n_sent && (!need_host || (enc.has_status && !status))) || (n_joined && !joined))
    return fail(SWT_ERR_INVALID, "null argument");
  int rc = enc.upload();
  if (rc) return rc;
  *n_tokens = UINT64_MAX;
  auto consume = [&](const uint8_t *d_text, uint64_t n_bytes, const uint64_t *d_off) {
    return host_encode_from_device(hs, enc, d_text, n_bytes, d_off, n_sent, out_ids, out_cap, out_off, status, n_tokens);
  };
  using Consume = decltype(consume);
  bool consumed = false;
  return with_prepared_joined(joined, n_joined, n_sent, need_host, &consumed,
      [](void *p, const uint8_t *d_text, uint64_t n_bytes, const uint64_t *d_off) { return (*static_cast<Consume *>(p))(d_text, n_bytes, d_off); },
      &consume);
}

}  // namespace swt
