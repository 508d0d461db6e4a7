// swt_tile.h -- what the encoders (FastBPE / NaiveBPE in swt_bpe_encode.hip, FastWP / NaiveWP in swt_wp.hip) share.
//
//   tile   = the sentences whose first byte lies in one window of the text (256 B .. 1 KiB, per kernel).  A tile owns
//            whole sentences: no sentence is seen by two workgroups, there are no data-path atomics, and a tile's
//            tokens are contiguous in the final output.
//   chunk  = the part of the tile's span staged in LDS at a time (16-byte aligned base so the staging loads are
//            dwordx4).  One chunk is the common case; longer spans are walked chunk by chunk.
//   per chunk: A stage bytes -> B decode/classify per byte -> C/D encoder body leaves one token id or kInvalidTok per
//            byte (WordPiece) or per symbol (BPE) -> E order-preserving ballot compaction to the tile's output run -> F
//            per-sentence local offsets.
// Shared HERE, by all four encoders:
//   around the encode kernel   DirectOut (the single-launch form), TileWorkspace, the plan before it, the scan of tile totals
//                              and the gather into the caller's CSR (ids + sentence offsets) after it (swt_tile.hip)
//   above the _dev calls       HostStage + HostEncoder and the three host entry forms (host_encode*, swt_tile.hip): argument
//                              checks, the pinned / one-copy / large paths, the unpacking with its capacity check
// NOT here: the device code of a chunk.  The two WordPiece kernels share theirs in swt_wp.hip (wp_tile_begin, wp_stage, wp_mark,
// wp_giant, wp_emit, wp_tile_end; only B, C and D are a kernel's own).  bpe_lane_kernel keeps its own phases (lane_split ..
// lane_emit): its split and its compaction work over symbol space, not bytes.
#pragma once

#include <functional>

#include "swt_common.h"
#include "swt_tilemap.h"

namespace swt {

constexpr int kThreads = 256;  // gather_kernel

// Direct mode of the encode kernels, for inputs of a few hundred bytes (the reference-style call: one sentence): ONE workgroup
// takes all sentences as its tile and writes the caller's arrays itself -- 64-bit sentence offsets, the closing offset and the
// token count -- so the call is one launch instead of plan + encode + scan + gather.  off == nullptr: the normal mode.
struct DirectOut {
  uint64_t *off;
  uint64_t *n_tokens;
  uint64_t n_sent;
};

// Per-call workspaces shared by both encoders (grow-only).
struct TileWorkspace {
  DevBuf plan, scratch, sent_local, tile_tok, tile_base, blk;
  int reserve(uint64_t n_bytes, uint64_t n_sent, uint64_t n_tiles);
  void release();
};

// tile_count(n_bytes, tile): swt_tilemap.h

// Host launchers of the skeleton's own kernels (defined in swt_tile.hip).
// plan[t] = the first sentence that begins at or behind map.boundary(t), for t in [0, map.n_tiles]; plan[n_tiles] = n_sent
void launch_plan(const uint64_t *d_sent_off, uint64_t n_sent, const TileMap &map, uint64_t *d_plan, hipStream_t st);
// the same for n_tiles tiles of one size (a one-segment map)
void launch_plan(const uint64_t *d_sent_off, uint64_t n_sent, uint64_t n_tiles, uint32_t tile, uint64_t *d_plan, hipStream_t st);
void launch_scan_only(uint64_t n_tiles, const TileWorkspace &ws, uint64_t *d_n_tokens, hipStream_t st);
// the same scan over 64-bit values: d_local[i] = exclusive sum inside i's group of 1024, blk = [ticket (zero), totals[nb],
// bases[nb]] with nb = ceil(n / 1024); global exclusive sum of i = blk[1 + nb + (i >> 10)] + d_local[i]
void launch_scan_u64(uint64_t n, const unsigned long long *d_in, unsigned long long *d_local, unsigned long long *blk,
                     uint64_t *d_total, hipStream_t st);
void launch_scan_gather(const uint64_t *d_sent_off, uint64_t n_sent, uint64_t n_tiles, const TileWorkspace &ws,
                        uint32_t *d_out_ids, uint64_t *d_out_off, uint64_t *d_n_tokens, hipStream_t st);
// After launch_scan_gather, with its tile bases: what travelled through scratch next to the ids of the same tiles -- a span
// (two words) and a word index per token slot -- to the same slots of the caller's arrays.
void launch_gather_spans(const uint64_t *d_sent_off, uint64_t n_tiles, const TileWorkspace &ws, const uint32_t *d_sp_scratch,
                         const uint32_t *d_wd_scratch, uint32_t *d_spans, uint32_t *d_word, hipStream_t st);

// ---- the host-call layer: what stands between a host entry point (swt_*_encode, swt_*_encode_joined and their naive forms) and
// the encoder's _dev call.  An encoder describes itself in a HostEncoder, keeps a HostStage in its handle, and its extern "C"
// functions are one line each.

// Staging buffers of the host entry points (grow-only, one set per handle).
struct HostStage {
  DevBuf in_text, in_off;                      // the large path: text and offsets on their way up
  DevBuf out_ids, out_off, out_status, n_tok;  // device text -> the caller's host arrays (the large path, the joined form)
  PinnedBuf pin;                               // the two small paths: inputs and outputs in one pinned buffer
  DevBuf small_in, small_out;                  // the one-copy path
  DevBuf out_spans, out_word;                  // the large path of an encoder with extra outputs (HostExtra)
  void release();
};

// Optional extra outputs of a host call, per token slot next to the ids: spans (two words each) and word indices (may be null).
// Every path of host_encode carries them behind the ids, sized as the ids are; they are copied out only when the ids fit.
struct HostExtra {
  uint32_t *spans;
  uint32_t *word;
};

struct HostEncoder {
  // the handle's tables to the device; runs after the null checks and before anything else is looked at
  std::function<int()> upload;
  // enqueues the device encode on the null stream (d_status is null when has_status is false)
  std::function<int(const uint8_t *d_text, uint64_t n_bytes, const uint64_t *d_off, uint64_t n_sent, uint32_t *d_ids,
                    uint64_t *d_out_off, uint8_t *d_status, uint64_t *d_n_tokens)> dev;
  uint64_t direct_bytes, direct_sents;  // up to here the _dev call is ONE launch that writes the caller's arrays (DirectOut)
  bool has_status;                      // per-sentence statuses (WordPiece)
  // the same with spans and word indices (device arrays of 2 * (n_bytes + 64) and n_bytes + 64 words); used instead of dev when
  // the host call was given a HostExtra
  std::function<int(const uint8_t *d_text, uint64_t n_bytes, const uint64_t *d_off, uint64_t n_sent, uint32_t *d_ids,
                    uint64_t *d_out_off, uint8_t *d_status, uint64_t *d_n_tokens, uint32_t *d_spans, uint32_t *d_word)> dev_extra = {};
};

// Text and offsets on the device -> ids, offsets, statuses and the count in the caller's host arrays.  Offsets, statuses and
// *n_tokens are written before SWT_ERR_CAPACITY is returned, here and below.
int host_encode_from_device(HostStage &hs, const HostEncoder &enc, const uint8_t *d_text, uint64_t n_bytes, const uint64_t *d_off,
                            uint64_t n_sent, uint32_t *out_ids, uint64_t out_cap, uint64_t *out_off, uint8_t *status, uint64_t *n_tokens,
                            const HostExtra *extra = nullptr);
// Host buffers -> ids.  By size alone: up to the single-launch limits the kernel reads and writes pinned host memory (no copy
// call at all); up to kSmallCallBytes / kSmallCallSents one copy up and one down; beyond, plain copies.
int host_encode(HostStage &hs, const HostEncoder &enc, const uint8_t *text, const uint64_t *sent_off, uint64_t n_sent,
                uint32_t *out_ids, uint64_t out_cap, uint64_t *out_off, uint8_t *status, uint64_t *n_tokens,
                const HostExtra *extra = nullptr);
// list[str] joined with U+0000 -> ids, the prepared text never coming back to the host (with_prepared_joined, swt_words.h).
// *n_tokens = UINT64_MAX on return: a sentence needs the host's str.lower() (need_host says which) and nothing was encoded.
int host_encode_joined(HostStage &hs, const HostEncoder &enc, const uint8_t *joined, uint64_t n_joined, uint64_t n_sent,
                       uint32_t *out_ids, uint64_t out_cap, uint64_t *out_off, uint8_t *status, uint64_t *n_tokens, uint8_t *need_host);

}  // namespace swt
