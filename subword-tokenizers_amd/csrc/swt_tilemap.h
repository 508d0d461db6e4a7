// swt_tilemap.h -- where the tiles of a text begin when they are not all one size.
//
// A TileMap cuts [0, n_bytes) into up to four segments of equal tiles, the tile size falling from segment to segment.  Every
// segment holds whole tiles (only the very last tile of the text may be short), so both directions are piecewise linear:
//   boundary(t)  the first byte of tile t
//   tile_of(x)   the tile that owns byte x = the largest t with boundary(t) <= x
// One comparison per segment and one division each.  The plan kernels (swt_tile.hip) take a TileMap by value; everything after the
// plan reads plan[] alone and never learns a tile's size.  A one-segment map is the uniform geometry, t * tile and x / tile.
//
// tilemap_taper is the schedule of bpe_lane_kernel's running-text form (swt_bpe_encode.hip, profiles/lane_taper.txt): guided
// self-scheduling over a statically ordered list -- a tile's size follows the bytes still to be handed out, divided by the wave
// slots of the chip, so the waves started last are short ones.
//
// Nothing from HIP is included here: a CPU test compiles this header with g++ (tests/test_tilemap.py).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SWT_TILEMAP_HD __host__ __device__
#else
#define SWT_TILEMAP_HD
#endif

namespace swt {

constexpr int kTileMapSegs = 4;

struct TileMap {
  uint64_t first_byte[kTileMapSegs];  // UINT64_MAX for a segment that is not there
  uint64_t first_tile[kTileMapSegs];
  uint32_t tile_bytes[kTileMapSegs];  // 0 for a segment that is not there
  uint32_t n_segs;
  uint64_t n_tiles;

  SWT_TILEMAP_HD uint64_t boundary(uint64_t t) const {
    int k = 0;
    for (int i = 1; i < kTileMapSegs; i++) k = t >= first_tile[i] ? i : k;
    return first_byte[k] + (t - first_tile[k]) * tile_bytes[k];
  }
  // for x at or past the end of the text: a tile index that may be n_tiles or more (the callers clamp, as they did for x / tile)
  SWT_TILEMAP_HD uint64_t tile_of(uint64_t x) const {
    int k = 0;
    for (int i = 1; i < kTileMapSegs; i++) k = x >= first_byte[i] ? i : k;
    return first_tile[k] + (x - first_byte[k]) / tile_bytes[k];
  }
};

// plan[t] = the first sentence whose first byte is at or behind boundary(t) (a lower bound over sent_off[0 .. n_sent)), for t in
// [0, n_tiles]; plan[n_tiles] = n_sent.  The two forms the plan kernels run, one call per thread.
// The search: tile t.
SWT_TILEMAP_HD inline uint64_t plan_search(const TileMap &map, const uint64_t *sent_off, uint64_t n_sent, uint64_t t) {
  if (t == map.n_tiles) return n_sent;
  const uint64_t target = map.boundary(t);
  uint64_t lo = 0, hi = n_sent;
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if (sent_off[mid] < target) lo = mid + 1; else hi = mid;
  }
  return lo;
}
// The pass: sentence s in [0, n_sent] is the entry of the tiles [lo, hi] (none when lo > hi) -- those with a boundary in
// (sent_off[s-1], sent_off[s]], from 0 for s = 0; an empty sentence owns none, so the first of several at one offset wins;
// "sentence" n_sent takes the boundaries past the last sentence's start and plan[n_tiles], which is written by it and only by it.
SWT_TILEMAP_HD inline void plan_range(const TileMap &map, const uint64_t *sent_off, uint64_t n_sent, uint64_t s, uint64_t &lo, uint64_t &hi) {
  lo = s ? map.tile_of(sent_off[s - 1]) + 1 : 0;
  hi = map.tile_of(sent_off[s]);
  if (s == n_sent) { hi = map.n_tiles; if (lo > hi) lo = hi; }
  else if (hi >= map.n_tiles) hi = map.n_tiles - 1;
}

inline uint64_t tile_count(uint64_t n_bytes, uint32_t tile) { return n_bytes ? (n_bytes + tile - 1) / tile : 1; }

// n_bytes in tiles of `tile` bytes: tile_count(n_bytes, tile) tiles, one for an empty text.
inline TileMap tilemap_uniform(uint64_t n_bytes, uint32_t tile) {
  TileMap m;
  for (int i = 0; i < kTileMapSegs; i++) { m.first_byte[i] = m.first_tile[i] = UINT64_MAX; m.tile_bytes[i] = 0; }
  m.first_byte[0] = m.first_tile[0] = 0;
  m.tile_bytes[0] = tile;
  m.n_segs = 1;
  m.n_tiles = tile_count(n_bytes, tile);
  return m;
}

// The taper.  sizes[0..n_sizes) fall strictly (n_sizes <= kTileMapSegs); c = c8 / 8.  The tile at byte x is the largest size z with
// z <= max(sizes[last], (n_bytes - x) / (c * slots)): tiles of size z are handed out while the bytes that remain are at least
// z * c * slots, what is left goes to the next size, and the smallest size takes the rest.  A size that gets no tile has no
// segment.  All in integers: remaining * 8 >= z * c8 * slots.
inline TileMap tilemap_taper(uint64_t n_bytes, uint64_t slots, uint32_t c8, const uint32_t *sizes, int n_sizes) {
  TileMap m = tilemap_uniform(n_bytes, sizes[0]);
  if (n_bytes == 0 || n_sizes < 2) return m;
  uint64_t x = 0, t = 0;
  int k = 0;
  for (int i = 0; i < n_sizes && x < n_bytes; i++) {
    const uint64_t z = sizes[i], rem = n_bytes - x, thr = z * c8 * slots;  // thr in eighths of a byte
    uint64_t cnt;
    if (i == n_sizes - 1) cnt = (rem + z - 1) / z;
    else if (rem * 8 >= thr) cnt = (rem * 8 - thr) / (8 * z) + 1;
    else continue;
    m.first_byte[k] = x;
    m.first_tile[k] = t;
    m.tile_bytes[k] = (uint32_t)z;
    k++;
    t += cnt;
    x = cnt * z >= rem ? n_bytes : x + cnt * z;  // a last tile that reaches the end of the text ends every segment
  }
  m.n_segs = (uint32_t)k;
  m.n_tiles = t;
  return m;
}

}  // namespace swt
