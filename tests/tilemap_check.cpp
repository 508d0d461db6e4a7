// The tile map of the encoders' plan (csrc/swt_tilemap.h) on the CPU: compiled and run by tests/test_tilemap.py, once plain and once
// with -fsanitize=address,undefined.  Exits 0 and prints the number of maps checked, or prints what failed and exits 1.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "swt_tilemap.h"

using namespace swt;

static const uint32_t kSizes[4] = {384, 256, 192, 128};
static unsigned long long g_maps = 0, g_plans = 0;

#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      std::printf("FAILED %s:%d %s\n  ", __FILE__, __LINE__, #cond); \
      std::printf(__VA_ARGS__);                           \
      std::printf("\n");                                  \
      std::exit(1);                                       \
    }                                                     \
  } while (0)

// the rule as the issue states it, one tile at a time: the tile at byte x is the largest size z with z <= max(smallest,
// (n_bytes - x) / (c * slots)), c = c8 / 8
static std::vector<uint64_t> walk(uint64_t n_bytes, uint64_t slots, uint32_t c8, int n_sizes) {
  std::vector<uint64_t> b;
  if (n_bytes == 0) { b.push_back(0); return b; }
  for (uint64_t x = 0; x < n_bytes;) {
    uint64_t z = kSizes[n_sizes - 1];
    for (int i = 0; i < n_sizes; i++)
      if ((uint64_t)kSizes[i] * c8 * slots <= (n_bytes - x) * 8) { z = kSizes[i]; break; }
    b.push_back(x);
    x += z;
  }
  return b;
}

// what every map must satisfy at tile t (and, through the segment edges, everywhere: both directions are piecewise linear)
static void check_tile(const TileMap &m, uint64_t n_bytes, uint64_t t, const char *what) {
  const uint64_t b = m.boundary(t);
  CHECK(m.tile_of(b) == t, "%s: tile_of(boundary(%llu)) = %llu", what, (unsigned long long)t, (unsigned long long)m.tile_of(b));
  if (t == 0) CHECK(b == 0, "%s: boundary(0) = %llu", what, (unsigned long long)b);
  else {
    CHECK(m.tile_of(b - 1) == t - 1, "%s: tile_of(boundary(%llu) - 1) = %llu", what, (unsigned long long)t, (unsigned long long)m.tile_of(b - 1));
    CHECK(m.boundary(t - 1) < b && b - m.boundary(t - 1) <= 384, "%s: tile %llu is %llu bytes", what, (unsigned long long)(t - 1),
          (unsigned long long)(b - m.boundary(t - 1)));
  }
  if (t + 1 < m.n_tiles) CHECK(m.boundary(t + 1) > b && m.boundary(t + 1) - b <= 384, "%s: tile %llu", what, (unsigned long long)t);
  else CHECK((n_bytes == 0 && b == 0) || (b < n_bytes && n_bytes - b <= 384), "%s: the last tile begins at %llu of %llu", what, (unsigned long long)b,
             (unsigned long long)n_bytes);
}

static void check_map(const TileMap &m, uint64_t n_bytes, const char *what) {
  g_maps++;
  CHECK(m.n_tiles >= 1 && m.n_segs >= 1 && m.n_segs <= (uint32_t)kTileMapSegs, "%s: %llu tiles, %u segments", what, (unsigned long long)m.n_tiles, m.n_segs);
  CHECK(m.first_byte[0] == 0 && m.first_tile[0] == 0, "%s: segment 0", what);
  std::vector<uint64_t> ts;
  if (m.n_tiles <= 4096) {
    for (uint64_t t = 0; t < m.n_tiles; t++) ts.push_back(t);
  } else {
    std::mt19937_64 rng(n_bytes * 31 + m.n_tiles);
    for (int i = 0; i < 256; i++) ts.push_back(rng() % m.n_tiles);
    for (uint32_t k = 0; k < m.n_segs; k++)
      for (int d = -3; d <= 3; d++) {
        const uint64_t t = m.first_tile[k] + (uint64_t)(int64_t)d;
        if (t < m.n_tiles) ts.push_back(t);
      }
    for (uint64_t t = m.n_tiles - 4; t < m.n_tiles; t++) ts.push_back(t);
  }
  for (uint64_t t : ts) check_tile(m, n_bytes, t, what);
  for (uint32_t k = 0; k < m.n_segs; k++) {
    CHECK(m.tile_bytes[k] >= 128 && m.tile_bytes[k] <= 1024 * 16, "%s: segment %u has tiles of %u", what, k, m.tile_bytes[k]);
    if (k) CHECK(m.first_tile[k] > m.first_tile[k - 1] && m.first_byte[k] > m.first_byte[k - 1] && m.tile_bytes[k] < m.tile_bytes[k - 1] &&
                 m.first_byte[k] - m.first_byte[k - 1] == (m.first_tile[k] - m.first_tile[k - 1]) * m.tile_bytes[k - 1],
                 "%s: segment %u does not hold whole tiles or is empty", what, k);
  }
  if (n_bytes) CHECK(m.tile_of(n_bytes - 1) == m.n_tiles - 1, "%s: the last byte is in tile %llu of %llu", what,
                     (unsigned long long)m.tile_of(n_bytes - 1), (unsigned long long)m.n_tiles);
}

// plan[] by both forms of the plan kernels against a plain lower bound over the boundaries
static void check_plan(const TileMap &m, const std::vector<uint64_t> &off, const char *what) {
  g_plans++;
  const uint64_t n_sent = off.size() - 1, nt = m.n_tiles;
  std::vector<uint64_t> want(nt + 1), pass(nt + 1, UINT64_MAX);
  for (uint64_t t = 0; t < nt; t++) want[t] = (uint64_t)(std::lower_bound(off.begin(), off.begin() + n_sent, m.boundary(t)) - off.begin());
  want[nt] = n_sent;
  for (uint64_t s = 0; s <= n_sent; s++) {
    uint64_t lo, hi;
    plan_range(m, off.data(), n_sent, s, lo, hi);
    for (uint64_t t = lo; t <= hi; t++) {  // hi <= n_tiles always; an empty range has lo > hi
      CHECK(t <= nt, "%s: the pass writes plan[%llu] of %llu", what, (unsigned long long)t, (unsigned long long)nt);
      CHECK(pass[t] == UINT64_MAX, "%s: plan[%llu] is written twice (sentences %llu and %llu)", what, (unsigned long long)t,
            (unsigned long long)pass[t], (unsigned long long)s);
      pass[t] = s;
    }
  }
  for (uint64_t t = 0; t <= nt; t++) {
    CHECK(pass[t] == want[t], "%s: the pass gives plan[%llu] = %llu, the lower bound %llu", what, (unsigned long long)t,
          (unsigned long long)pass[t], (unsigned long long)want[t]);
    const uint64_t srch = plan_search(m, off.data(), n_sent, t);
    CHECK(srch == want[t], "%s: the search gives plan[%llu] = %llu, the lower bound %llu", what, (unsigned long long)t,
          (unsigned long long)srch, (unsigned long long)want[t]);
  }
}

static void check_plans(const TileMap &m, uint64_t n_bytes, std::mt19937_64 &rng, const char *what) {
  if (m.n_tiles > 2048 || n_bytes == 0) return;
  std::vector<uint64_t> off;
  // random offsets, some of them repeated (empty sentences) and some on a boundary
  const int n = 1 + (int)(rng() % 200);
  for (int i = 0; i < n; i++) {
    const uint64_t r = rng();
    off.push_back((r & 3) == 0 ? m.boundary((r >> 8) % m.n_tiles) : (r >> 8) % (n_bytes + 1));
    if ((r & 12) == 0) off.push_back(off.back());
  }
  off.push_back(0);
  std::sort(off.begin(), off.end());
  off.push_back(n_bytes);
  check_plan(m, off, what);
  // 300 empty sentences at one offset (a boundary, a byte before it and a byte behind it), text before and behind them
  for (int d = -1; d <= 1; d++) {
    const uint64_t b = m.boundary((rng() >> 8) % m.n_tiles);
    const uint64_t at = std::min<uint64_t>(n_bytes, b == 0 && d < 0 ? 0 : b + (uint64_t)(int64_t)d);
    std::vector<uint64_t> e(1, 0);
    for (int i = 0; i < 301; i++) e.push_back(at);
    e.push_back(n_bytes);
    check_plan(m, e, what);
  }
  // one sentence over all tiles
  check_plan(m, std::vector<uint64_t>{0, n_bytes}, what);
}

int main() {
  std::mt19937_64 rng(384512);
  char what[160];
  // uniform maps are t * tile and x / tile, with tile_count() tiles
  for (uint32_t tile : {128u, 256u, 384u, 768u, 1024u, 6144u})
    for (uint64_t n : {0ull, 1ull, 127ull, 128ull, 129ull, 383ull, 384ull, 385ull, 767ull, 768ull, 769ull, 1025ull, 8526871ull, (1ull << 40) + 5}) {
      const TileMap m = tilemap_uniform(n, tile);
      std::snprintf(what, sizeof what, "uniform n=%llu tile=%u", (unsigned long long)n, tile);
      CHECK(m.n_tiles == tile_count(n, tile) && m.n_segs == 1, "%s: %llu tiles", what, (unsigned long long)m.n_tiles);
      for (uint64_t t : {0ull, 1ull, 2ull, (unsigned long long)(m.n_tiles / 2), (unsigned long long)(m.n_tiles - 1), (unsigned long long)m.n_tiles})
        CHECK(m.boundary(t) == t * tile, "%s: boundary(%llu)", what, (unsigned long long)t);
      for (uint64_t x : {0ull, 1ull, (unsigned long long)tile - 1, (unsigned long long)tile, (unsigned long long)(n / 2), (unsigned long long)n})
        CHECK(m.tile_of(x) == x / tile, "%s: tile_of(%llu)", what, (unsigned long long)x);
      if (tile <= 384) check_map(m, n, what);
      if (tile <= 384) check_plans(m, n, rng, what);
    }
  // the taper: every c the option takes (c8 = 2..64), with 128 and with 192 bytes as the smallest size
  for (uint64_t slots : {1ull, 2ull, 3ull, 7ull, 6400ull, 10000ull})
    for (int n_sizes : {4, 3})
      for (uint32_t c8 = 2; c8 <= 64; c8++) {
        std::vector<uint64_t> ns = {0, 1, 127, 128, 129, 191, 192, 193, 255, 256, 257, 383, 384, 385, 1025, 1100, 8192, 8526871, 1ull << 32, (1ull << 32) + 1,
                                    (1ull << 40) - 1, 1ull << 40, (1ull << 40) + 77};
        for (int i = 0; i < n_sizes; i++) {
          const uint64_t thr8 = (uint64_t)kSizes[i] * c8 * slots;  // the threshold of size i in eighths of a byte
          for (uint64_t base : {thr8 / 8, (thr8 + 7) / 8})
            for (int d = -1; d <= 1; d++) {
              const uint64_t v = base + (uint64_t)(int64_t)d;
              if (v <= (1ull << 41)) { ns.push_back(v); ns.push_back(v + kSizes[i]); ns.push_back(v + 3 * kSizes[0] + 5); }
            }
        }
        for (uint64_t n : ns) {
          const TileMap m = tilemap_taper(n, slots, c8, kSizes, n_sizes);
          std::snprintf(what, sizeof what, "taper n=%llu slots=%llu c8=%u sizes=%d", (unsigned long long)n, (unsigned long long)slots, c8, n_sizes);
          check_map(m, n, what);
          for (uint32_t k = 0; k < m.n_segs; k++) {
            bool known = false;
            for (int i = 0; i < n_sizes; i++) known |= m.tile_bytes[k] == kSizes[i];
            CHECK(known, "%s: tiles of %u bytes", what, m.tile_bytes[k]);
          }
          if (n <= (4ull << 20)) {  // the rule itself, tile by tile: n_tiles is the count of boundaries, and every boundary is the rule's
            const std::vector<uint64_t> b = walk(n, slots, c8, n_sizes);
            CHECK(b.size() == m.n_tiles, "%s: %llu tiles, the rule gives %llu", what, (unsigned long long)m.n_tiles, (unsigned long long)b.size());
            for (uint64_t t = 0; t < m.n_tiles; t++)
              CHECK(m.boundary(t) == b[t], "%s: boundary(%llu) = %llu, the rule gives %llu", what, (unsigned long long)t,
                    (unsigned long long)m.boundary(t), (unsigned long long)b[t]);
          }
          if ((c8 & 3) == 0 || c8 < 8) check_plans(m, n, rng, what);
        }
      }
  std::printf("ok: %llu maps, %llu plans\n", g_maps, g_plans);
  return 0;
}
