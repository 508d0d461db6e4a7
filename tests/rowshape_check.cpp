// The launch geometry of the row kernels (csrc/swt_rows.h) on the CPU: compiled and run by tests/test_rowshape.py, once plain and
// once with -fsanitize=address,undefined.  Exits 0 and prints the number of shapes checked, or prints what failed and exits 1.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "swt_rows.h"

using namespace swt;

#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      std::printf("FAILED %s:%d %s\n  ", __FILE__, __LINE__, #cond); \
      std::printf(__VA_ARGS__);                           \
      std::printf("\n");                                  \
      std::exit(1);                                       \
    }                                                     \
  } while (0)

int main() {
  const uint32_t waves = 4;
  std::vector<uint32_t> widths = {0x7FFFFFFFu};
  for (uint32_t w = 1; w <= 9; w++) widths.push_back(w);
  for (uint32_t c : {16u, 64u, 256u})
    for (uint32_t w = c - 1; w <= c + 1; w++) widths.push_back(w);
  std::vector<uint64_t> rows = {0, 1, 63, 64, 65, 1ull << 28, (1ull << 32) - 1};
  for (uint64_t c : {1ull << 20, 1ull << 24})
    for (uint64_t r = c - 1; r <= c + 1; r++) rows.push_back(r);
  unsigned long long n = 0, doubled = 0;
  for (uint32_t width : widths) {
    const uint32_t g = bt_group(width);
    CHECK(g >= 1 && g <= 64 && (g & (g - 1)) == 0, "width %u: group %u", width, g);
    // the smallest power of two with 4 g >= width, or 64
    CHECK((uint64_t)kBtQuad * g >= width || g == 64, "width %u: group %u does not cover the row", width, g);
    CHECK(g == 1 || (uint64_t)kBtQuad * (g / 2) < width, "width %u: group %u, half of it would do", width, g);
    for (uint64_t r : rows) {
      const RowShape s = bt_shape(r, g, waves);
      const uint64_t first = g >= 16 ? 1 : 4, per_set = (uint64_t)waves * (64 / g);
      n++;
      doubled += s.sets > first;
      // 1 or 4, doubled only while the grid would exceed 2^20
      CHECK(s.sets >= first && s.sets % first == 0 && ((s.sets / first) & (s.sets / first - 1)) == 0, "width %u rows %llu: %llu sets", width,
            (unsigned long long)r, (unsigned long long)s.sets);
      if (s.sets > first) {
        const uint64_t half = per_set * (s.sets / 2);
        CHECK(r / half + (r % half != 0) > kBtMaxGrid, "width %u rows %llu: %llu sets where half as many fit the grid", width,
              (unsigned long long)r, (unsigned long long)s.sets);
      }
      CHECK(s.sets <= 0xFFFFFFFFull, "width %u rows %llu: %llu sets do not fit 32 bits", width, (unsigned long long)r, (unsigned long long)s.sets);
      CHECK(s.grid <= kBtMaxGrid, "width %u rows %llu: a grid of %u", width, (unsigned long long)r, s.grid);
      // the grid covers the rows, and one workgroup fewer would not; nothing here overflows: 2^20 * 4 * 64 * sets < 2^64
      const uint64_t per_block = per_set * s.sets;
      CHECK(per_block <= (1ull << 40), "width %u rows %llu: %llu rows a workgroup", width, (unsigned long long)r, (unsigned long long)per_block);
      CHECK((uint64_t)s.grid * per_block >= r, "width %u rows %llu: grid %u of %llu rows each", width, (unsigned long long)r, s.grid,
            (unsigned long long)per_block);
      CHECK(s.grid == 0 ? r == 0 : (uint64_t)(s.grid - 1) * per_block < r, "width %u rows %llu: grid %u, one fewer would do", width,
            (unsigned long long)r, s.grid);
    }
  }
  CHECK(doubled > 0, "no shape reached the doubling of the sets");
  std::printf("ok: %llu shapes, %llu with doubled sets\n", n, doubled);
  return 0;
}
