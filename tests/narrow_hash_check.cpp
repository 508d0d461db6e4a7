// The hash pair of the table of 16-bit codes (narrow_hash, csrc/swt_bpe_narrow.h) on the CPU: compiled and run by
// tests/test_narrow_hash.py, which writes the merge lists.  argv[1] = a list, one merge a line as three symbol ids "left right
// merged" (a code point, or SWT_SYM_BASE + k); argv[2] = the log2 of the slots the table must come out with, 0 for any.
// Exits 0 and prints what it checked, or prints what failed and exits 1.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <vector>

#include "swt_bpe_narrow.h"

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

int main(int argc, char **argv) {
  CHECK(argc == 3, "usage: narrow_hash_check list bits");
  std::FILE *f = std::fopen(argv[1], "r");
  CHECK(f, "cannot open %s", argv[1]);
  std::vector<uint32_t> left, right, merged;
  for (unsigned l, r, m; std::fscanf(f, "%u %u %u", &l, &r, &m) == 3;) { left.push_back(l); right.push_back(r); merged.push_back(m); }
  std::fclose(f);
  const uint32_t n = (uint32_t)left.size(), want_bits = (uint32_t)std::atoi(argv[2]);
  CHECK(n > 0, "an empty list");
  // the last merge of a pair is the one the rank table holds
  std::map<uint64_t, uint32_t> last;
  for (uint32_t i = 0; i < n; i++) last[((uint64_t)left[i] << 32) | right[i]] = i;
  std::vector<bool> live(n);
  for (uint32_t i = 0; i < n; i++) live[i] = last[((uint64_t)left[i] << 32) | right[i]] == i;
  NarrowTable t;
  narrow_build(left.data(), right.data(), merged.data(), n, true, live, t);
  CHECK(t.eligible, "%u merges: not eligible (or not placed)", n);
  CHECK(t.slots.size() == (size_t)1 << t.bits, "%zu slots at %u bits", t.slots.size(), t.bits);
  CHECK(want_bits == 0 || t.bits == want_bits, "2^%u slots, the parent's table had 2^%u", t.bits, want_bits);

  // every live pair finds its value, and the filled slots are the live pairs, each once
  std::map<uint32_t, uint32_t> value_of;  // key -> value
  for (uint32_t i = 0; i < n; i++) {
    if (!live[i]) continue;
    const uint32_t l = t.code(left[i]), r = t.code(right[i]), g = t.code(merged[i]);
    CHECK(l < kNarrowMaxCodes && r < kNarrowMaxCodes && g < kNarrowMaxCodes, "merge %u has codes %x %x %x", i, l, r, g);
    CHECK(t.find(l, r) == ((i << 16) | g), "merge %u found as %08x", i, t.find(l, r));
    value_of[narrow_key(l, r)] = (i << 16) | g;
  }
  size_t filled = 0;
  const uint32_t sh = 32u - t.bits;
  for (size_t s = 0; s < t.slots.size(); s++) {
    const NarrowSlot &e = t.slots[s];
    if (e.key == kNarrowEmptyKey) { CHECK(e.value == 0xFFFFFFFFu, "an empty slot with a value"); continue; }
    filled++;
    auto it = value_of.find(e.key);
    CHECK(it != value_of.end() && it->second == e.value, "slot %zu holds %08x -> %08x, no live pair", s, e.key, e.value);
    const NarrowHash h = narrow_hash(e.key >> 16, e.key & 0xFFFFu, sh);
    CHECK(h.h1 < t.slots.size() && h.h2 < t.slots.size() && (s == h.h1 || s == h.h2), "slot %zu is neither slot of its pair", s);
  }
  CHECK(filled == value_of.size(), "%zu slots filled for %zu live pairs", filled, value_of.size());

  // absent pairs: one operand of a live pair changed, pairs with FOREIGN, pairs anywhere
  std::mt19937 rng(20240229u + n);
  const uint32_t n_codes = t.letters() + n;
  size_t absent = 0;
  auto miss = [&](uint32_t l, uint32_t r) {
    if (value_of.count(narrow_key(l, r))) return;
    CHECK(t.find(l, r) == 0xFFFFFFFFu, "absent pair %x %x found as %08x", l, r, t.find(l, r));
    absent++;
  };
  for (int k = 0; k < 6000; k++) {
    const uint32_t i = rng() % n, l = t.code(left[i]), r = t.code(right[i]);
    miss(l, rng() % n_codes);
    miss(rng() % n_codes, r);
    miss(l, r ^ (1u << (rng() % 15)));  // one bit of one operand
    miss(l ^ (1u << (rng() % 15)), r);
    miss(l, kNarrowForeign);
    miss(kNarrowForeign, r);
    miss(rng() % (kNarrowForeign + 1), rng() % (kNarrowForeign + 1));
  }
  miss(kNarrowForeign, kNarrowForeign);
  miss(kNarrowDead, kNarrowDead);
  std::printf("ok: %u merges, %zu live, %u letters, 2^%u slots, %zu absent pairs\n", n, value_of.size(), t.letters(), t.bits, absent);
  return 0;
}
