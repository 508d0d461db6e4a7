// The 16-bit symbol codes of the FastBPE lane kernel (csrc/swt_bpe_narrow.h) on the CPU: compiled and run by
// tests/test_lane_narrow.py, once plain and once with -fsanitize=address,undefined.  argv[1] = a merges.json (a list of pairs of
// strings).  Exits 0 and prints what it checked, or prints what failed and exits 1.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <set>
#include <string>
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

struct Merges {
  std::vector<uint32_t> left, right, merged;
  uint32_t n() const { return (uint32_t)left.size(); }
  void add(uint32_t l, uint32_t r, uint32_t m) { left.push_back(l); right.push_back(r); merged.push_back(m); }
  // the last merge of a pair is the one the rank table holds
  std::vector<bool> live() const {
    std::map<uint64_t, uint32_t> last;
    for (uint32_t i = 0; i < n(); i++) last[((uint64_t)left[i] << 32) | right[i]] = i;
    std::vector<bool> v(n());
    for (uint32_t i = 0; i < n(); i++) v[i] = last[((uint64_t)left[i] << 32) | right[i]] == i;
    return v;
  }
  NarrowTable build(bool packed) const {
    NarrowTable t;
    narrow_build(left.data(), right.data(), merged.data(), n(), packed, live(), t);
    return t;
  }
};

// every live merge is found under its codes with value rank << 16 | code of the merged symbol; the slots hold nothing else
static void check_finds(const Merges &m, const NarrowTable &t, const char *what) {
  const std::vector<bool> live = m.live();
  size_t n_live = 0, filled = 0;
  for (uint32_t i = 0; i < m.n(); i++) {
    const uint32_t l = t.code(m.left[i]), r = t.code(m.right[i]), g = t.code(m.merged[i]);
    CHECK(l < kNarrowMaxCodes && r < kNarrowMaxCodes && g < kNarrowMaxCodes, "%s: merge %u has codes %x %x %x", what, i, l, r, g);
    if (!live[i]) continue;
    n_live++;
    CHECK(t.find(l, r) == ((i << 16) | g), "%s: merge %u found as %08x", what, i, t.find(l, r));
  }
  for (const NarrowSlot &s : t.slots) filled += s.key != kNarrowEmptyKey;
  CHECK(filled == n_live && t.slots.size() == (size_t)1 << t.bits, "%s: %zu slots filled for %zu pairs", what, filled, n_live);
}

static void check_alphabet(const Merges &m, const NarrowTable &t, const char *what) {
  std::set<uint32_t> want;
  for (uint32_t i = 0; i < m.n(); i++)
    for (uint32_t s : {m.left[i], m.right[i]})
      if (s < kNarrowSymBase) want.insert(s);
  CHECK(std::vector<uint32_t>(want.begin(), want.end()) == t.cp_of_code, "%s: the alphabet is not the ascending set of base code points", what);
  for (uint32_t c = 0; c < t.letters(); c++) CHECK(t.code(t.cp_of_code[c]) == c, "%s: letter %u", what, c);
  for (uint32_t c = 1; c < t.letters(); c++) CHECK(t.cp_of_code[c - 1] < t.cp_of_code[c], "%s: order at %u", what, c);
  CHECK(t.code(kNarrowSymBase) == t.letters() && t.code(kNarrowSymBase + 7) == t.letters() + 7, "%s: merged symbols", what);
  // code | class << 16 per code point: every letter its code, everything else FOREIGN, the class bits those of the table given
  std::vector<uint8_t> cls(t.n_cps());
  for (size_t i = 0; i < cls.size(); i++) cls[i] = (uint8_t)((i * 7u) & 0xFFu);
  const std::vector<uint32_t> e = t.code_of_cp(cls.data()), e0 = t.code_of_cp(nullptr);
  CHECK(e.size() == t.n_cps() && e.size() >= kNarrowMinCps && e.size() > (t.letters() ? t.cp_of_code.back() : 0u), "%s: n_cps", what);
  for (uint32_t cp = 0; cp < (uint32_t)e.size(); cp++) {
    CHECK((e[cp] & 0xFFFFu) == t.code(cp) && (e[cp] >> 16) == (cls[cp] & 3u) && e0[cp] == t.code(cp), "%s: code_of_cp[%u] = %08x", what, cp, e[cp]);
    CHECK(want.count(cp) ? (e[cp] & 0xFFFFu) < t.letters() : (e[cp] & 0xFFFFu) == kNarrowForeign, "%s: code point %u", what, cp);
  }
}

// chain merges over the letters `alpha`: (alpha[0], alpha[1]) -> S0, then (S(k-1), alpha[k % A]) -> Sk
static Merges chain(const std::vector<uint32_t> &alpha, uint32_t n) {
  Merges m;
  for (uint32_t k = 0; k < n; k++) m.add(k ? kNarrowSymBase + k - 1 : alpha[0], alpha[k ? k % alpha.size() : 1], kNarrowSymBase + k);
  return m;
}

// ---- a merges.json: [["a", "b"], ...], symbols named as the package names them (one code point: its ordinal; else
// SWT_SYM_BASE + k in order of first appearance)
static std::vector<std::string> json_strings(const std::string &s) {
  std::vector<std::string> out;
  for (size_t i = 0; i < s.size(); i++) {
    if (s[i] != '"') continue;
    std::string cur;
    for (i++; i < s.size() && s[i] != '"'; i++) {
      if (s[i] != '\\') { cur += s[i]; continue; }
      i++;
      CHECK(i < s.size(), "a backslash ends the file");
      if (s[i] == 'u') {
        CHECK(i + 4 < s.size(), "a short \\u escape");
        const uint32_t cp = (uint32_t)std::strtoul(s.substr(i + 1, 4).c_str(), nullptr, 16);
        CHECK(cp < 0xD800 || cp >= 0xE000, "surrogate escapes are not expected in a merges file");
        if (cp < 0x80) cur += (char)cp;
        else if (cp < 0x800) { cur += (char)(0xC0 | (cp >> 6)); cur += (char)(0x80 | (cp & 0x3F)); }
        else { cur += (char)(0xE0 | (cp >> 12)); cur += (char)(0x80 | ((cp >> 6) & 0x3F)); cur += (char)(0x80 | (cp & 0x3F)); }
        i += 4;
      } else {
        cur += s[i];  // \" \\ \/
      }
    }
    out.push_back(cur);
  }
  return out;
}
static uint32_t intern(const std::string &s, std::map<std::string, uint32_t> &index) {
  size_t n_cp = 0;
  uint32_t cp = 0;
  for (size_t i = 0; i < s.size();) {
    const uint8_t b = (uint8_t)s[i];
    const int len = b < 0x80 ? 1 : b < 0xE0 ? 2 : b < 0xF0 ? 3 : 4;
    cp = len == 1 ? b : (uint32_t)(b & (0xFF >> (len + 1)));
    for (int k = 1; k < len && i + k < s.size(); k++) cp = (cp << 6) | ((uint8_t)s[i + k] & 0x3F);
    i += len;
    n_cp++;
  }
  if (n_cp == 1) return cp;
  auto it = index.find(s);
  if (it == index.end()) it = index.emplace(s, (uint32_t)index.size()).first;
  return kNarrowSymBase + it->second;
}

int main(int argc, char **argv) {
  CHECK(argc == 2, "usage: narrow_check merges.json");
  // 1. a small list by hand: the alphabet comes out ascending whatever the order of the list, a pair listed twice keeps its last
  {
    Merges m;
    m.add(0x142, 'z', kNarrowSymBase + 0);                    // ł z
    m.add('a', 'b', kNarrowSymBase + 1);
    m.add(kNarrowSymBase + 1, 0x1F600, kNarrowSymBase + 2);   // ab + an emoji
    m.add('a', 'b', kNarrowSymBase + 3);                      // listed again: the table holds this one
    m.add('b', 'a', kNarrowSymBase + 4);
    const NarrowTable t = m.build(true);
    CHECK(t.eligible, "the small list");
    CHECK((t.cp_of_code == std::vector<uint32_t>{'a', 'b', 'z', 0x142, 0x1F600}), "alphabet of the small list");
    check_alphabet(m, t, "small");
    check_finds(m, t, "small");
    CHECK(t.find(t.code('a'), t.code('b')) == ((3u << 16) | (t.letters() + 3)), "the later of a repeated pair");
    CHECK(t.find(t.code('a'), t.code('z')) == 0xFFFFFFFFu && t.find(kNarrowForeign, t.code('a')) == 0xFFFFFFFFu, "absent pairs");
    CHECK(t.code('c') == kNarrowForeign && t.code(0x10FFFF) == kNarrowForeign && t.code(0) == kNarrowForeign, "foreign code points");
    CHECK(!m.build(false).eligible && m.build(false).slots.empty(), "a table that is not packed");
  }
  // 2. the bound: letters + merges <= 0x7FFD, for alphabets of 2, 3 and 45 letters
  size_t bounds = 0;
  for (uint32_t a : {2u, 3u, 45u}) {
    std::vector<uint32_t> alpha;
    for (uint32_t k = 0; k < a; k++) alpha.push_back(k % 2 ? 0x400 + k : 'a' + k);
    for (int d = -1; d <= 1; d++) {
      const Merges m = chain(alpha, kNarrowMaxCodes - a + d);
      const NarrowTable t = m.build(true);
      CHECK(t.eligible == (d <= 0), "%u letters + %u merges: eligible %d", a, m.n(), (int)t.eligible);
      if (t.eligible) {
        CHECK(t.letters() == a && t.letters() + m.n() <= kNarrowMaxCodes, "letters");
        check_alphabet(m, t, "chain");
        check_finds(m, t, "chain");
      } else {
        CHECK(t.slots.empty() && t.cp_of_code.empty(), "an ineligible table is empty");
      }
      bounds++;
    }
  }
  {
    // a symbol named far above the merges counts too: its code would not fit
    Merges m = chain({'a', 'b'}, 10);
    m.add('a', kNarrowSymBase + 0x7FFB, kNarrowSymBase + 10);
    CHECK(!m.build(true).eligible, "a symbol whose code does not fit");
    Merges ok = chain({'a', 'b'}, 10);
    ok.add('a', kNarrowSymBase + 0x7FF9, kNarrowSymBase + 10);
    CHECK(ok.build(true).eligible, "a symbol whose code just fits");
    check_finds(ok, ok.build(true), "high symbol");
  }
  // 3. the merges file: every merge found, 10,000 absent pairs missed
  std::FILE *f = std::fopen(argv[1], "rb");
  CHECK(f, "cannot open %s", argv[1]);
  std::string text;
  char buf[65536];
  for (size_t got; (got = std::fread(buf, 1, sizeof buf, f)) > 0;) text.append(buf, got);
  std::fclose(f);
  const std::vector<std::string> strs = json_strings(text);
  CHECK(!strs.empty() && strs.size() % 2 == 0, "%zu strings in %s", strs.size(), argv[1]);
  Merges m;
  std::map<std::string, uint32_t> index;
  for (size_t i = 0; i < strs.size(); i += 2) {
    const uint32_t l = intern(strs[i], index), r = intern(strs[i + 1], index), g = intern(strs[i] + strs[i + 1], index);
    m.add(l, r, g);
  }
  const NarrowTable t = m.build(true);
  CHECK(t.eligible, "%u merges over %u letters", m.n(), t.letters());
  check_alphabet(m, t, "file");
  check_finds(m, t, "file");
  std::set<uint32_t> keys;
  for (uint32_t i = 0; i < m.n(); i++) keys.insert(narrow_key(t.code(m.left[i]), t.code(m.right[i])));
  std::mt19937 rng(10000);
  const uint32_t n_codes = t.letters() + m.n();
  size_t absent = 0;
  while (absent < 10000) {
    // half of them near the table's own pairs (one member changed), half anywhere, FOREIGN included
    uint32_t l, r;
    if (absent % 2) { const uint32_t i = rng() % m.n(); l = t.code(m.left[i]); r = rng() % n_codes; }
    else { l = rng() % (kNarrowForeign + 1); r = rng() % (kNarrowForeign + 1); }
    if (keys.count(narrow_key(l, r))) continue;
    CHECK(t.find(l, r) == 0xFFFFFFFFu, "absent pair %x %x found as %08x", l, r, t.find(l, r));
    absent++;
  }
  std::printf("ok: %u merges of the file over %u letters in 2^%u slots, %zu absent pairs, %zu bounds\n", m.n(), t.letters(), t.bits, absent, bounds);
  return 0;
}
