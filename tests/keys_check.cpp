// What narrow_build (csrc/swt_bpe_narrow.h) says about how a merge round of the narrow kernel gets the merged code from a rank:
// compiled and run by tests/test_lane_keys.py, once plain and once with -fsanitize=address,undefined.  A list is SEQUENTIAL when the
// code of merged[i] is letters + i for every live merge i; any other eligible list stays eligible and hands the device
// code_of_rank.  Either way find() returns rank << 16 | code of the merged symbol, as before.  argv[1] = a merges.json.
// Exits 0 and prints what it checked, or prints what failed and exits 1.
#include <cstdio>
#include <cstdlib>
#include <map>
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

// a list of pairs of strings, its symbols named as the package names them: one code point (ASCII here) its ordinal, any other
// string SWT_SYM_BASE + k in order of first appearance -- left, right, then the merged string
struct List {
  std::vector<uint32_t> left, right, merged;
  std::map<std::string, uint32_t> index;
  uint32_t id(const std::string &s) {
    if (s.size() == 1) return (uint8_t)s[0];
    auto it = index.find(s);
    if (it == index.end()) it = index.emplace(s, (uint32_t)index.size()).first;
    return kNarrowSymBase + it->second;
  }
  void add(const std::string &l, const std::string &r) {
    const uint32_t a = id(l), b = id(r), g = id(l + r);
    left.push_back(a); right.push_back(b); merged.push_back(g);
  }
  uint32_t n() const { return (uint32_t)left.size(); }
  std::vector<bool> live() const {
    std::map<uint64_t, uint32_t> last;
    for (uint32_t i = 0; i < n(); i++) last[((uint64_t)left[i] << 32) | right[i]] = i;
    std::vector<bool> v(n());
    for (uint32_t i = 0; i < n(); i++) v[i] = last[((uint64_t)left[i] << 32) | right[i]] == i;
    return v;
  }
  NarrowTable build(bool packed = true) const {
    NarrowTable t;
    narrow_build(left.data(), right.data(), merged.data(), n(), packed, live(), t);
    return t;
  }
};

// eligible, sequential as expected, every live merge found under rank << 16 | code, and code_of_rank the code by rank
static void check(const List &m, bool sequential, const char *what) {
  const NarrowTable t = m.build();
  CHECK(t.eligible, "%s: eligible", what);
  CHECK(t.sequential == sequential, "%s: sequential %d", what, (int)t.sequential);
  CHECK(t.code_of_rank.size() == m.n(), "%s: code_of_rank has %zu entries", what, t.code_of_rank.size());
  const std::vector<bool> live = m.live();
  bool seq = true;
  for (uint32_t i = 0; i < m.n(); i++) {
    const uint32_t g = t.code(m.merged[i]);
    if (!live[i]) {
      CHECK(t.code_of_rank[i] == kNarrowDead, "%s: rank %u is not live", what, i);
      continue;
    }
    CHECK(t.find(t.code(m.left[i]), t.code(m.right[i])) == ((i << 16) | g), "%s: merge %u found as %08x", what, i,
          t.find(t.code(m.left[i]), t.code(m.right[i])));
    CHECK(t.code_of_rank[i] == g && g < kNarrowMaxCodes, "%s: code_of_rank[%u] = %x", what, i, t.code_of_rank[i]);
    // what the kernel does with a key: the rank is its high half, the merged code comes from the rank
    const uint32_t key = (t.find(t.code(m.left[i]), t.code(m.right[i])) & 0xFFFF0000u) | 31u;
    CHECK(key < kNarrowNoPair && (key >> 16) == i && (key & 31u) == 31u, "%s: key of merge %u", what, i);
    if (t.sequential) CHECK(t.letters() + (key >> 16) == g, "%s: letters + rank of merge %u", what, i);
    seq = seq && g == t.letters() + i;
  }
  CHECK(seq == sequential, "%s: the condition itself", what);
}

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
        if (cp < 0x80) cur += (char)cp;
        else if (cp < 0x800) { cur += (char)(0xC0 | (cp >> 6)); cur += (char)(0x80 | (cp & 0x3F)); }
        else { cur += (char)(0xE0 | (cp >> 12)); cur += (char)(0x80 | ((cp >> 6) & 0x3F)); cur += (char)(0x80 | (cp & 0x3F)); }
        i += 4;
      } else {
        cur += s[i];
      }
    }
    out.push_back(cur);
  }
  return out;
}
// the symbol of a string of the file: one code point (of any length in UTF-8) its ordinal
static uint32_t file_id(const std::string &s, std::map<std::string, uint32_t> &index) {
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
  CHECK(argc == 2, "usage: keys_check merges.json");
  size_t lists = 0;
  // sequential: every merged string is a new one and no string is spelled before the merge that produces it
  {
    List m;
    for (auto p : {std::pair<const char *, const char *>{"a", "a"}, {"a", "b"}, {"ab", "ab"}, {"aa", "aa"}, {"abab", "abab"}, {"aaaa", "a"}}) m.add(p.first, p.second);
    check(m, true, "equal ranks");
    lists++;
  }
  // not sequential: a pair listed twice keeps its last merge (the earlier one is not live), whose string has the earlier number
  {
    List m;
    m.add("a", "b"); m.add("ab", "c"); m.add("a", "b"); m.add("abc", "d");
    check(m, false, "a pair listed twice");
    CHECK(m.build().find(0, 1) == ((2u << 16) | (4u + 0u)), "the later of a repeated pair: %08x", m.build().find(0, 1));
    lists++;
  }
  // not sequential: "ab" is spelled (and numbered) by the merge before the one that produces it
  {
    List m;
    for (auto p : {std::pair<const char *, const char *>{"ab", "c"}, {"a", "b"}, {"aa", "a"}, {"a", "a"}, {"c", "d"}, {"x", "y"}, {"b", "c"}}) m.add(p.first, p.second);
    check(m, false, "a string spelled before its merge");
    const NarrowTable t = m.build();
    CHECK(t.code_of_rank[0] == t.letters() + 1 && t.code_of_rank[1] == t.letters() + 0, "code_of_rank of the first two: %x %x", t.code_of_rank[0], t.code_of_rank[1]);
    lists++;
  }
  // not sequential: two pairs spell the same string, one symbol for two ranks
  {
    List m;
    m.add("b", "c"); m.add("a", "b"); m.add("a", "bc"); m.add("ab", "c"); m.add("abc", "d");
    check(m, false, "a merged string spelled twice");
    const NarrowTable t = m.build();
    CHECK(t.code_of_rank[2] == t.code_of_rank[3] && t.code_of_rank[2] == t.letters() + 2 && t.code_of_rank[4] == t.letters() + 3, "the codes of ranks 2, 3, 4");
    CHECK(t.find(t.code('a'), t.letters() + 0) == ((2u << 16) | (t.letters() + 2)) && t.find(t.letters() + 1, t.code('c')) == ((3u << 16) | (t.letters() + 2)),
          "both pairs of the repeated string");
    lists++;
  }
  // an ineligible list has neither
  {
    List m;
    m.add("a", "b");
    const NarrowTable t = m.build(false);
    CHECK(!t.eligible && !t.sequential && t.code_of_rank.empty() && t.slots.empty(), "a table that is not packed");
    lists++;
  }
  // the pretrained merges: all merged strings distinct, so the benchmark's table -- any prefix of the list -- is sequential
  std::FILE *f = std::fopen(argv[1], "rb");
  CHECK(f, "cannot open %s", argv[1]);
  std::string text;
  char buf[65536];
  for (size_t got; (got = std::fread(buf, 1, sizeof buf, f)) > 0;) text.append(buf, got);
  std::fclose(f);
  const std::vector<std::string> strs = json_strings(text);
  CHECK(!strs.empty() && strs.size() % 2 == 0, "%zu strings in %s", strs.size(), argv[1]);
  uint32_t n_file = 0;
  for (size_t keep : {(size_t)8000, strs.size() / 2}) {
    List m;
    std::map<std::string, uint32_t> index;
    for (size_t i = 0; i < 2 * keep; i += 2) {
      const uint32_t l = file_id(strs[i], index), r = file_id(strs[i + 1], index), g = file_id(strs[i] + strs[i + 1], index);
      m.left.push_back(l); m.right.push_back(r); m.merged.push_back(g);
    }
    check(m, true, "the merges file");
    n_file = m.n();
    lists++;
  }
  std::printf("ok: %zu lists, %u merges of the file sequential\n", lists, n_file);
  return 0;
}
