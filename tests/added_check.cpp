// The pattern table and the per-position lookup of the added-token search (csrc/swt_added.h) in a plain host program:
// tests/test_added_table.py writes the cases, builds this with g++ (once more with -fsanitize=address,undefined) and runs it.
//
// Input, one record per line, every string in hex ("-" for the empty one):
//   P <pattern>                                    a pattern of the table that follows
//   B                                              build the table from the patterns read since the last B
//   T <text> <blanked> <n> {<pattern> <start> <length>} * n    a text, what it looks like blanked, its matches in bytes
//   R <pattern>                                    a pattern that build() must refuse by itself
// The matches of a text are made here by the rule of include/swt.h over added_longest: from the left, the longest pattern at the
// first position that has one; on at the match's end.  The blanked text is made with added_blank_byte.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "swt_added.h"

using namespace swt;

static std::vector<uint8_t> unhex(const std::string &s) {
  std::vector<uint8_t> out;
  if (s == "-") return out;
  for (size_t i = 0; i + 1 < s.size(); i += 2) out.push_back((uint8_t)std::stoi(s.substr(i, 2), nullptr, 16));
  return out;
}

static const char *build(AddedHost &H, const std::vector<std::vector<uint8_t>> &pats) {
  std::vector<uint8_t> bytes;
  std::vector<uint64_t> off{0};
  for (const auto &p : pats) {
    bytes.insert(bytes.end(), p.begin(), p.end());
    off.push_back(bytes.size());
  }
  bytes.push_back(0);
  return H.build(bytes.data(), off.data(), (uint32_t)pats.size(), nullptr, 0);
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1]);
  std::string line;
  std::vector<std::vector<uint8_t>> pats;
  AddedHost H;
  bool built = false;
  size_t n_texts = 0, n_matches = 0, n_refused = 0, n_tables = 0;
  while (std::getline(in, line)) {
    std::istringstream ss(line);
    std::string kind, a, b;
    ss >> kind;
    if (kind == "P") {
      ss >> a;
      pats.push_back(unhex(a));
    } else if (kind == "B") {
      if (const char *why = build(H, pats)) { std::printf("FAIL: a table of %zu patterns refused: %s\n", pats.size(), why); return 1; }
      if (H.edges.size() != ((size_t)1 << H.bits) || H.root.size() != 256) { std::printf("FAIL: table shape\n"); return 1; }
      size_t used = 0;
      for (uint64_t e : H.edges) used += e != 0;
      if (2 * used > H.edges.size()) { std::printf("FAIL: the edge table is more than half full\n"); return 1; }
      pats.clear();
      built = true;
      n_tables++;
    } else if (kind == "R") {
      ss >> a;
      AddedHost R;
      if (!build(R, {unhex(a)})) { std::printf("FAIL: pattern %s was not refused\n", a.c_str()); return 1; }
      n_refused++;
    } else if (kind == "T") {
      if (!built) return 2;
      size_t n = 0;
      ss >> a >> b >> n;
      // (an exact copy: the sanitizer sees a read past the text's end)
      const std::vector<uint8_t> text = unhex(a), want_blank = unhex(b);
      std::vector<uint8_t> blank(text);
      const AddedTable T = H.view();
      std::vector<uint32_t> got;
      for (size_t i = 0; i < text.size();) {
        uint32_t pat = 0;
        const uint32_t len = added_longest(T, text.data() + i, (uint32_t)(text.size() - i), &pat);
        if (!len) { i++; continue; }
        got.insert(got.end(), {pat, (uint32_t)i, len});
        uint8_t lead = 0;
        uint32_t k = 0;
        for (uint32_t j = 0; j < len; j++) {
          if ((text[i + j] & 0xC0) != 0x80) { lead = text[i + j]; k = 0; }
          blank[i + j] = added_blank_byte(lead, k++);
        }
        i += len;
      }
      std::vector<uint32_t> want(3 * n);
      for (uint32_t &x : want) ss >> x;
      if (got != want || blank != want_blank) {
        std::printf("FAIL: text %zu (%s): %zu matches, %zu wanted\n", n_texts, a.c_str(), got.size() / 3, n);
        return 1;
      }
      n_texts++;
      n_matches += n;
    }
  }
  std::printf("ok: %zu tables, %zu texts, %zu matches, %zu patterns refused\n", n_tables, n_texts, n_matches, n_refused);
  return 0;
}
