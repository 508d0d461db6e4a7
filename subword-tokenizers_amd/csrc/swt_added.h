// swt_added.h -- what the host and the device share of the added-token search (swt_added.hip; include/swt.h has the rule).
//
// The patterns are kept in a byte trie.  Node 0 is the root; its children stand in a dense table by first byte, which is also
// the first-byte reject: root[b] == 0 means that no pattern starts with b, and a text position is done after one load.  Every
// other edge (node, byte) -> child is an entry of one open-addressing table (linear probing, at most half full); end[node] is
// the pattern that ends in the node, plus one, or 0.  The walk from a text position follows at most max_len edges, so the work
// of a position is bounded by the longest pattern and not by the number of patterns.
//
// The header needs nothing of HIP: tests/added_check.cpp includes it in a plain host program.
#pragma once

#include <cstdint>
#include <cstring>
#include <vector>

// host and device under hipcc, nothing in a plain host program
#if defined(__HIPCC__)
#define SWT_ADDED_HD __host__ __device__
#else
#define SWT_ADDED_HD
#endif

namespace swt {

constexpr uint32_t kAddedMaxPatterns = 4096;
constexpr uint32_t kAddedMaxBytes = 64;  // of one pattern

// A view of the tables, host or device pointers alike.
struct AddedTable {
  const uint32_t *root;   // [256]: the child of the root by first byte, 0: none
  const uint64_t *edges;  // [1 << bits]: (node * 256 + byte + 1) << 32 | child, 0: an empty slot
  const uint32_t *end;    // [nodes]: the pattern that ends here + 1, 0: none
  uint32_t bits;
  uint32_t max_len;       // bytes of the longest pattern
};

SWT_ADDED_HD inline uint32_t added_edge_slot(uint32_t key, uint32_t bits) { return (key * 0x9E3779B1u) >> (32 - bits); }

// The longest pattern that matches at p, of which `avail` bytes may be read: its length in bytes, 0 for none; *pat its index.
SWT_ADDED_HD inline uint32_t added_longest(const AddedTable &T, const uint8_t *p, uint32_t avail, uint32_t *pat) {
  if (!avail) return 0;
  uint32_t node = T.root[p[0]];
  if (!node) return 0;
  const uint32_t mask = (1u << T.bits) - 1u, n = avail < T.max_len ? avail : T.max_len;
  uint32_t best = 0, i = 1;
  for (;;) {
    const uint32_t e = T.end[node];
    if (e) { best = i; *pat = e - 1; }
    if (i == n) break;
    const uint32_t key = node * 256u + p[i] + 1u;
    uint32_t slot = added_edge_slot(key, T.bits), child = 0;
    for (;;) {
      const uint64_t v = T.edges[slot];
      if (!v) break;
      if ((uint32_t)(v >> 32) == key) { child = (uint32_t)v; break; }
      slot = (slot + 1) & mask;
    }
    if (!child) break;
    node = child;
    i++;
  }
  return best;
}

// The whitespace bytes that hide one byte of a match from the encoders: a code point is overwritten with a whitespace code
// point of its own UTF-8 length -- U+0020, U+00A0 (C2 A0), U+2003 (E2 80 83).  `lead` is the lead byte of the code point the
// byte belongs to, k the byte's index inside it.
SWT_ADDED_HD inline uint8_t added_blank_byte(uint8_t lead, uint32_t k) {
  if (lead < 0x80) return 0x20;
  if (lead < 0xE0) return k == 0 ? 0xC2 : 0xA0;
  return k == 0 ? 0xE2 : (k == 1 ? 0x80 : 0x83);
}

// The tables on the host.  build() checks the patterns (include/swt.h) and returns null, or why they are refused.
struct AddedHost {
  std::vector<uint32_t> root, end;
  std::vector<uint64_t> edges;
  uint32_t bits = 0, max_len = 0, n_patterns = 0;

  AddedTable view() const { return AddedTable{root.data(), edges.data(), end.data(), bits, max_len}; }

  // strict UTF-8 of code points U+0001 .. U+FFFF without the surrogates; cls (may be null): the class table, whose bit
  // ws_bit marks the code points the pre-tokenizer drops
  static const char *check_pattern(const uint8_t *p, uint64_t n, const uint8_t *cls, uint8_t ws_bit) {
    if (n < 1 || n > kAddedMaxBytes) return "a pattern takes 1 .. 64 bytes";
    for (uint64_t i = 0; i < n;) {
      const uint8_t b = p[i];
      uint32_t cp, len;
      if (b < 0x80) { cp = b; len = 1; }
      else if (b >= 0xC2 && b < 0xE0) { cp = b & 0x1F; len = 2; }
      else if (b >= 0xE0 && b < 0xF0) { cp = b & 0x0F; len = 3; }
      else if (b >= 0xF0 && b < 0xF8) return "a code point past U+FFFF";
      else return "not UTF-8";
      if (i + len > n) return "not UTF-8";
      for (uint32_t k = 1; k < len; k++) {
        if ((p[i + k] & 0xC0) != 0x80) return "not UTF-8";
        cp = (cp << 6) | (p[i + k] & 0x3F);
      }
      if (len == 3 && cp < 0x800) return "not UTF-8";
      if (cp >= 0xD800 && cp < 0xE000) return "a surrogate";
      if (cp == 0) return "U+0000";
      if (cls && (cls[cp] & ws_bit)) return "a whitespace code point";
      i += len;
    }
    return nullptr;
  }

  const char *build(const uint8_t *bytes, const uint64_t *off, uint32_t n, const uint8_t *cls, uint8_t ws_bit) {
    if (n < 1 || n > kAddedMaxPatterns) return "1 .. 4096 patterns";
    uint64_t total = 0;
    for (uint32_t k = 0; k < n; k++) {
      if (off[k + 1] < off[k]) return "offsets must not decrease";
      if (const char *why = check_pattern(bytes + off[k], off[k + 1] - off[k], cls, ws_bit)) return why;
      total += off[k + 1] - off[k];
    }
    bits = 4;
    while ((1ull << bits) < 2 * total + 2) bits++;
    root.assign(256, 0);
    end.assign(1, 0);
    edges.assign((size_t)1 << bits, 0);
    max_len = 0;
    n_patterns = n;
    const uint32_t mask = (1u << bits) - 1u;
    for (uint32_t k = 0; k < n; k++) {
      const uint8_t *p = bytes + off[k];
      const uint32_t len = (uint32_t)(off[k + 1] - off[k]);
      if (len > max_len) max_len = len;
      uint32_t node = root[p[0]];
      if (!node) {
        node = root[p[0]] = (uint32_t)end.size();
        end.push_back(0);
      }
      for (uint32_t i = 1; i < len; i++) {
        const uint32_t key = node * 256u + p[i] + 1u;
        uint32_t slot = added_edge_slot(key, bits);
        while (edges[slot] && (uint32_t)(edges[slot] >> 32) != key) slot = (slot + 1) & mask;
        if (!edges[slot]) {
          edges[slot] = ((uint64_t)key << 32) | (uint32_t)end.size();
          end.push_back(0);
        }
        node = (uint32_t)edges[slot];
      }
      if (end[node]) return "a pattern is given twice";
      end[node] = k + 1;
    }
    return nullptr;
  }
};

}  // namespace swt
