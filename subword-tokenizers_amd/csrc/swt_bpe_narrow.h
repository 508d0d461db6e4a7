// swt_bpe_narrow.h -- 16-bit symbol codes for bpe_lane_kernel (swt_bpe_encode.hip), built on the host.
//
// The lane kernel keeps a chunk's symbols in LDS.  A symbol id is a code point or SWT_SYM_BASE + k and needs 32 bits; a table
// below 32 k symbols can number its own symbols in 15:
//   0 .. A-1    the letters: the distinct base code points (ids below SWT_SYM_BASE) that are the left or the right of a merge,
//               ascending
//   A + k       the symbol SWT_SYM_BASE + k
//   0x7FFE      FOREIGN: a code point outside the alphabet.  No pair holds it, so it never merges
//   0x7FFF      a consumed slot
//   bit 15      SWT_BPE_CONT
// The rank table of the codes is a two-choice cuckoo table as the one of the ids is (two slots a pair), keyed on l << 16 | r, exact
// in 32 bits: a slot is {key, value} in 8 bytes, value = rank << 16 | code of the merged symbol.  Its two hashes are its own
// (narrow_hash): they share their first stage, which 15-bit codes allow and the ids of the wide table (bpe_hash) do not.
//
// The kernel's val[] entry of a pair is the round's KEY, rank << 16 | the slot's index in its word (slot_key, swt_bpe_encode.hip):
// only the rank half of a table value gets there, and a round learns the merged code from the rank.  Where the list's live merge i
// produces the symbol SWT_SYM_BASE + i (any list whose merged strings are all new ones, every trained list) that is one add,
// letters + rank (NarrowTable::sequential); any other eligible list reads code_of_rank[rank].
//
// Nothing from HIP is included here: a CPU test compiles this header with g++ (tests/test_lane_narrow.py).
#pragma once

#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SWT_NARROW_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define SWT_NARROW_HD inline
#endif

namespace swt {

// The hashes of the rank table of the IDS (and of NaiveBPE's table of first positions): 24-bit multiplies (full-rate v_mul_u32_u24; symbol ids are below 2^24 for any table under five
// million merges, larger ids only hash worse) with one xor-shift between them.
struct BpeHash { uint32_t a, b, c; };
constexpr BpeHash kHash1{0x9E3779u, 0x85EBCBu, 0xC2B2AFu}, kHash2{0x27D4EBu, 0x165667u, 0x9E3779u};
SWT_NARROW_HD uint32_t bpe_hash(uint32_t l, uint32_t r, uint32_t sh, BpeHash k) {
  uint32_t x = (l & 0xFFFFFFu) * k.a + (r & 0xFFFFFFu) * k.b;
  x ^= x >> 16;
  return ((x & 0xFFFFFFu) * k.c) >> sh;   // sh = 32 - log2(slots)
}

constexpr uint32_t kNarrowSymBase = 0x110000u;  // SWT_SYM_BASE (include/swt.h; swt_bpe_encode.hip asserts that they agree)
constexpr uint32_t kNarrowCont = 0x8000u, kNarrowDead = 0x7FFFu, kNarrowForeign = 0x7FFEu;
constexpr uint32_t kNarrowMaxCodes = 0x7FFDu;   // letters + merges of an eligible table: its codes end below 0x7FFD
constexpr uint32_t kNarrowEmptyKey = 0xFFFFFFFFu;  // l = 0xFFFF is no code
// val[] of a FOREIGN symbol holds its code point (21 bits) under this bit.  Ranks of an eligible table are below 0x7FFD, so any
// value from here up is "no pair", as kNoRank (all ones) is.
constexpr uint32_t kNarrowNoPair = 0x80000000u, kNarrowCpMask = 0x1FFFFFu;
constexpr uint32_t kNarrowMinCps = 1024;  // code_of_cp covers at least the code points the class copy in LDS covers

struct NarrowSlot { uint32_t key, value; };
SWT_NARROW_HD uint32_t narrow_key(uint32_t l, uint32_t r) { return (l << 16) | r; }

// The two slots of a pair of CODES.  One multiply chain serves both: x = l * A + r * B (a v_mul_u32_u24 and a v_mad_u32_u24),
// the first slot is the top of x, the second the top of x's low 24 bits times C -- five vector instructions where two calls of
// bpe_hash take ten.  Codes are below 2^15 and differ in few bits, so the top bits of one odd multiply spread them as well as
// bpe_hash's xor-shift did: the pretrained lists settle in tables of the same size (tests/test_narrow_hash.py).  sh = 32 - log2(slots).
struct NarrowHash { uint32_t h1, h2; };
constexpr uint32_t kNarrowHashA = 0x9E3779u, kNarrowHashB = 0x85EBCBu, kNarrowHashC = 0xC2B2AFu;
SWT_NARROW_HD NarrowHash narrow_hash(uint32_t l, uint32_t r, uint32_t sh) {
  const uint32_t x = (l & 0xFFFFFFu) * kNarrowHashA + (r & 0xFFFFFFu) * kNarrowHashB;
  return NarrowHash{x >> sh, ((x & 0xFFFFFFu) * kNarrowHashC) >> sh};
}

// Every eligible table runs the narrow kernel with keys in val[].  `sequential` only says how a round gets the merged code from
// the rank: letters + rank, or (a list that spells a merged string before the merge producing it, or twice) code_of_rank[rank],
// which the device reads from memory.  No table loses its eligibility to the keys and the value form of a slot stays what it was.
struct NarrowTable {
  bool eligible = false;
  bool sequential = false;             // code(merged[i]) == letters + i for every live merge i
  std::vector<uint32_t> code_of_rank;  // [n_merges] code(merged[i]) of a live merge, kNarrowDead of any other
  std::vector<uint32_t> cp_of_code;  // the alphabet, ascending
  std::vector<NarrowSlot> slots;
  uint32_t bits = 0;

  uint32_t letters() const { return (uint32_t)cp_of_code.size(); }
  // the code of symbol id `s`, kNarrowForeign for a code point outside the alphabet
  uint32_t code(uint32_t s) const {
    if (s >= kNarrowSymBase) return letters() + (s - kNarrowSymBase);
    auto it = std::lower_bound(cp_of_code.begin(), cp_of_code.end(), s);
    return it != cp_of_code.end() && *it == s ? (uint32_t)(it - cp_of_code.begin()) : kNarrowForeign;
  }
  // what the device reads per code point below n_cps(): code | class << 16 (`cls`: the class table, SWT_CLS_* bits, or null)
  uint32_t n_cps() const { return std::max(kNarrowMinCps, cp_of_code.empty() ? 0u : cp_of_code.back() + 1u); }
  std::vector<uint32_t> code_of_cp(const uint8_t *cls) const {
    std::vector<uint32_t> v(n_cps());
    for (uint32_t cp = 0; cp < (uint32_t)v.size(); cp++) v[cp] = kNarrowForeign | (cls ? (uint32_t)(cls[cp] & 3u) << 16 : 0u);
    for (uint32_t c = 0; c < letters(); c++) v[cp_of_code[c]] = (v[cp_of_code[c]] & 0xFFFF0000u) | c;
    return v;
  }
  // the value of the pair of CODES (l, r) as a device lookup finds it, all ones when the table has no such pair
  uint32_t find(uint32_t l, uint32_t r) const {
    const uint32_t sh = 32u - bits, key = narrow_key(l, r);
    const NarrowHash h = narrow_hash(l, r, sh);
    const NarrowSlot &a = slots[h.h1], &b = slots[h.h2];
    return (a.key == key ? a.value : 0xFFFFFFFFu) & (b.key == key ? b.value : 0xFFFFFFFFu);
  }
};

// Two-choice cuckoo placement over narrow_hash, as place_slots (swt_bpe_encode.hip) does it for the ids: first slot, second slot, else evict (but
// not from the slot the entry was just evicted from); a table that does not settle gets twice the slots.
inline bool narrow_place(const std::vector<NarrowSlot> &entries, std::vector<NarrowSlot> &slots, uint32_t &bits_out) {
  uint32_t bits = 4;
  while ((1ull << bits) < 2ull * entries.size() + 2) bits++;
  const uint32_t bits0 = bits;
  for (;; bits++) {
    if (bits > 28 || bits > bits0 + 4) return false;
    const uint32_t sh = 32u - bits;
    slots.assign((size_t)1 << bits, NarrowSlot{kNarrowEmptyKey, 0xFFFFFFFFu});
    bool ok = true;
    for (size_t i = 0; i < entries.size() && ok; i++) {
      NarrowSlot cur = entries[i];
      uint32_t avoid = 0xFFFFFFFFu;
      ok = false;
      for (int kick = 0; kick < 2000; kick++) {
        const uint32_t l = cur.key >> 16, r = cur.key & 0xFFFFu;
        const NarrowHash h = narrow_hash(l, r, sh);
        const uint32_t h1 = h.h1, h2 = h.h2;
        if (slots[h1].key == kNarrowEmptyKey) { slots[h1] = cur; ok = true; break; }
        if (slots[h2].key == kNarrowEmptyKey) { slots[h2] = cur; ok = true; break; }
        const uint32_t j = h1 == avoid ? h2 : h1;
        std::swap(cur, slots[j]);
        avoid = j;
      }
    }
    if (ok) break;
  }
  bits_out = bits;
  return true;
}

// The alphabet, the eligibility and the table of a merge list.  `packed`: the table's values are rank << 16 | (merged -
// SWT_SYM_BASE) (swt_bpe_table::packed); `live[i]`: merge i is the one the rank table holds for its pair (the last of a pair listed
// several times).  Eligible: packed, A + n_merges <= kNarrowMaxCodes, and every symbol the list names has a code below that too.
// An ineligible table is left empty.
inline void narrow_build(const uint32_t *left, const uint32_t *right, const uint32_t *merged, uint32_t n_merges, bool packed,
                         const std::vector<bool> &live, NarrowTable &t) {
  t = NarrowTable();
  if (!packed) return;
  uint32_t top = n_merges;  // symbols SWT_SYM_BASE + 0 .. top-1
  for (uint32_t i = 0; i < n_merges; i++) {
    if (merged[i] < kNarrowSymBase) { t = NarrowTable(); return; }  // (a packed table has none)
    for (uint32_t s : {left[i], right[i], merged[i]}) {
      if (s < kNarrowSymBase) t.cp_of_code.push_back(s);
      else top = std::max(top, s - kNarrowSymBase + 1u);
    }
  }
  std::sort(t.cp_of_code.begin(), t.cp_of_code.end());
  t.cp_of_code.erase(std::unique(t.cp_of_code.begin(), t.cp_of_code.end()), t.cp_of_code.end());
  if ((uint64_t)t.letters() + top > kNarrowMaxCodes) { t = NarrowTable(); return; }
  std::vector<NarrowSlot> entries;
  t.code_of_rank.assign(n_merges, kNarrowDead);
  t.sequential = true;
  for (uint32_t i = 0; i < n_merges; i++)
    if (live[i]) {
      const uint32_t g = t.code(merged[i]);
      entries.push_back(NarrowSlot{narrow_key(t.code(left[i]), t.code(right[i])), (i << 16) | g});
      t.code_of_rank[i] = g;
      if (g != t.letters() + i) t.sequential = false;
    }
  if (!narrow_place(entries, t.slots, t.bits)) { t = NarrowTable(); return; }
  t.eligible = true;
}

}  // namespace swt
