// swt_bpe_encode.hip -- FastBPE batched encode on gfx950.
//
// Replaces, for a whole batch of sentences at once:
//   SubwordTokenizer.preprocessing   /root/reference/source/utils.py:26-29   (split only; lower() is the caller's)
//   FastBPE.tokenize                 /root/reference/source/bpe.py:245-249
//   FastBPE.encode_word / _pairs     /root/reference/source/bpe.py:202-243
//   the rank dict                    /root/reference/source/bpe.py:200,257
//
// One kernel, bpe_lane_kernel: one 64-lane wavefront per tile (workgroup = one wave, so every barrier is a wave-local fence):
//   tile   = the sentences whose first byte lies in one window of the text (whole sentences, no data-path atomics between
//            workgroups, a tile's tokens are contiguous in the output)
//   chunk  = the part of the tile's span staged in LDS at a time; longer spans are cut at word boundaries
// The split stays byte-parallel and looks every adjacent pair up in the two-choice rank table (slot_value) on the way, then
// ONE LANE OWNS ONE WORD through the merge rounds (live-slot mask, a lane takes the next word when its own is finished, four
// lanes a word once few words are left); the phases are described where the kernel stands, below.
// A word longer than a chunk falls to a one-lane global-memory path (correct, slow, pathological inputs only).
//
// The ORDERED form of the same kernel (template parameter Ordered, entry points swt_bpe_encode_naive*) is NaiveBPE.encode_word,
// /root/reference/source/bpe.py:114-134: the merges applied in LIST order (bpe.py:126-127 over _replace_pair, bpe.py:25-48), which
// differs from FastBPE's lowest-rank-first on lists that repeat a pair or rank a pair below a merge producing one of its symbols.
// Only such lists take it (any trained list is order-equivalent and runs the FastBPE kernels as they are), so it is written for
// correctness, not speed: ONE LANE PER WORD through the literal rounds, no one-occurrence rounds, no four-lane tail.  On S85k-open
// it costs 0.418 ms per call against FastBPE's 0.153 (2.7 x), 2 % more than the FastBPE kernel on the same improper table, which
// takes the same rounds: DESIGN.md section 4.2d.
//
// The literal form of a merge round -- the best adjacent pair, its occurrences merged left to right, the word compacted -- is
// written twice, once per storage: literal_rounds() for a word in LDS with its cached pair values, walker_rounds() for one lane
// over global memory (a word longer than a chunk).  Both run under a MERGE RULE (RankRule, ListRule, DropRule, below), which says
// what FastBPE's rank order, NaiveBPE's list order and BPE-dropout do differently in a round.
#include <cstring>
#include <type_traits>
#include <unordered_map>
#include <utility>

#include "swt_bpe_narrow.h"
#include "swt_dedup.h"
#include "swt_philox.h"
#include "swt_tile.h"
#include "swt_words.h"

namespace swt {

struct alignas(16) BpeSlot {
  uint64_t key;     // left << 32 | right, kEmptyKey when free
  uint32_t rank;    // table value: rank, or rank << 16 | (merged - SWT_SYM_BASE) in a packed table
  uint32_t merged;  // symbol id of left+right
};

constexpr uint8_t kClsWs = 1, kClsPunct = 2;
constexpr uint32_t kNoRank = 0xFFFFFFFFu;
#ifndef SWT_LANE_TILE
#define SWT_LANE_TILE 384
#endif
// (the tail of the merge rounds, lane_tail: four lanes a word once 16 words are left in a chunk.  Measured on S85k-open, ms per call:
// no tail 0.187; 2 lanes a word from 32 words 0.184; 4 from 16: 0.176; 8 from 8: 0.180; 4 from 16 and then 8 from 8: 0.1775)
#ifndef SWT_LANE_CAP
#define SWT_LANE_CAP 512
#endif
constexpr int kLaneTile = SWT_LANE_TILE;  // the word-lane kernel (bpe_lane_kernel): bytes of sentence starts per tile ...
constexpr int kLaneCap = SWT_LANE_CAP;    // ... and staged bytes per chunk (a batch of 64 word lanes wants ~350 bytes of text)
// A wave of the running-text form takes a SPAN of K consecutive tiles (lane_span below) as one long tile, chunk by chunk.
constexpr uint32_t kLaneMaxSpan = 16;
// The tiles of the running-text form taper towards the end of the text (lane_map below, swt_tilemap.h): no tile is larger than
// kLaneTile, so LDS, registers and the chunk loop are those of the uniform geometry.
constexpr uint32_t kTaperSizes[4] = {(uint32_t)kLaneTile, 256u, 192u, 128u};
// The NARROW form of the running-text kernel (16-bit symbols in LDS, swt_bpe_narrow.h; LaneLds below) spends the LDS it saves on
// bytes: a larger chunk in the same LDS per wave, and a tile that keeps the 128 bytes of headroom kLaneTile has under kLaneCap.
constexpr int kNarrowCap = 640, kNarrowTile = kNarrowCap - (SWT_LANE_CAP - SWT_LANE_TILE);
constexpr uint32_t kNarrowTaperSizes[4] = {(uint32_t)kNarrowTile, 256u, 192u, 128u};
constexpr int kNarrowTaperDefault = 256 + 2;  // SWT_OPT_LANE_TAPER = 0 under the narrow sizes: c = 2/8, 192 bytes the smallest (profiles/lane_narrow.txt)
constexpr uint32_t kTaperMaxC8 = 64, kTaperMaxSlots = 1u << 20;  // the ranges of SWT_OPT_LANE_TAPER and SWT_OPT_LANE_SLOTS
constexpr int kTaperDefault = 256 + 3;  // what SWT_OPT_LANE_TAPER = 0 means: c = 3/8, 192 bytes the smallest (profiles/lane_taper.txt section 2)
constexpr uint64_t kDirectBytes = 1024, kDirectSents = 64;  // up to here one workgroup and one launch do the whole call

// The rank table is a two-choice cuckoo table (built once on the host, swt_bpe_table_create): a pair lives in slot h1 or in
// slot h2, so a lookup is two independent 16-byte loads and two compares -- no probe loop, and a wave never goes round
// again because one of its lanes met a collision.  The hashes are 24-bit multiplies (full-rate v_mul_u32_u24; symbol ids
// are below 2^24 for any table under five million merges, larger ids only hash worse) with one xor-shift between them.
// (BpeHash, kHash1, kHash2, bpe_hash: swt_bpe_narrow.h, beside narrow_hash, the hash pair of the table of 16-bit codes.)
static_assert(kNarrowSymBase == SWT_SYM_BASE, "swt_bpe_narrow.h numbers the merged symbols from SWT_SYM_BASE");
static_assert((kNarrowCont << 16) == SWT_BPE_CONT, "the emit moves the continuation bit of a code to that of an id");

__device__ __forceinline__ bool slot_lookup(const BpeSlot *__restrict__ slots, uint32_t sh, uint32_t l, uint32_t r,
                                            uint32_t &rank, uint32_t &merged) {
  const uint4 r1 = *reinterpret_cast<const uint4 *>(&slots[bpe_hash(l, r, sh, kHash1)]);
  const uint4 r2 = *reinterpret_cast<const uint4 *>(&slots[bpe_hash(l, r, sh, kHash2)]);
  const bool h1 = r1.x == r && r1.y == l, h2 = r2.x == r && r2.y == l;
  rank = h1 ? r1.z : r2.z;
  merged = h1 ? r1.w : r2.w;
  return h1 || h2;
}

__device__ __forceinline__ uint32_t slot_value(const BpeSlot *__restrict__ slots, uint32_t sh, uint32_t l, uint32_t r) {
  const uint4 r1 = *reinterpret_cast<const uint4 *>(&slots[bpe_hash(l, r, sh, kHash1)]);
  const uint4 r2 = *reinterpret_cast<const uint4 *>(&slots[bpe_hash(l, r, sh, kHash2)]);
  // both loads are issued before either is looked at; a pair lives in at most one slot and kNoRank is all ones, so the two
  // selects combine with AND (written as a select of a select the compiler makes the second load wait for the first compare)
  const uint32_t a = (r1.x == r && r1.y == l) ? r1.z : kNoRank;
  const uint32_t b = (r2.x == r && r2.y == l) ? r2.z : kNoRank;
  return a & b;
}
// Pointers the kernel reads out of a record in memory (NarrowDir) are generic to the compiler, and a load through one is a flat
// load: it counts against the LDS counter too and cannot take a scalar base.  They all point into device-global memory.
template <class T>
using GlobalPtr = const __attribute__((address_space(1))) T *;
template <class T>
__device__ __forceinline__ GlobalPtr<T> global_ptr(const T *p) { return (GlobalPtr<T>)p; }
// The same over the table of 16-bit codes (swt_bpe_narrow.h): two 8-byte loads, one compare each.  l and r without kNarrowCont.
// Both slots come from one multiply chain (narrow_hash), and a slot's address is the table's base -- a scalar -- and a 32-bit
// byte offset (a table has at most 2^28 slots), so no 64-bit add is made per slot.
__device__ __forceinline__ uint32_t slot_value(const NarrowSlot *__restrict__ slots, uint32_t sh, uint32_t l, uint32_t r) {
  const NarrowHash h = narrow_hash(l, r, sh);
  const GlobalPtr<char> base = global_ptr(reinterpret_cast<const char *>(slots));
  typedef uint32_t Pair __attribute__((ext_vector_type(2)));  // {key, value}: one 8-byte load
  const Pair r1 = *reinterpret_cast<GlobalPtr<Pair>>(base + (h.h1 << 3));
  const Pair r2 = *reinterpret_cast<GlobalPtr<Pair>>(base + (h.h2 << 3));
  const uint32_t key = narrow_key(l, r);
  const uint32_t a = r1.x == key ? r1.y : kNoRank;
  const uint32_t b = r2.x == key ? r2.y : kNoRank;
  return a & b;
}
// What the narrow kernel reads beside its rank table, one record per handle in device memory (the kernel's merged_of_rank
// argument, which a packed table does not use, points at it).
struct NarrowDir {
  const BpeSlot *wide_slots;   // the table of the ids, for the one-lane walker of a word longer than a chunk
  const uint32_t *code_of_cp;  // [n_cps] code | class << 16 (NarrowTable::code_of_cp)
  const uint32_t *cp_of_code;  // [letters] the alphabet, for the emit
  const uint32_t *code_of_rank;  // null for a sequential table (NarrowTable::sequential), whose kernel (Seq) does not read it; else [n_merges] the merged code of a rank
  uint32_t wide_sh, n_cps, letters, pad;
};
// Narrow: an entry of val[] is the round's KEY, rank << 16 | the slot's index in its word, so the minimum of a word is a plain
// minimum over what a scan reads.  `v`: a table value (rank << 16 | code), or kNoRank -- which stays "no pair" (>= kNarrowNoPair)
// under any slot.  Dead slots hold kNoRank, a FOREIGN symbol's entry kNarrowNoPair | code point: neither wins a minimum.
__device__ __forceinline__ uint32_t slot_key(uint32_t v, uint32_t slot) { return (v & 0xFFFF0000u) | slot; }
// the code of the symbol that the merge of rank `rank` produces.  Seq: the table is sequential (NarrowTable::sequential) and the
// kernel keeps no pointer for it; a branch on the pointer in one kernel cost the sequential tables 0.75 M vector instructions a
// launch and 1.6 % of the step in registers spilled around the rounds (profiles/lane_keys.txt section 6)
template <bool Seq>
__device__ __forceinline__ uint32_t narrow_merged(const NarrowDir &D, uint32_t rank) {
  if constexpr (Seq) return D.letters + rank; else return global_ptr(D.code_of_rank)[rank];
}

// ---- The MERGE RULES.  The literal form of a round (literal_rounds, walker_rounds) is one loop; a rule answers what the three
// orders do differently in it:
//   value(v)    the table value of a pair -> the value a round compares (kNoRank: the pair does not merge);
//   takes(k)    whether the pair at slot k of the round's sequence takes part in this round.  Asked only of a pair that beats the
//               minimum so far, and in the merge of an occurrence of the winning pair;
//   next(rank)  the round that merged the pair of `rank` is over: what the next round starts from;
//   begin()     a round begins: what takes() keeps within a round starts empty (a draw does not outlive its round; kept across
//               rounds in the rule, the four draws and their group cost the dropout form 1.5 % of its time);
//   lookup()    the walker's probe of a pair: its value(), and the merged symbol where the slot holds the round's.
// kChain: a value may stand for a later list position than the table's, so the merged symbol is the position's (info[2 * rank]).
// A rule is the rule of ONE word.  What travels from the kernel to the word routines makes it: of(L, where) for the word whose
// first symbol is symbol `where` of the chunk in L, of(s, pos) for the word at byte `pos` of the text, in sentence s.

template <bool Packed>
__device__ __forceinline__ uint32_t value_rank(uint32_t v) { return Packed ? (v >> 16) : v; }  // the rank (list position) half of a table value

// FastBPE's rank order (bpe.py:210-238): lowest rank first.  Every answer is a constant: its rounds test nothing and draw nothing.
struct RankRule {
  static constexpr bool kChain = false;
  __device__ __forceinline__ uint32_t value(uint32_t v) const { return v; }
  __device__ __forceinline__ void begin() {}
  __device__ __forceinline__ bool takes(uint32_t) const { return true; }
  __device__ __forceinline__ void next(uint32_t) {}
  // the walker's probe of a pair: its value and, from the slot, its merged symbol; false when the pair does not merge
  __device__ __forceinline__ bool lookup(const BpeSlot *__restrict__ slots, uint32_t sh, uint32_t l, uint32_t r, uint32_t &v, uint32_t &mg) const {
    return slot_lookup(slots, sh, l, r, v, mg);
  }
  template <class Lds>
  __device__ __forceinline__ RankRule of(const Lds &, uint32_t) const { return *this; }  // every word's rule: in a chunk,
  __device__ __forceinline__ RankRule of(uint64_t, uint64_t) const { return *this; }     // and at a byte of the text
};

// NaiveBPE's list order (bpe.py:126-127) as a RISING FLOOR: a round takes the smallest list position >= floor over the word's
// adjacent pairs, merges all occurrences of that pair left to right (bpe.py:25-48) and sets floor = position + 1.  That is the
// literal loop: the merges below the floor have been applied or found nothing to apply to, and no position between the floor and
// the minimum has an occurrence in the word.  A pair listed several times has several positions; the ordered table
// (swt_bpe_table::h_oslots) holds the FIRST, and info[2 * i + 1] chains position i to the next position of the same pair (kNoRank
// at the end); info[2 * i] is the merged symbol of position i.
template <bool Packed>
struct ListRule {
  static constexpr bool kChain = true;
  const uint32_t *__restrict__ info;
  uint32_t floor = 0;
  // the value of the pair's first position >= floor, kNoRank when there is none
  __device__ __forceinline__ uint32_t value(uint32_t v) const {
    if (v == kNoRank) return v;
    uint32_t r = value_rank<Packed>(v);
    if (r >= floor) return v;
    do r = info[2 * r + 1]; while (r < floor);  // (the end of the chain, kNoRank, is below no floor)
    if (r == kNoRank) return kNoRank;
    return Packed ? ((r << 16) | (info[2 * r] - SWT_SYM_BASE)) : r;
  }
  __device__ __forceinline__ void begin() {}
  __device__ __forceinline__ bool takes(uint32_t) const { return true; }
  __device__ __forceinline__ void next(uint32_t rank) { floor = rank + 1u; }
  // (the merged symbol is the winning position's, which the walker reads from info once the round's pair is known)
  __device__ __forceinline__ bool lookup(const BpeSlot *__restrict__ slots, uint32_t sh, uint32_t l, uint32_t r, uint32_t &v, uint32_t &mg) const {
    v = value(slot_value(slots, sh, l, r));
    mg = 0;
    return true;
  }
  template <class Lds>
  __device__ __forceinline__ ListRule of(const Lds &, uint32_t) const { return *this; }  // every word's rule, the floor at 0
  __device__ __forceinline__ ListRule of(uint64_t, uint64_t) const { return *this; }
};

// BPE-dropout (include/swt.h, swt_bpe_encode_dropout): FastBPE's order with every candidate pair of a round skipped when its
// draw says so.  The draw of pair k in round t of the word with the key (i, b) -- its sentence and its first byte's offset in
// it -- is word k & 3 of Philox at the counter ((t << 16) + (k >> 2), b, i, epoch): one call serves four neighbours.  A pair
// that does not beat the minimum so far cannot change it, so the loops do not ask for its draw: which calls are made is theirs.
struct DropDraw {  // what a dropout launch draws with: kernel arguments of the dropout kernels, and of no other
  unsigned long long drop_below;  // 0 .. 2^32
  uint32_t key0, key1, epoch;
};
struct DropWord { uint32_t i, b; };
struct DropRule {
  static constexpr bool kChain = false;
  const DropDraw &dd;
  const DropWord w;
  uint32_t t = 0, t16 = 0;       // the rounds begun, and the round at hand << 16
  uint32_t group = 0xFFFFFFFFu;  // k >> 2 of the call `x` holds (a word has fewer than 2^32 symbols: no group is all ones)
  Philox x{};                    // the draws are asked for in any order of k; the last call's four words are kept
  __device__ __forceinline__ DropRule(const DropDraw &d, const DropWord &word) : dd(d), w(word) {}
  __device__ __forceinline__ uint32_t value(uint32_t v) const { return v; }
  __device__ __forceinline__ bool takes(uint32_t k) {
    if ((k >> 2) != group) {
      group = k >> 2;
      x = philox4x32_10(t16 + group, w.b, w.i, dd.epoch, dd.key0, dd.key1);
    }
    const uint32_t q = k & 3u;
    const uint32_t v = q == 0u ? x.x[0] : q == 1u ? x.x[1] : q == 2u ? x.x[2] : x.x[3];
    return v >= dd.drop_below;
  }
  __device__ __forceinline__ void begin() { t16 = t++ << 16; group = 0xFFFFFFFFu; x = Philox{}; }  // (no draw outlives its round)
  __device__ __forceinline__ void next(uint32_t) {}  // (begin() counts the rounds)
  // the walker's probe of a pair: its value and, from the slot, its merged symbol; false when the pair does not merge
  __device__ __forceinline__ bool lookup(const BpeSlot *__restrict__ slots, uint32_t sh, uint32_t l, uint32_t r, uint32_t &v, uint32_t &mg) const {
    return slot_lookup(slots, sh, l, r, v, mg);
  }
};

// The literal rounds on a symbol array in global memory, the one-lane fallback for a word longer than a chunk (bpe.py:210-238
// under RankRule, bpe.py:124-127 under ListRule): repeat { the best adjacent pair; replace all of its occurrences left to right,
// non-overlapping }.  Returns the new length.
template <bool Packed, class Rule>
__device__ uint32_t walker_rounds(uint32_t *s, uint32_t n, const BpeSlot *__restrict__ slots, uint32_t sh, Rule rule) {
  while (n >= 2) {
    rule.begin();
    uint32_t best = kNoRank, bm = 0, bl = 0, br = 0;
    uint32_t a = s[0];
    for (uint32_t k = 0; k + 1 < n; k++) {
      const uint32_t b = s[k + 1];
      uint32_t v, mg;
      if (rule.lookup(slots, sh, a, b, v, mg) && v < best && rule.takes(k)) { best = v; bm = mg; bl = a; br = b; }
      a = b;
    }
    if (best == kNoRank) break;
    if constexpr (Rule::kChain) bm = rule.info[2 * value_rank<Packed>(best)];
    uint32_t j = 0, i = 0;  // i counts in the round's sequence, which is what takes() goes by; j <= i
    while (i < n) {
      const uint32_t x = s[i];
      if (i + 1 < n && x == bl && s[i + 1] == br && rule.takes(i)) { s[j++] = bm; i += 2; }
      else { s[j++] = x; i++; }
    }
    n = j;
    rule.next(value_rank<Packed>(best));
  }
  return n;
}

struct GiantResult { uint64_t end; uint32_t ntok; };

// One lane, global memory only: the word (or single separator) starting at byte `pos`, bounded by
// `send` (end of its sentence).  Tokens go to `out` (which doubles as the symbol workspace).
// `rule`: the word's merge rule (walker_rounds).
template <bool Packed, class Rule>
__device__ GiantResult giant_word(const uint8_t *__restrict__ text, uint64_t pos, uint64_t send,
                                  const uint8_t *__restrict__ cls_tab, const BpeSlot *__restrict__ slots, uint32_t sh, uint32_t *out,
                                  const Rule &rule) {
  GiantResult r{pos, 0};
  uint32_t n = 0;
  bool first = true;
  while (r.end < send) {
    const uint8_t b = text[r.end];
    int len = utf8_len(b);
    if (r.end + len > send) len = (int)(send - r.end);
    uint32_t cp = b;
    if (b >= 0x80 && len > 1) {
      cp = b & (0xFF >> (len + 1));
      for (int i = 1; i < len; i++) cp = (cp << 6) | (text[r.end + i] & 0x3F);
    }
    const uint8_t c = utf8_is_cont(b) ? kClsWs : ((cls_tab && cp < kNumCodePoints) ? cls_tab[cp] : (uint8_t)0);
    if (c & kClsWs) { if (first) r.end += len; break; }
    if (c & kClsPunct) { if (first) { out[n++] = cp; r.end += len; } break; }
    out[n++] = cp;
    r.end += len;
    first = false;
  }
  n = walker_rounds<Packed>(out, n, slots, sh, rule);
  for (uint32_t i = 1; i < n; i++) out[i] |= SWT_BPE_CONT;
  r.ntok = n;
  return r;
}

// ======================================================================================================================
// bpe_lane_kernel, phase by phase (one chunk of a tile at a time):
//   A    stage the chunk's bytes in LDS (one dwordx4 per lane) and mark the sentence starts in it
//   B/C  64 bytes per step: decode the code point at each UTF-8 lead byte, class from a two-bit LDS copy of the table, then
//        everything structural (word starts, symbols, the cut for a span longer than the chunk) comes from 64-bit ballot
//        masks.  The symbols are left DENSE (indexed by symbol, not by byte) together with the table value of every adjacent
//        pair (probed right there, all lanes at once).
//   W    the multi-symbol words of the chunk, longest class first (9+, 5-8, 2-4 symbols)
//   D    lane = word.  The word's slots stay where the split put them; a 32-bit mask says which are still live.  A round =
//        leftmost minimum over the live slots' cached pair values (four slots per step) -> the pair merges in place, its
//        right slot dies, and the two pairs next to the merged symbol are probed again (four loads in flight).  A lane whose
//        word is finished takes the next word of the list.  On a PROPER table (every pair ranks above the merges that produce
//        its symbols: any trained table) merging one occurrence per round is the reference's "all occurrences of the best
//        pair, left to right" (bpe.py:221-235) -- what is left of the pair is still the minimum and is found leftmost-first
//        in the next round.  Tables without that property, and words beyond 32 symbols, take literal_rounds(): the same loop
//        in its literal form (all occurrences per round, compaction), one lane per word, under the kernel's merge rule.
//   E/F  order-preserving ballot compaction over the SYMBOL space to the tile's output run; the tile-local token offset of
//        every sentence, through the split's symbol masks.
// Template parameters:
//   Packed = true: the table value of a pair is rank << 16 | (merged - SWT_SYM_BASE), so a merge round learns the merged
//            symbol without touching memory (tables below 65,534 merges); false: the value is the rank and the merged symbol
//            is read from merged_of_rank[].
//   Proper: the table is proper (above), so the one-occurrence rounds of D apply.
//   Mode:  0 = tiles of running text (plan, sent_local / tile_tok for the scan + gather), 1 = the unique-word pass of the
//          dedup path (every "sentence" is a unique word: its token run -- place in scratch and length -- goes straight to
//          drec[s], and length | s to the word's table slot, rec[uslot[s]]; nobody needs a scan or a gather of that launch's
//          output), 2 = one workgroup writing the caller's arrays (DirectOut).  A template parameter, not a run-time test:
//          each form keeps only its own arguments in scalar registers (one kernel for all three spilled 44 of them).
//   Ordered: NaiveBPE's list order (bpe.py:126-127) instead of lowest rank first: `slots` is the table of FIRST list positions,
//          `merged_of_rank` the interleaved (merged symbol, next position of the same pair) array, and every multi-symbol word
//          goes through the literal rounds under a ListRule, one lane per word.  Launched only for a table that is not
//          order-equivalent (swt_bpe_table::order_equivalent), where the two orders can disagree.
// Measured and dropped (profiles/r03_experiments/bpe_lane_*.txt): one wave running the rounds for the words of four tiles
// (fewer instructions, but three waves of four idle meanwhile: 0.229 against 0.200 ms), tiles that place their own output by a
// decoupled look-back, and tiles that plan themselves (two launches instead of four).
//   Narrow: the symbols in LDS are the 16-bit codes of swt_bpe_narrow.h and `slots` is the table keyed on them (NarrowSlot, with
//          merged_of_rank pointing at a NarrowDir).  9 bytes of LDS per staged byte instead of 11, so kNarrowCap = 640 bytes fit
//          where kLaneCap = 512 did, a wave pools a quarter more words for the same rounds, and the same number of waves reside.
//          The split reads a code point's code AND its class from one table (code_of_cp), so the two-bit class copy in LDS and the
//          1 KB every wave loads for it are gone.  A code point outside the alphabet is FOREIGN: it never merges, and its val[]
//          entry -- which no lookup can fill -- carries the code point to the emit.  Running text (Mode 0) on a packed table
//          below 32 k symbols only; Ordered, Modes 1 and 2 and every other table keep the wide kernel as it was.
//          The val[] entry of a pair is the round's KEY, rank << 16 | the slot's index in its word (slot_key): the split writes
//          it with the slot counted across its blocks, a round writes its two entries with theirs, and the three scans (scan_keys,
//          lane_tail) are plain minima, 6 vector instructions and 2 ds_read2_b32 per four slots where building the keys from the
//          values took 15 and 4 (profiles/lane_keys.txt).  The merged code comes from the key's rank (narrow_merged): letters + rank
//          in the kernel of a sequential table (template parameter Seq), code_of_rank[rank] in that of any other.
//   Dropout: BPE-dropout (swt_bpe_encode_dropout*, include/swt.h): every multi-symbol word goes through the literal rounds
//          under a DropRule, one lane per word, with the candidate pairs of every round dropped by their Philox draws.  Wide
//          symbols, Modes 0 and 2 (two occurrences of a word may differ: no unique-word pass).  The draws are arguments of these
//          instantiations alone (DirectDrop).  DESIGN.md section 4.2e.
// Ordered and Dropout stop at the kernel: it makes one thing of them (lane_rules) -- a RankRule, a ListRule, or the DropSite that
// makes every word its DropRule -- and that is what lane_chunk_end, giant_word and lane_rounds take.  A RankRule is empty and its
// answers are constants, so the kernels of FastBPE's order carry nothing for the other two and test nothing.
template <bool Narrow>
struct LaneSym {  // how a symbol stands in LDS
  using type = uint32_t;
  using Slot = BpeSlot;
  static constexpr uint32_t kCont = SWT_BPE_CONT, kDead = kInvalidTok;
};
template <>
struct LaneSym<true> {
  using type = uint16_t;
  using Slot = NarrowSlot;
  static constexpr uint32_t kCont = kNarrowCont, kDead = kNarrowDead;
};
template <int Cap, bool NarrowSyms = false>
struct LaneLds {
  static constexpr int Blocks = Cap / 64;
  static constexpr bool Narrow = NarrowSyms;
  using Sym = typename LaneSym<Narrow>::type;
  __attribute__((aligned(16))) uint8_t txt[Cap + 16];  // staged bytes; once the split is done, a single-wave kernel's word list
  Sym sym[Cap + 4];           // per symbol: id (| SWT_BPE_CONT unless it opens its word), kInvalidTok once consumed; Narrow: its code
  uint32_t val[Cap + 4];      // per symbol: table value of (this symbol, next live symbol of the word), kNoRank when none; Narrow: its key (slot_key)
  uint16_t wl[Cap + 2];       // first symbol of every word, in text order
  unsigned long long sbits[Blocks + 1];    // sentence-start bit per byte
  unsigned long long symmask[Blocks + 1];  // symbol bit per byte
  unsigned long long vmask[Blocks + 1];    // phase E: live-token bit per symbol
  uint32_t sympre[Blocks + 1];             // symbols before each 64-byte block
  uint32_t blkpre[Blocks + 1];             // tokens before each block of 64 symbols
};
// what outlives a chunk: kept out of LaneLds so that a chunk's arrays stay one block
template <bool Narrow>
struct LaneShared {
  uint32_t cls2[64];                       // classes of U+0000..U+03FF, two bits each
  GiantResult giant;
};
template <>
struct LaneShared<true> {                  // the narrow split reads the class beside the code (NarrowDir::code_of_cp)
  static constexpr uint32_t *cls2 = nullptr;
  GiantResult giant;
};

// What a wave carries from chunk to chunk of its tile, and what it knows about the chunk at hand.
struct LaneTile {
  uint64_t s_lo, s_hi;           // the tile's sentences
  uint64_t span_base, span_end;  // their bytes
  uint64_t s_next;               // first sentence whose local offset is not recorded yet
  uint64_t cb;                   // first byte not encoded yet
  uint32_t *tile_out;            // the tile's run in scratch
  uint32_t run;                  // tokens emitted so far
};
struct LaneChunk {
  uint64_t abase;                // 16-byte aligned base of the staged bytes
  uint32_t off0, staged, nblk;   // first byte of the chunk inside the staged bytes, staged bytes, 64-byte blocks
  uint32_t ce;                   // end of the chunk (the cut, or staged)
  uint32_t nsym, nw;             // symbols and words of the chunk
  int cut;                       // last word boundary (for a span longer than the chunk), -1 when none
  bool last, giant;              // the tile ends with this chunk; the chunk was one word longer than the staged bytes
};

// LDS traffic between the lanes of ONE wave needs no hardware barrier (a wave's LDS instructions execute in order); the
// compiler must not move accesses across the point, that is all.
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Lane masks without a detour through a vector register.  lane_ballot: the mask of a predicate straight from the compare that
// makes it (__ballot turns the bool into an int and compares that again: a v_cndmask and a v_cmp_ne per mask).  lane_bit: this
// lane's bit of a mask that is the same in every lane, as a predicate (the mask itself serves as the condition; (m >> lane) & 1
// is two 64-bit vector operations and a compare).  lanes_below: base + the set bits of such a mask below this lane (v_mbcnt).
__device__ __forceinline__ unsigned long long lane_ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }
__device__ __forceinline__ bool lane_bit(unsigned long long uniform_mask) { return __builtin_amdgcn_inverse_ballot_w64(uniform_mask); }
__device__ __forceinline__ uint32_t lanes_below(unsigned long long uniform_mask, uint32_t base) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(uniform_mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)uniform_mask, base));
}

constexpr uint32_t kDirtyVal = 0xFFFFFFFEu;  // above every table value (ranks stay below 2^32 - 2), below kNoRank

// The literal rounds (bpe.py:210-238 under RankRule, bpe.py:124-127 under ListRule) on one word whose symbols S[0..n) and pair
// values V[0..n) (V[n-1] = kNoRank) live in LDS: every round merges ALL occurrences of the best pair left to right, compacts the
// word and probes only the pairs that changed.  A cached value outlives the round under every rule: it stays the pair's rank
// whatever was dropped around it (DropRule), and one above the round's minimum is a position >= the new floor, so it stays the
// pair's first such position (ListRule; the values the split left come from the table of first positions and are valid at
// floor 0).  All slots of the winning pair hold the same value, so V[i] == m finds them.  The compaction reads slot i -- the index
// takes() goes by -- and writes slot j <= i.
// Narrow: S holds 16-bit codes.  A FOREIGN symbol's V entry is its code point (>= kNarrowNoPair, so it is never the minimum); it
// moves with the symbol when the word is compacted and is neither marked dirty nor reset.  The pair entries come in as keys
// (slot_key) and are read by their RANK half alone: the word is finished here, so the low half -- the split's slot, stale once the
// word is compacted, or the code of a value looked up here -- is never read as a slot.
template <bool Packed, bool Narrow = false, bool Seq = false, class Rule>
__device__ void literal_rounds(typename LaneSym<Narrow>::type *S, uint32_t *V, const uint32_t n0, const typename LaneSym<Narrow>::Slot *__restrict__ slots,
                               uint32_t sh, const uint32_t *__restrict__ merged_of_rank, const NarrowDir &D, Rule rule) {
  constexpr uint32_t kCont = LaneSym<Narrow>::kCont, kDead = LaneSym<Narrow>::kDead;
  uint32_t n = n0;
  for (;;) {
    rule.begin();
    uint32_t m = kNoRank;
    for (uint32_t k = 0; k + 1 < n; k++) {
      const uint32_t v = V[k];
      if (m > v && rule.takes(k)) m = v;  // (a pair that does not beat the minimum so far cannot change it: it is not asked about)
    }
    if (Narrow ? m >= kNarrowNoPair : m == kNoRank) break;
    const uint32_t rank = Packed ? (m >> 16) : m;
    uint32_t mg;
    if constexpr (Narrow) mg = narrow_merged<Seq>(D, rank);
    else mg = Packed ? (SWT_SYM_BASE + (m & 0xFFFFu)) : merged_of_rank[Rule::kChain ? 2 * rank : rank];
    uint32_t i = 0, j = 0;
    while (i < n) {
      const uint32_t vi = V[i];
      // (Narrow: no other kind of entry has a rank's high half)
      const bool take = i + 1 < n && (Narrow ? (vi >> 16) == (m >> 16) : vi == m) && rule.takes(i);
      const uint32_t s = take ? mg : (S[i] & ~kCont);
      if (take && j && !(Narrow && (S[j - 1] & ~kCont) == kNarrowForeign)) V[j - 1] = kDirtyVal;
      S[j] = j ? (s | kCont) : s;
      V[j] = take ? kDirtyVal : vi;
      i += take ? 2u : 1u;
      j++;
    }
    n = j;
    rule.next(rank);
    if (!(Narrow && (S[n - 1] & ~kCont) == kNarrowForeign)) V[n - 1] = kNoRank;
    for (uint32_t k = 0; k + 1 < n; k++)
      if (V[k] == kDirtyVal) V[k] = rule.value(slot_value(slots, sh, S[k] & ~kCont, S[k + 1] & ~kCont));
  }
  for (uint32_t k = n; k < n0; k++) S[k] = kDead;
}

// classes of the first 1,024 code points: 16 per lane, two bits each (SWT_CLS_BERT_WS | SWT_CLS_BERT_PUNCT)
__device__ __forceinline__ void lane_classes(LaneShared<false> &L, const uint8_t *__restrict__ cls_tab, int lane) {
  uint32_t w = 0;
  if (cls_tab) {
    const uint4 v = reinterpret_cast<const uint4 *>(cls_tab)[lane];
    auto pk = [](uint32_t d) {
      uint32_t x = d & 0x03030303u;
      x = (x | (x >> 6)) & 0x000F000Fu;
      return (x | (x >> 12)) & 0xFFu;
    };
    w = pk(v.x) | (pk(v.y) << 8) | (pk(v.z) << 16) | (pk(v.w) << 24);
  }
  L.cls2[lane] = w;
}

// ---- A + B/C of one chunk: stage the bytes, then 64 bytes per step: classes, word structure from ballot masks, the dense
// symbols, the list of word starts, and the table value of every adjacent pair of a word.
// Narrow: the symbols are codes, read with the class from D.code_of_cp (cls2 is not there); a FOREIGN symbol's val[] entry gets
// its code point.
template <int Cap, bool Narrow>
__device__ __forceinline__ void lane_split(LaneLds<Cap, Narrow> &L, const uint32_t *cls2, const NarrowDir &D, const uint8_t *__restrict__ text,
                                           uint64_t n_bytes, const uint64_t *__restrict__ sent_off, const uint8_t *__restrict__ cls_tab,
                                           const typename LaneSym<Narrow>::Slot *__restrict__ slots, uint32_t sh, const LaneTile &T, LaneChunk &C,
                                           int lane) {
  constexpr int Blocks = Cap / 64;
  constexpr uint32_t kCont = LaneSym<Narrow>::kCont;
  const unsigned long long le = (2ull << lane) - 1ull;  // me and below
  const uint64_t abase = T.cb & ~15ull;
  const uint32_t off0 = (uint32_t)(T.cb - abase);
  const uint64_t avail = T.span_end - abase;
  const bool last = avail <= (uint64_t)Cap;
  const uint32_t staged = last ? (uint32_t)avail : (uint32_t)Cap;
  const uint32_t nblk = (staged + 63) >> 6;

  // ---- A. stage [abase, abase+staged): one dwordx4 per lane
  for (uint32_t c = lane * 16; c < staged; c += 64 * 16) {
    const uint64_t g = abase + c;
    if (g + 16 <= n_bytes && ((reinterpret_cast<uintptr_t>(text + g) & 15) == 0)) {
      *reinterpret_cast<uint4 *>(&L.txt[c]) = *reinterpret_cast<const uint4 *>(text + g);
    } else {
      for (int i = 0; i < 16; i++) L.txt[c + i] = (g + i < n_bytes) ? text[g + i] : (uint8_t)' ';
    }
  }
  if (lane <= Blocks) L.sbits[lane] = 0ull;
  wave_sync();
  for (uint64_t s = T.s_next + lane; s < T.s_hi; s += 64) {
    const uint64_t o = sent_off[s];
    if (o >= abase + staged) break;
    if (o >= T.cb) atomicOr(&L.sbits[(o - abase) >> 6], 1ull << ((o - abase) & 63));
  }
  wave_sync();

  // ---- B/C.  Scalars carried from block to block (the two flags as integers: a bool that lives across the loop is kept as a
  // lane mask, and every use of it in scalar logic went through a v_cndmask and a v_readfirstlane):
  uint32_t nsym = 0, nw = 0;  // symbols and words so far
  unsigned long long prev_wb = 1ull;  // 1: the byte before this block belongs to a whitespace/punctuation char (or chunk start)
  uint32_t pend_shut = 1u;    // 0: the last symbol of the previous block may have its successor in this one
  uint32_t pend_cp = 0;
  int cut = -1;               // last word boundary (for a span longer than the chunk)
  // Every mask of a block comes from ONE vector compare, taken where the compare stands (lane_ballot; a predicate that first
  // crosses a branch is made into a register and compared again), and is combined with the others as a scalar.  With
  // d = p - off0: off0 <= p < staged is d < n_in (off0 < staged), and off0 < p && p + 4 <= staged is d - 1 < n_cut.
  const uint32_t n_in = staged - off0, n_cut = max(n_in, 4u) - 4u;
  // The class of a lane is tested where it lies: Narrow, bits 16 and 17 of the code_of_cp entry; a lane outside the chunk, which
  // behaves as whitespace, holds kClsOut there.  The masks are scalars (no class table: nothing in the chunk has a class).
  constexpr uint32_t kClsAt = Narrow ? 16u : 0u, kClsOut = 4u << kClsAt;
  const uint32_t ws_bits = Narrow ? ((cls_tab ? kClsWs << kClsAt : 0u) | kClsOut) : kClsWs;
  const uint32_t pn_bits = Narrow ? (cls_tab ? kClsPunct << kClsAt : 0u) : kClsPunct;
  for (uint32_t blk = 0; blk < nblk; blk++) {
    const uint32_t p = blk * 64 + lane;
    const uint32_t d = p - off0;
    const bool inr = d < n_in;
    const unsigned long long INR = lane_ballot(inr);
    const unsigned long long CUTR = lane_ballot(d - 1u < n_cut);
    const uint8_t b = inr ? L.txt[p] : (uint8_t)' ';
    const bool lead = !utf8_is_cont(b);
    const unsigned long long LEAD = lane_ballot(lead);
    uint32_t cp = b;
    if (b >= 0xC0) {
      int len = utf8_len(b);
      if (p + len > staged) len = (int)(staged - p);
      if (len > 1) {
        cp = b & (0xFF >> (len + 1));
        for (int i = 1; i < len; i++) cp = (cp << 6) | (L.txt[p + i] & 0x3F);
      }
    }
    uint32_t c = Narrow ? kClsOut : kClsWs;  // bytes outside the chunk behave as whitespace
    uint32_t sy = cp;     // the symbol: the code point, or (Narrow) its code
    if constexpr (Narrow) {
      sy = kNarrowForeign;
      if (inr && lead) {
        if (cp < D.n_cps) {
          c = global_ptr(D.code_of_cp)[cp];  // (the code below the class: no test reads it)
          sy = c & 0xFFFFu;
        } else {
          c = (cls_tab && cp < kNumCodePoints) ? (uint32_t)(cls_tab[cp] & 3u) << kClsAt : 0u;
          // an ill-formed sequence that decodes past U+10FFFF reads as the symbol id it equals, as it does in the wide kernel
          if (cp >= SWT_SYM_BASE && cp - SWT_SYM_BASE + D.letters < kNarrowMaxCodes) sy = cp - SWT_SYM_BASE + D.letters;
        }
      }
    } else if (inr && lead)
      c = cp < 1024u ? ((cls2[cp >> 4] >> ((cp & 15u) << 1)) & 3u) : ((cls_tab && cp < kNumCodePoints) ? (cls_tab[cp] & 3u) : 0u);
    const unsigned long long WSm = lane_ballot((c & ws_bits) != 0u) & LEAD;
    const unsigned long long PNm = lane_ballot((c & pn_bits) != 0u) & LEAD;
    const unsigned long long CONT = ~LEAD;
    unsigned long long WB = WSm | PNm | (prev_wb & CONT);  // (prev_wb is bit 0 alone)
    WB |= (WB << 1) & CONT;
    WB |= (WB << 1) & CONT;
    WB |= (WB << 1) & CONT;
    const unsigned long long SS = L.sbits[blk];
    const unsigned long long first_bit = blk == 0 ? (1ull << off0) : 0ull;  // off0 < 16
    const unsigned long long before = (WB << 1) | prev_wb | SS | first_bit;
    const unsigned long long SYM = LEAD & ~WSm & INR;
    const unsigned long long WSTART = SYM & (PNm | before);
    {
      const unsigned long long CUT = LEAD & (WSm | PNm | SS) & CUTR;
      if (CUT) cut = (int)(blk * 64 + 63 - __builtin_clzll(CUT));
    }
    const bool is_sym = lane_bit(SYM);
    const bool wstart = lane_bit(WSTART);
    const unsigned long long after = SYM & ~le;
    const uint32_t q = after ? (uint32_t)__builtin_ctzll(after) : 64u;
    // HASNEXT: the symbols whose next symbol in the block continues their word, as a scalar.  In bit-reversed order the next
    // symbol of a lane lies BELOW it: a one added above every continuing symbol to the mask of the non-symbol lanes carries up
    // through them and sets exactly the symbol it belongs to (a symbol lane is a zero there and takes at most that one carry).
    const unsigned long long rsym = __builtin_bitreverse64(SYM);
    const unsigned long long HASNEXT = __builtin_bitreverse64((~rsym + (__builtin_bitreverse64(SYM & ~WSTART) << 1)) & rsym);
    const bool hasnext = lane_bit(HASNEXT);
    const uint32_t f = SYM ? (uint32_t)__builtin_ctzll(SYM) : 64u;
    const bool joins = pend_shut == 0u && f < 64 && !((WSTART >> (f & 63)) & 1ull);
    const uint32_t si = lanes_below(SYM, nsym);
    const uint32_t cpn = __shfl(sy, (int)(q & 63));
    // lane 63 never has a successor inside the block: it probes the pair that straddles the block boundary (Narrow: not behind a
    // FOREIGN symbol, whose entry is taken)
    const unsigned long long JP = (joins && !(Narrow && pend_cp == kNarrowForeign)) ? 1ull << 63 : 0ull;
    const bool jp = lane_bit(JP);
    const uint32_t cpf = __builtin_amdgcn_readlane(sy, (int)(f & 63));
    const bool want = lane_bit(HASNEXT | JP);
    if (wstart) L.wl[lanes_below(WSTART, nw)] = (uint16_t)si;
    uint32_t v = kNoRank;
    if constexpr (Narrow) {
      // the value goes in as the key of its slot (slot_key): the symbol's place in its word, counted from the word's first
      // symbol, which the word list holds by now -- this block's word starts were written just above, and a lane's word is
      // the last that starts at or below it (the straddling pair's: the last of the blocks before).  A symbol that has a
      // successor has a word: the first symbol of a chunk starts one.
      wave_sync();
      if (want) {
        const uint32_t first = L.wl[jp ? nw - 1u : lanes_below(WSTART >> 1, nw - 1u + (uint32_t)(WSTART & 1ull))];
        v = slot_key(slot_value(slots, sh, jp ? pend_cp : sy, jp ? cpf : cpn), (jp ? nsym - 1u : si) - first);
      }
    } else if (want) {
      v = slot_value(slots, sh, jp ? pend_cp : sy, jp ? cpf : cpn);
    }
    if (is_sym) {
      L.sym[si] = wstart ? sy : (sy | kCont);
      if (!hasnext) L.val[si] = kNoRank;
    }
    if (want) L.val[jp ? nsym - 1 : si] = v;
    if constexpr (Narrow) {
      if (is_sym && sy == kNarrowForeign) L.val[si] = kNarrowNoPair | (cp & kNarrowCpMask);
    }
    if (lane == 0) { L.symmask[blk] = SYM; L.sympre[blk] = nsym; }
    nw += (uint32_t)__popcll(WSTART);
    nsym += (uint32_t)__popcll(SYM);
    if (SYM) {
      const int li = 63 - __builtin_clzll(SYM);
      const unsigned long long tail = li == 63 ? 0ull : ~((2ull << li) - 1ull);
      const unsigned long long shut = ((WSm | PNm | SS) & tail) | (PNm & (1ull << li));
      pend_shut = (uint32_t)shut | (uint32_t)(shut >> 32);
      pend_cp = __builtin_amdgcn_readlane(sy, li);
    } else {
      pend_shut = 1u;  // a block without symbols holds whitespace: every word ended
    }
    prev_wb = WB >> 63;
  }
  wave_sync();
  C.abase = abase;
  C.off0 = off0;
  C.staged = staged;
  C.nblk = nblk;
  C.ce = staged;
  C.nsym = nsym;
  C.nw = nw;
  C.cut = cut;
  C.last = last;
  C.giant = false;
}

// ---- the end of a chunk that does not end the tile: one word longer than the staged bytes goes to the one-lane walker (and the
// chunk is done: C.giant), anything else is cut at its last word boundary.  Closes the word list and moves T.cb past the chunk.
// rules: what makes the long word its merge rule (lane_rules).
template <int Cap, int Mode, bool Packed, bool Narrow, class Rules>
__device__ __forceinline__ void lane_chunk_end(LaneLds<Cap, Narrow> &L, GiantResult &giant, const uint8_t *__restrict__ text, const uint64_t *__restrict__ sent_off,
                                               const uint8_t *__restrict__ cls_tab, const BpeSlot *__restrict__ slots, uint32_t sh,
                                               LaneTile &T, LaneChunk &C, int lane, uint32_t *__restrict__ sent_local,
                                               const uint32_t *__restrict__ uslot, unsigned long long *__restrict__ rec,
                                               unsigned long long *__restrict__ drec, const DirectOut &direct, const Rules &rules) {
  constexpr bool kDirect = Mode == 2, kRec = Mode == 1;
  if (!C.last) {
    if (C.cut < 0) {
      // a single word longer than the LDS chunk: one lane, global memory
      if (lane == 0) {
        uint64_t s = T.s_next;
        while (s < T.s_hi && sent_off[s] <= T.cb) s++;
        const uint64_t send = sent_off[s];  // s <= s_hi and sent_off[s_hi] = span_end > cb
        // the word's sentence is the last that starts at or before it, s - 1 (the tile's first starts at span_base <= cb: s > s_lo)
        giant = giant_word<Packed>(text, T.cb, send, cls_tab, slots, sh, T.tile_out + T.run, rules.of(s - 1, T.cb));
      }
      wave_sync();
      const GiantResult g = giant;
      uint32_t mine = 0;
      for (uint64_t s = T.s_next + lane; s < T.s_hi; s += 64) {
        if (sent_off[s] >= g.end) break;
        if (kDirect) direct.off[s] = T.run; else if (Mode == 0) sent_local[s] = T.run;
        if (kRec) {
          drec[s] = (unsigned long long)(T.span_base + T.run) | ((unsigned long long)g.ntok << 32);
          rec[uslot[s]] = (unsigned long long)s | ((unsigned long long)g.ntok << 32);
        }
        mine++;
      }
      for (int d = 32; d >= 1; d >>= 1) mine += __shfl_xor(mine, d);
      T.s_next += mine;
      T.run += g.ntok;
      T.cb = g.end;
      C.giant = true;
      C.nw = 0;
      C.nsym = 0;
      wave_sync();
      return;
    }
    // the cut is a word boundary: symbols and words at or beyond it are staged again by the next chunk
    C.ce = (uint32_t)C.cut;
    C.nsym = L.sympre[C.ce >> 6] + (uint32_t)__popcll(L.symmask[C.ce >> 6] & ((1ull << (C.ce & 63)) - 1ull));
    uint32_t keep = 0;
    for (uint32_t k0 = 0; k0 < C.nw; k0 += 64) {
      const uint32_t k = k0 + lane;
      keep += (uint32_t)__popcll(__ballot(k < C.nw && L.wl[k] < C.nsym));
    }
    C.nw = keep;
  }
  if (lane == 0) L.wl[C.nw] = (uint16_t)C.nsym;
  T.cb = C.abase + C.ce;
  wave_sync();
}

// ---- W. the words with two symbols or more by length class: how many, then their entries (the word's index in wl[]) into a list
// that holds all 9+ words first, then the 5-8, then the 2-4 (o2 / o1 / o0 = where this wave's share of each class begins)
template <int Cap, bool Narrow>
__device__ __forceinline__ void lane_words_count(const LaneLds<Cap, Narrow> &L, uint32_t nw, int lane, uint32_t &c2, uint32_t &c1, uint32_t &c0) {
  c0 = c1 = c2 = 0;
  for (uint32_t k0 = 0; k0 < nw; k0 += 64) {
    const uint32_t k = k0 + lane;
    const uint32_t n = k < nw ? (uint32_t)L.wl[k + 1] - (uint32_t)L.wl[k] : 0u;
    c0 += (uint32_t)__popcll(__ballot(n >= 2 && n <= 4));
    c1 += (uint32_t)__popcll(__ballot(n >= 5 && n <= 8));
    c2 += (uint32_t)__popcll(__ballot(n >= 9));
  }
}
template <int Cap, bool Narrow>
__device__ __forceinline__ void lane_words_write(const LaneLds<Cap, Narrow> &L, uint32_t nw, int lane, uint16_t *list, uint32_t o2, uint32_t o1,
                                                 uint32_t o0) {
  const unsigned long long lt = (1ull << lane) - 1ull;
  for (uint32_t k0 = 0; k0 < nw; k0 += 64) {
    const uint32_t k = k0 + lane;
    const uint32_t n = k < nw ? (uint32_t)L.wl[k + 1] - (uint32_t)L.wl[k] : 0u;
    const unsigned long long M0 = __ballot(n >= 2 && n <= 4), M1 = __ballot(n >= 5 && n <= 8), M2 = __ballot(n >= 9);
    if (n >= 9) list[o2 + (uint32_t)__popcll(M2 & lt)] = (uint16_t)k;
    else if (n >= 5) list[o1 + (uint32_t)__popcll(M1 & lt)] = (uint16_t)k;
    else if (n >= 2) list[o0 + (uint32_t)__popcll(M0 & lt)] = (uint16_t)k;
    o0 += (uint32_t)__popcll(M0);
    o1 += (uint32_t)__popcll(M1);
    o2 += (uint32_t)__popcll(M2);
  }
}

// ---- D. merge rounds (bpe.py:210-238) over a list of words, one lane per word.  A lane whose word is finished takes the next
// one of the list, so the wave goes through about as many rounds as its longest word needs -- the short words fill the lanes
// beside it.  An entry of the list is an index into wl[].
//
// The minimum of a round is found as a KEY = rank | slot (packed values: rank:16 | merged:16 -> rank:16 | 0:11 | slot:5; wide
// values: rank << 5 | slot), so one min per slot yields the leftmost smallest rank and its place; a dead slot's value is all
// ones (written when the slot dies) and slots past the word read slot n-1, which never has a pair.  (Scanning for the next
// minimum WHILE the two lookups of a round are in flight -- their slots blanked first, their values joining the minimum on
// arrival -- was measured and is not faster: 0.1905 against 0.1872 ms per call; the rounds are not waiting on the L2.)
template <bool Packed>
__device__ __forceinline__ uint32_t rank_key(uint32_t v, uint32_t slot) {
  return Packed ? ((v & 0xFFFF0000u) | slot) : (v >= (1u << 27) ? (0xFFFFFFE0u | slot) : ((v << 5) | slot));
}
template <bool Packed>
__device__ __forceinline__ uint32_t scan_key(const uint32_t *V, uint32_t n) {
  const uint32_t nm1 = n - 1u;
  uint32_t key = 0xFFFFFFFFu;
  for (uint32_t i0 = 0; i0 < nm1; i0 += 4) {
    const uint32_t i1 = min(i0 + 1u, nm1), i2 = min(i0 + 2u, nm1), i3 = min(i0 + 3u, nm1);
    const uint32_t k0 = rank_key<Packed>(V[i0], i0), k1 = rank_key<Packed>(V[i1], i1);
    const uint32_t k2 = rank_key<Packed>(V[i2], i2), k3 = rank_key<Packed>(V[i3], i3);
    key = min(min(key, k0), min(min(k1, k2), k3));
  }
  return key;
}
// Narrow: val[] holds the keys themselves, so a trip is two reads of two entries off one clamped base and two min3.  The base of
// the last trip is pulled back to n - 4 (a group that overlaps the one before is harmless to a minimum) and entry n - 1 -- the
// last symbol's, never a pair -- may be read; a word of two or three symbols reads entries 0 and 1 twice (d = 0) or 0, 1, 2
// (d = 1), never its neighbour's.
struct KeyScan {
  uint32_t lim4, d4;  // the largest base, and the second read's distance from the first; both in bytes
  __device__ __forceinline__ explicit KeyScan(uint32_t n) : lim4(4u * (n - 2u - min(n - 2u, 2u))), d4(4u * min(n - 2u, 2u)) {}
};
#ifdef SWT_SCAN_TRIPS
// diagnostic builds only: trips of the three scan loops as the WAVE executes them (one count per trip, by its first active lane):
// [0] when a lane takes a word, [1] after a round, [2] in the tail
__device__ unsigned long long g_scan_trips[3];
#endif
template <int Which>
__device__ __forceinline__ uint32_t scan_trip(const uint32_t *V, uint32_t i0, const KeyScan &ks, uint32_t key) {  // i0: a multiple of 4
#ifdef SWT_SCAN_TRIPS
  if (threadIdx.x == (unsigned)__builtin_ctzll(__ballot(1))) atomicAdd(&g_scan_trips[Which], 1ull);
#endif
  const uint32_t o = min(4u * i0, ks.lim4);
  const char *const v0 = reinterpret_cast<const char *>(V);
  const uint32_t *a = reinterpret_cast<const uint32_t *>(v0 + o), *b = reinterpret_cast<const uint32_t *>(v0 + ks.d4 + o);
  return min(min(min(min(key, a[0]), a[1]), b[0]), b[1]);
}
template <int Which>
__device__ __forceinline__ uint32_t scan_keys(const uint32_t *V, uint32_t n, const KeyScan &ks) {
  const uint32_t nm1 = n - 1u;
  uint32_t key = 0xFFFFFFFFu;
  for (uint32_t i0 = 0; i0 < nm1; i0 += 4) key = scan_trip<Which>(V, i0, ks, key);
  return key;
}
// A lane's word as the rounds hand it to their tail.
struct LaneWord {
  uint32_t n, alive;  // symbols (0: the lane holds no word), live slots (bit i: slot i still holds a symbol)
  uint32_t where;     // first symbol of the word in sym[] / val[]
};

// ---- the tail of the rounds.  Two thirds of a tile's rounds run with a handful of words left -- the longest ones, which started
// first -- and a round costs the wave the same whether 60 lanes take part or 5 (S85k-open, simulated from the oracle: 13.8 rounds per
// tile, 8.8 of them with <= 16 words, 6.9 with <= 8).  So the last 64 / TL words get TL lanes each: lane j of a word scans its share
// of the slots, a shuffle finds the word's minimum, every lane of the group follows the merge (same values, LDS broadcasts), lane 0
// writes it and looks the left pair up while lane 1 looks up the right.  LEAD = the lanes that hold a word's state on entry (at
// most 64 / TL of them); the function returns when every word is finished.
template <bool Packed, uint32_t TL, bool Seq, int Cap, bool Narrow>
__device__ __forceinline__ void lane_tail(LaneLds<Cap, Narrow> &L, const LaneWord &W, unsigned long long LEAD, int lane,
                                          const typename LaneSym<Narrow>::Slot *__restrict__ slots, uint32_t sh,
                                          const uint32_t *__restrict__ merged_of_rank, const NarrowDir &D) {
  constexpr uint32_t kNoKey = Narrow ? kNarrowNoPair : Packed ? 0xFFFF0000u : 0xFFFFFFE0u;  // keys from here up: no pair
  constexpr uint32_t kCont = LaneSym<Narrow>::kCont, kDead = LaneSym<Narrow>::kDead;
  // group g of TL lanes takes over the g-th word
  const uint32_t g = (uint32_t)lane / TL, j = (uint32_t)lane % TL;
  unsigned long long mrest = LEAD;
  for (uint32_t i = 0; i < g; i++) mrest &= mrest - 1ull;
  const bool have = mrest != 0ull;
  const int src = have ? __builtin_ctzll(mrest) : 0;
  const uint32_t t_w = __shfl(W.where, src), t_n = __shfl(W.n, src), t_alive = __shfl(W.alive, src);
  typename LaneSym<Narrow>::type *const S = L.sym + t_w;
  uint32_t *const V = L.val + t_w;
  uint32_t n = have ? t_n : 0u, alive = t_alive;
  [[maybe_unused]] const KeyScan ks(max(n, 2u));
  for (;;) {
    if (__ballot(n != 0u) == 0ull) break;
    if (n != 0u) {
      const uint32_t nm1 = n - 1u;
      uint32_t k = 0xFFFFFFFFu;
#pragma unroll
      for (uint32_t q0 = 0; q0 < 32u / TL; q0 += 4) {  // this lane's share of the (at most 32) slots
        const uint32_t i0 = (32u / TL) * j + q0;
        if (i0 < nm1) {
          if constexpr (Narrow) {
            k = scan_trip<2>(V, i0, ks, k);
          } else {
            const uint32_t i1 = min(i0 + 1u, nm1), i2 = min(i0 + 2u, nm1), i3 = min(i0 + 3u, nm1);
            k = min(k, min(min(rank_key<Packed>(V[i0], i0), rank_key<Packed>(V[i1], i1)), min(rank_key<Packed>(V[i2], i2), rank_key<Packed>(V[i3], i3))));
          }
        }
      }
#pragma unroll
      for (uint32_t d = 1; d < TL; d <<= 1) k = min(k, (uint32_t)__shfl_xor(k, (int)d));
      const uint32_t im = k & 31u;
      const uint32_t hi = alive & (0xFFFFFFFEu << im);
      if (k >= kNoKey || hi == 0u) {
        n = 0u;  // the same decision in all lanes of the group
      } else {
        const uint32_t m = Narrow ? k >> 16 : V[im];  // Narrow: the rank, which the key holds
        const uint32_t r = (uint32_t)__builtin_ctz(hi);
        const uint32_t hi2 = hi & (hi - 1u);
        const uint32_t lo = alive & ((1u << im) - 1u);
        const bool has_rr = hi2 != 0u, has_pl = lo != 0u;
        const uint32_t rr = has_rr ? (uint32_t)__builtin_ctz(hi2) : 0u, pl = has_pl ? 31u - (uint32_t)__builtin_clz(lo) : 0u;
        alive &= ~(1u << r);
        uint32_t mg;
        if constexpr (Narrow) mg = narrow_merged<Seq>(D, m); else mg = Packed ? (SWT_SYM_BASE + (m & 0xFFFFu)) : merged_of_rank[m];
        const uint32_t sl = S[pl] & ~kCont, sr = S[rr] & ~kCont;
        wave_sync();  // every lane has read the old symbols before lane 0 changes them
        const bool left = j == 0u && has_pl, right = j == 1u && has_rr;
        uint32_t v = kNoRank;
        if (left || right) v = slot_value(slots, sh, left ? sl : mg, left ? mg : sr);
        if constexpr (Narrow) v = slot_key(v, left ? pl : im);  // the entry of slot pl (lane 0) or im (lane 1)
        if (j == 0u) {
          S[im] = im ? (mg | kCont) : mg;
          S[r] = kDead;
          V[r] = kNoRank;
          if (has_pl && !(Narrow && sl == kNarrowForeign)) V[pl] = v;  // a FOREIGN symbol's entry is its code point
        }
        if (j == 1u) V[im] = v;  // kNoRank when nothing follows
      }
    }
    wave_sync();
  }
}

// BPE-dropout: what makes a word its DropRule -- the draws, and what a lane needs to find the key (i, b) of the word it takes,
// the chunk's place in the text and the tile's sentences.
struct DropSite {
  DropDraw dd;
  const uint64_t *sent_off;
  uint64_t s_lo, s_hi;  // the tile's sentences: sent_off[s_lo] <= every byte of the tile < sent_off[s_hi]
  uint64_t abase;       // LaneChunk::abase
  uint32_t nblk;        // LaneChunk::nblk
  __device__ __forceinline__ DropRule of(uint64_t s, uint64_t pos) const { return DropRule(dd, DropWord{(uint32_t)s, (uint32_t)(pos - sent_off[s])}); }
  // Symbol -> byte is the inverse of the split's byte -> symbol maps: the block whose sympre is the last at or below `where`, then
  // that many set bits into its symmask.  Byte -> sentence is a search of the tile's sentence offsets for the last at or below the
  // byte (empty sentences share an offset with the next sentence that has bytes, which is the last of them).
  template <int Cap>
  __device__ __forceinline__ DropRule of(const LaneLds<Cap, false> &L, uint32_t where) const {
    uint32_t blk = 0;
    while (blk + 1 < nblk && L.sympre[blk + 1] <= where) blk++;
    unsigned long long m = L.symmask[blk];
    for (uint32_t r = where - L.sympre[blk]; r != 0u && m != 0ull; r--) m &= m - 1ull;
    const uint64_t pos = abase + (uint64_t)blk * 64u + (m ? (uint32_t)__builtin_ctzll(m) : 0u);
    uint64_t lo = s_lo, hi = s_hi;
    while (hi - lo > 1) {
      const uint64_t mid = lo + (hi - lo) / 2;
      if (sent_off[mid] <= pos) lo = mid; else hi = mid;
    }
    return of(lo, pos);
  }
};
// The one thing a kernel makes of Ordered and Dropout, once per tile: what gives every word its merge rule (a DropSite learns
// the place of every chunk from the kernel).
template <bool Packed, bool Ordered, bool Dropout, class Direct>
__device__ __forceinline__ auto lane_rules(const uint32_t *__restrict__ info, const Direct &direct, const uint64_t *__restrict__ sent_off, const LaneTile &T) {
  if constexpr (Dropout) return DropSite{direct.draw, sent_off, T.s_lo, T.s_hi, 0u, 0u};
  else if constexpr (Ordered) return ListRule<Packed>{info};
  else return RankRule{};
}

// The rounds proper: until the list is empty and at most 16 words are still merging, which are returned for the tail.
// rules: what makes a word its merge rule (lane_rules).  Only under a RankRule are there rounds proper; under the other two
// every multi-symbol word is finished in the literal rounds where its lane takes it.
template <bool Packed, bool Proper, bool Seq, int Cap, bool Narrow, class Rules>
__device__ __forceinline__ LaneWord lane_rounds(LaneLds<Cap, Narrow> &L, const uint16_t *list, uint32_t n_list, int lane,
                                                const typename LaneSym<Narrow>::Slot *__restrict__ slots, uint32_t sh,
                                                const uint32_t *__restrict__ merged_of_rank, const NarrowDir &D, const Rules &rules) {
  constexpr bool Ranked = std::is_same_v<Rules, RankRule>;
  static_assert(Ranked || !(Narrow || Proper), "list order and dropout: wide symbols, the literal rounds alone");
  static_assert(!(Narrow && !Packed), "the narrow form is that of a packed table");
  constexpr uint32_t kNoKey = Narrow ? kNarrowNoPair : Packed ? 0xFFFF0000u : 0xFFFFFFE0u;  // keys from here up: no pair
  constexpr uint32_t kCont = LaneSym<Narrow>::kCont, kDead = LaneSym<Narrow>::kDead;
  const unsigned long long lt = (1ull << lane) - 1ull;
  uint32_t next = 0;  // first word of the list no lane has taken (the same in every lane)
  uint32_t n = 0, alive = 0, where = 0;  // this lane's word: symbols (0: none), live slots, first slot
  uint32_t key = 0xFFFFFFFFu;            // its smallest rank | the slot that holds it
  [[maybe_unused]] KeyScan ks(2u);       // Narrow: what a scan of its entries needs, kept with the word
  typename LaneSym<Narrow>::type *S = L.sym;
  uint32_t *V = L.val;
  for (;;) {
    const unsigned long long IDLE = __ballot(n == 0u);
    if (IDLE && next < n_list) {
      const uint32_t k = next + (uint32_t)__popcll(IDLE & lt);
      if (n == 0u && k < n_list) {
        const uint32_t e = list[k];
        where = L.wl[e];
        n = (uint32_t)L.wl[e + 1] - where;
        S = &L.sym[where];
        V = &L.val[where];
        alive = n >= 32u ? 0xFFFFFFFFu : (1u << n) - 1u;
        if (!Proper || n > 32u) {
          literal_rounds<Packed, Narrow, Seq>(S, V, n, slots, sh, merged_of_rank, D, rules.of(L, where));
          n = 0u;
        } else {
          if constexpr (Narrow) { ks = KeyScan(n); key = scan_keys<0>(V, n, ks); } else key = scan_key<Packed>(V, n);
        }
      }
      next += (uint32_t)__popcll(IDLE);
    }
    const unsigned long long BUSY = __ballot(n != 0u);
    if (next >= n_list && __popcll(BUSY) <= 16) break;  // the last few (long) words: several lanes each, lane_tail
    if (BUSY == 0ull) continue;  // every word just taken went through the literal rounds: take the next ones
    if (n != 0u) {
      // slot im merges with the next live slot r; pl / rr = the live slots either side of the pair
      const uint32_t im = key & 31u;
      const uint32_t hi = alive & (0xFFFFFFFEu << im);
      if (key >= kNoKey || hi == 0u) {
        n = 0u;  // the word is finished (hi == 0 cannot happen: a slot with a pair value has a live successor)
      } else {
        const uint32_t m = Narrow ? key >> 16 : V[im];  // Narrow: the rank, which the key holds
        const uint32_t r = (uint32_t)__builtin_ctz(hi);
        const uint32_t hi2 = hi & (hi - 1u);
        const uint32_t lo = alive & ((1u << im) - 1u);
        const bool has_rr = hi2 != 0u, has_pl = lo != 0u;
        const uint32_t rr = has_rr ? (uint32_t)__builtin_ctz(hi2) : 0u, pl = has_pl ? 31u - (uint32_t)__builtin_clz(lo) : im;
        alive &= ~(1u << r);
        uint32_t mg;
        if constexpr (Narrow) mg = narrow_merged<Seq>(D, m); else mg = Packed ? (SWT_SYM_BASE + (m & 0xFFFFu)) : merged_of_rank[m];
        const uint32_t sl = S[pl] & ~kCont, sr = S[rr] & ~kCont;
        S[im] = im ? (mg | kCont) : mg;
        S[r] = kDead;
        V[r] = kNoRank;
        const uint32_t v1 = slot_value(slots, sh, sl, mg), v2 = has_rr ? slot_value(slots, sh, mg, sr) : kNoRank;
        if (has_pl && !(Narrow && sl == kNarrowForeign)) V[pl] = Narrow ? slot_key(v1, pl) : v1;  // a FOREIGN symbol's entry is its code point
        V[im] = Narrow ? slot_key(v2, im) : v2;
        if constexpr (Narrow) key = scan_keys<1>(V, n, ks); else key = scan_key<Packed>(V, n);
      }
    }
  }
  return LaneWord{n, alive, where};
}

// ---- E + F of one chunk: order-preserving compaction of the live symbols into the tile's output run, then the tile-local
// token offset of every sentence starting in [cb, ce) (and == ce on the last chunk): byte -> symbol through the split's
// masks, symbol -> token through phase E's.  Advances the tile's sentences and its run.
// Narrow: a code goes out as the id it stands for -- a letter through D.cp_of_code, a merged symbol by its number, a FOREIGN one
// from its val[] entry.
template <int Cap, int Mode, bool Narrow>
__device__ __forceinline__ void lane_emit(LaneLds<Cap, Narrow> &L, const NarrowDir &D, const uint64_t *__restrict__ sent_off, LaneTile &T, const LaneChunk &C, int lane,
                                          uint32_t *__restrict__ sent_local, const uint32_t *__restrict__ uslot,
                                          unsigned long long *__restrict__ rec, unsigned long long *__restrict__ drec,
                                          const DirectOut &direct) {
  constexpr bool kDirect = Mode == 2, kRec = Mode == 1;
  const unsigned long long lt = (1ull << lane) - 1ull;
  uint32_t total = 0;
  for (uint32_t j0 = 0; j0 < C.nsym; j0 += 64) {
    const uint32_t j = j0 + lane;
    constexpr uint32_t kDead = LaneSym<Narrow>::kDead;
    const uint32_t sv = j < C.nsym ? L.sym[j] : kDead;
    const unsigned long long m = __ballot(sv != kDead);
    if (lane == 0) { L.vmask[j0 >> 6] = m; L.blkpre[j0 >> 6] = total; }
    uint32_t id = sv;
    if constexpr (Narrow) {
      const uint32_t c = sv & ~kNarrowCont;  // (a dead slot's code is neither a letter nor FOREIGN: it reads nothing)
      id = c + (SWT_SYM_BASE - D.letters);
      if (c < D.letters) id = global_ptr(D.cp_of_code)[c];
      if (c == kNarrowForeign) id = L.val[j] & kNarrowCpMask;
      id |= (sv & kNarrowCont) << 16;
    }
    if (sv != kDead) T.tile_out[T.run + total + (uint32_t)__popcll(m & lt)] = id;
    total += (uint32_t)__popcll(m);
  }
  wave_sync();
  auto tokens_before = [&](uint64_t rel) -> uint32_t {
    if (rel >= C.ce || (rel >> 6) >= C.nblk) return total;
    const uint32_t sidx = L.sympre[rel >> 6] + (uint32_t)__popcll(L.symmask[rel >> 6] & ((1ull << (rel & 63)) - 1ull));
    if (sidx >= C.nsym) return total;
    return L.blkpre[sidx >> 6] + (uint32_t)__popcll(L.vmask[sidx >> 6] & ((1ull << (sidx & 63)) - 1ull));
  };
  uint32_t mine = 0;
  for (uint64_t s = T.s_next + lane; s < T.s_hi; s += 64) {
    const uint64_t rel = sent_off[s] - C.abase;
    if (rel > C.ce || (rel == C.ce && !C.last)) break;
    const uint32_t e = tokens_before(rel);
    if (kDirect) direct.off[s] = T.run + e; else if (Mode == 0) sent_local[s] = T.run + e;
    if (kRec && rel < C.ce) {  // a word never straddles the cut, so its end lies in this chunk too
      const uint32_t e2 = tokens_before(sent_off[s + 1] - C.abase);
      drec[s] = (unsigned long long)(T.span_base + T.run + e) | ((unsigned long long)(e2 - e) << 32);
      rec[uslot[s]] = (unsigned long long)s | ((unsigned long long)(e2 - e) << 32);
    }
    mine++;
  }
  for (int d = 32; d >= 1; d >>= 1) mine += __shfl_xor(mine, d);
  T.s_next += mine;
  T.run += total;
  wave_sync();
}

#ifdef SWT_STAMPS
// diagnostic builds only: wall_clock64() at the begin and the end of Mode 0 wave t, [2t] and [2t + 1] (zero: the wave had no work)
constexpr uint32_t kLaneStamps = 65536;  // S85k in tapering tiles: 31 k to 45 k waves
__device__ unsigned long long g_lane_stamp[2 * kLaneStamps];
#endif

// One wave per tile: running text (Mode 0), the unique words of the dedup path (Mode 1), the single-workgroup call (Mode 2).
// The DROPOUT form (swt_bpe_encode_dropout*, include/swt.h; template parameter Dropout): the same wave over the same staging,
// split, emit, scan and gather, every multi-symbol word through the literal rounds under a DropRule -- one lane per word, as the
// ordered form.  Wide symbols, Mode 0 or 2.  Its draws travel behind the DirectOut in its last argument (DirectDrop); every other
// instantiation has the arguments it always had.
struct DirectDrop : DirectOut { DropDraw draw; };
template <bool Packed, bool Proper, int Cap, int Mode, bool Ordered = false, bool Narrow = false, bool Seq = false, bool Dropout = false>
__global__ __launch_bounds__(64) void bpe_lane_kernel(
    const uint8_t *__restrict__ text, uint64_t n_bytes, const uint64_t *__restrict__ sent_off,
    const uint64_t *__restrict__ plan, const uint8_t *__restrict__ cls_tab, const BpeSlot *__restrict__ slots,
    uint32_t sh, const uint32_t *__restrict__ merged_of_rank, uint32_t *__restrict__ scratch,
    uint32_t *__restrict__ sent_local, uint32_t *__restrict__ tile_tok, const uint32_t *__restrict__ uslot,
    unsigned long long *__restrict__ rec, unsigned long long *__restrict__ drec, std::conditional_t<Dropout, DirectDrop, DirectOut> direct) {
  constexpr bool kDirect = Mode == 2;
  static_assert(Cap % 64 == 0 && Cap <= 4032, "11 B of LDS per staged byte and the masks (Narrow: 9 B); wl[] and the word list hold 16-bit indices");
  static_assert(!Narrow || (Mode == 0 && Packed && !Ordered), "the narrow form: running text, a packed table, FastBPE's order");
  static_assert(!Seq || Narrow, "Seq says where the narrow form's rounds get the merged code from");
  static_assert(!Narrow || kLaneCap != 512 || sizeof(LaneLds<Cap, true>) + sizeof(LaneShared<true>) <= sizeof(LaneLds<kLaneCap>) + sizeof(LaneShared<false>),
                "the narrow kernel's chunk is sized to the LDS of the wide one, so that as many waves reside");
  static_assert(!Dropout || (Mode != 1 && !Narrow && !Ordered && !Proper), "the dropout form: running text or the single workgroup, wide symbols, FastBPE's ranks");
  using Slot = typename LaneSym<Narrow>::Slot;
  __shared__ LaneLds<Cap, Narrow> L;
  __shared__ LaneShared<Narrow> SH;
  const Slot *const tab = reinterpret_cast<const Slot *>(slots);  // Narrow: the launch passes the table of the codes here
  NarrowDir D{};
  if constexpr (Narrow) D = *reinterpret_cast<const NarrowDir *>(merged_of_rank);
  const int lane = threadIdx.x;
  const uint64_t t = blockIdx.x;
#ifdef SWT_STAMPS
  const unsigned long long stamp0 = wall_clock64();
#endif
  LaneTile T;
  T.s_lo = kDirect ? 0 : plan[t];
  T.s_hi = kDirect ? direct.n_sent : plan[t + 1];
  if (T.s_lo == T.s_hi) {
    if (Mode == 0 && lane == 0) tile_tok[t] = 0;
    return;
  }
  if constexpr (!Narrow) lane_classes(SH, cls_tab, lane);
  T.span_base = sent_off[T.s_lo];
  T.span_end = sent_off[T.s_hi];
  T.tile_out = scratch + T.span_base;
  T.run = 0;
  T.s_next = T.s_lo;
  T.cb = T.span_base;
  uint16_t *const list = reinterpret_cast<uint16_t *>(L.txt);  // the staged bytes are not read again once the split is done
  auto rules = lane_rules<Packed, Ordered, Dropout>(merged_of_rank, direct, sent_off, T);
  for (;;) {
    LaneChunk C;
    lane_split(L, SH.cls2, D, text, n_bytes, sent_off, cls_tab, tab, sh, T, C, lane);
    // (the one-lane walker of a word longer than a chunk works on ids, whatever the kernel's symbols are)
    // (Narrow: their table comes out of the directory as a generic pointer and stays one: the walker's three loads of a slot are
    // the kernel's only flat loads, and marking the table global cost the kernel 0.5 M vector instructions a launch in registers
    // moved about, profiles/lane_diet.txt section 4)
    if constexpr (Dropout) { rules.abase = C.abase; rules.nblk = C.nblk; }
    lane_chunk_end<Cap, Mode, Packed>(L, SH.giant, text, sent_off, cls_tab, Narrow ? D.wide_slots : slots, Narrow ? D.wide_sh : sh, T, C, lane, sent_local, uslot,
                                      rec, drec, direct, rules);
    if (C.giant) continue;
    uint32_t c2, c1, c0;
    lane_words_count(L, C.nw, lane, c2, c1, c0);
    lane_words_write(L, C.nw, lane, list, 0u, c2, c2 + c1);
    wave_sync();
    // the rounds, then four lanes a word once the list is empty and 16 words are left (lane_tail)
    // (dropout: every word is finished where its lane takes it, and nothing is left for the tail)
    const LaneWord W = lane_rounds<Packed, Proper, Seq, Cap>(L, list, c2 + c1 + c0, lane, tab, sh, merged_of_rank, D, rules);
    const unsigned long long BUSY = __ballot(W.n != 0u);
    if (BUSY != 0ull) lane_tail<Packed, 4, Seq, Cap>(L, W, BUSY, lane, tab, sh, merged_of_rank, D);
    wave_sync();
    lane_emit<Cap, Mode>(L, D, sent_off, T, C, lane, sent_local, uslot, rec, drec, direct);
    if (C.last) break;
  }
  if (lane == 0) {
    if (kDirect) { direct.off[T.s_hi] = T.run; *direct.n_tokens = T.run; }
    else if (Mode == 0) tile_tok[t] = T.run;
#ifdef SWT_STAMPS
    if (Mode == 0 && t < kLaneStamps) { g_lane_stamp[2 * t] = stamp0; g_lane_stamp[2 * t + 1] = wall_clock64(); }
#endif
  }
}

}  // namespace swt

using namespace swt;

struct swt_bpe_table {
  std::vector<BpeSlot> h_slots;    // built on the host at create; uploaded on first encode
  std::vector<uint32_t> h_merged;  // merged symbol id by rank
  bool packed = false;             // slot value = rank << 16 | (merged - SWT_SYM_BASE)
  bool proper = false;             // every pair ranks above the merges that produce its symbols (any trained table)
  BpeSlot *d_slots = nullptr;
  uint32_t *d_merged = nullptr;
  uint32_t bits = 0;
  // NaiveBPE's list order (swt_bpe_encode_naive*).  order_equivalent: no pair listed twice and the table proper, so list order
  // and lowest-rank-first give the same tokens and the naive entry points run the FastBPE path as it is.  Otherwise the ordered
  // form of the kernel runs over h_oslots (the FIRST list position of every pair, same layout and hashes as h_slots) and h_oinfo
  // ([2i] merged symbol of position i, [2i + 1] next position of the same pair or kNoRank), uploaded on the first naive call.
  bool order_equivalent = false;
  std::vector<BpeSlot> h_oslots;
  std::vector<uint32_t> h_oinfo;
  BpeSlot *d_oslots = nullptr;
  uint32_t *d_oinfo = nullptr;
  uint32_t obits = 0;
  uint32_t n_merges = 0;
  TileWorkspace ws;
  HostStage stage;  // the host entry points (host_encode*, swt_tile.h)
  // word-level dedup inside one call
  TileWorkspace ws2;          // workspaces of the encode over the unique words
  DedupEngine dd;
  int opt_unique_tile = 0;  // SWT_OPT_UNIQUE_TILE
  int opt_lane_span = 0;    // SWT_OPT_LANE_SPAN
  int opt_lane_taper = 0;   // SWT_OPT_LANE_TAPER
  int opt_lane_slots = 0;   // SWT_OPT_LANE_SLOTS
  int opt_lane_narrow = 0;  // SWT_OPT_LANE_NARROW
  int last_lane_narrow = -1;  // what the last running-text launch took: 1 the narrow kernel, 0 a wide one, -1 none yet (diagnostics)
  uint64_t lane_slots[4] = {0, 0, 0, 0};  // wave slots of the device for the running-text kernel of this table ([1]: its ordered form, [2]: its narrow form, [3]: its dropout form)
  // 16-bit symbol codes (swt_bpe_narrow.h) for the narrow form of the running-text kernel; empty unless narrow.eligible
  NarrowTable narrow;
  NarrowSlot *d_nslots = nullptr;
  uint32_t *d_ncodes = nullptr;  // code_of_cp, then cp_of_code, then (a table that is not sequential) code_of_rank
  NarrowDir *d_ndir = nullptr;
};

// The narrow kernel's tables.  The handle has them once d_ndir is set, and d_ndir is set last: a call that fails on the way
// frees what it allocated and leaves the handle without them, so the next call tries again and no launch sees half of them.
static int bpe_upload_narrow(swt_bpe_table *t) {
  if (!t->narrow.eligible || t->d_ndir) return SWT_OK;
  const NarrowTable &n = t->narrow;
  std::vector<uint32_t> codes = n.code_of_cp(host_class_table());
  const uint32_t n_cps = (uint32_t)codes.size();
  codes.insert(codes.end(), n.cp_of_code.begin(), n.cp_of_code.end());
  const size_t at_ranks = codes.size();
  if (!n.sequential) codes.insert(codes.end(), n.code_of_rank.begin(), n.code_of_rank.end());
  NarrowSlot *d_nslots = nullptr;
  uint32_t *d_ncodes = nullptr;
  NarrowDir *d_ndir = nullptr;
  hipError_t e = hipMalloc((void **)&d_nslots, n.slots.size() * sizeof(NarrowSlot));
  if (e == hipSuccess) e = hipMemcpy(d_nslots, n.slots.data(), n.slots.size() * sizeof(NarrowSlot), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMalloc((void **)&d_ncodes, (codes.size() + 1) * 4);
  if (e == hipSuccess) e = hipMemcpy(d_ncodes, codes.data(), codes.size() * 4, hipMemcpyHostToDevice);
  const NarrowDir dir{t->d_slots, d_ncodes, d_ncodes + n_cps, n.sequential ? nullptr : d_ncodes + at_ranks, 32u - t->bits, n_cps, n.letters(), 0u};
  if (e == hipSuccess) e = hipMalloc((void **)&d_ndir, sizeof dir);
  if (e == hipSuccess) e = hipMemcpy(d_ndir, &dir, sizeof dir, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    if (d_nslots) (void)hipFree(d_nslots);
    if (d_ncodes) (void)hipFree(d_ncodes);
    if (d_ndir) (void)hipFree(d_ndir);
    SWT_HIP(e);
  }
  t->d_nslots = d_nslots;
  t->d_ncodes = d_ncodes;
  t->d_ndir = d_ndir;
  return SWT_OK;
}

static int bpe_upload(swt_bpe_table *t) {
  if (t->d_slots) return bpe_upload_narrow(t);
  int rc = ensure_device();
  if (rc) return rc;
  SWT_HIP(hipMalloc((void **)&t->d_slots, t->h_slots.size() * sizeof(BpeSlot)));
  SWT_HIP(hipMemcpy(t->d_slots, t->h_slots.data(), t->h_slots.size() * sizeof(BpeSlot), hipMemcpyHostToDevice));
  SWT_HIP(hipMalloc((void **)&t->d_merged, (t->h_merged.size() + 1) * 4));
  if (!t->h_merged.empty())
    SWT_HIP(hipMemcpy(t->d_merged, t->h_merged.data(), t->h_merged.size() * 4, hipMemcpyHostToDevice));
  return bpe_upload_narrow(t);
}

static int bpe_upload_ordered(swt_bpe_table *t) {
  if (t->d_oslots || t->order_equivalent) return SWT_OK;
  SWT_HIP(hipMalloc((void **)&t->d_oslots, t->h_oslots.size() * sizeof(BpeSlot)));
  SWT_HIP(hipMemcpy(t->d_oslots, t->h_oslots.data(), t->h_oslots.size() * sizeof(BpeSlot), hipMemcpyHostToDevice));
  SWT_HIP(hipMalloc((void **)&t->d_oinfo, (t->h_oinfo.size() + 2) * 4));
  if (!t->h_oinfo.empty())
    SWT_HIP(hipMemcpy(t->d_oinfo, t->h_oinfo.data(), t->h_oinfo.size() * 4, hipMemcpyHostToDevice));
  return SWT_OK;
}

// what a launch reads the ranks from: the FastBPE table, or the ordered one (first positions + chain)
struct BpeView { const BpeSlot *slots; const uint32_t *merged; uint32_t sh; };
static BpeView bpe_view(const swt_bpe_table *t, bool ordered) {
  return ordered ? BpeView{t->d_oslots, t->d_oinfo, 32u - t->obits} : BpeView{t->d_slots, t->d_merged, 32u - t->bits};
}

// Which bpe_lane_kernel a launch gets.  Mode (the kernel's: 0 tiles of running text, 1 the unique words of the dedup path, 2 the
// single workgroup) is the caller's; from the table come Packed and Proper, from the entry point Ordered (which has no Proper
// form: every word goes through the literal rounds), from the tile size of the launch the chunk size -- `cap` bytes where the tiled
// forms have it (128, 256), kLaneCap otherwise; the single workgroup exists at kLaneCap only.
using LaneKernel = decltype(&bpe_lane_kernel<true, true, kLaneCap, 0>);
template <int Cap, int Mode>
static LaneKernel lane_kernel_at(bool packed, bool proper, bool ordered) {
  if (ordered) return packed ? bpe_lane_kernel<true, false, Cap, Mode, true> : bpe_lane_kernel<false, false, Cap, Mode, true>;
  if (packed) return proper ? bpe_lane_kernel<true, true, Cap, Mode> : bpe_lane_kernel<true, false, Cap, Mode>;
  return proper ? bpe_lane_kernel<false, true, Cap, Mode> : bpe_lane_kernel<false, false, Cap, Mode>;
}
template <int Mode>
static LaneKernel lane_kernel(const swt_bpe_table *t, bool ordered, int cap = kLaneCap) {
  if constexpr (Mode != 2) {
    if (cap == 128) return lane_kernel_at<128, Mode>(t->packed, t->proper, ordered);
    if (cap == 256) return lane_kernel_at<256, Mode>(t->packed, t->proper, ordered);
  }
  return lane_kernel_at<kLaneCap, Mode>(t->packed, t->proper, ordered);
}
// The narrow form (16-bit symbols, kNarrowCap bytes a chunk) runs the running text of an eligible table in FastBPE's order from
// one chip-full of kLaneTile-byte tiles up: below that every wave is resident at once, the call lasts as long as its longest
// wave, and a larger tile only makes that wave longer (profiles/lane_narrow.txt section 5: 64 KB to 1 MB lose 5 - 11 us to the
// narrow kernel, 2.5 MB gains 5).  SWT_OPT_LANE_NARROW = 1 keeps the wide kernel, 2 takes the narrow one at every size.  The
// unique-word pass and the single workgroup stay wide: their chunks are sized by their tiles (128 to 512 bytes of words, one
// short call), not by the LDS, so 16-bit symbols would buy them nothing.
static uint64_t lane_slots(swt_bpe_table *t, bool ordered, bool narrow, bool dropout = false);
static bool lane_narrow(swt_bpe_table *t, bool ordered, uint64_t n_bytes) {
  if (!t->narrow.eligible || ordered || t->opt_lane_narrow == 1) return false;
  return t->opt_lane_narrow == 2 || n_bytes >= (uint64_t)kLaneTile * lane_slots(t, false, false);
}
// The dropout form (bpe_lane_kernel's Dropout): running text or the single workgroup, by the table's values alone.
using DropoutKernel = decltype(&bpe_lane_kernel<true, false, kLaneCap, 0, false, false, false, true>);
template <int Mode>
static DropoutKernel lane_kernel_dropout(const swt_bpe_table *t) {
  return t->packed ? bpe_lane_kernel<true, false, kLaneCap, Mode, false, false, false, true> : bpe_lane_kernel<false, false, kLaneCap, Mode, false, false, false, true>;
}
static LaneKernel lane_kernel_narrow(const swt_bpe_table *t) {
  if (t->narrow.sequential) return t->proper ? bpe_lane_kernel<true, true, kNarrowCap, 0, false, true, true> : bpe_lane_kernel<true, false, kNarrowCap, 0, false, true, true>;
  return t->proper ? bpe_lane_kernel<true, true, kNarrowCap, 0, false, true> : bpe_lane_kernel<true, false, kNarrowCap, 0, false, true>;
}
// The largest tile of a running-text call.  The narrow kernel's own geometry has kNarrowTile; a call whose geometry is SET
// (SWT_OPT_LANE_TAPER, SWT_OPT_LANE_SPAN) keeps the sizes those options are documented with, kLaneTile at the top, whichever
// kernel runs it -- the narrow kernel takes any tile up to its own -- unless SWT_OPT_LANE_NARROW = 2 asks for the narrow sizes.
static bool lane_narrow_tiles(swt_bpe_table *t, bool ordered, uint64_t n_bytes) {
  return lane_narrow(t, ordered, n_bytes) && (t->opt_lane_narrow == 2 || (!t->opt_lane_taper && !t->opt_lane_span));
}

extern "C" {

// diagnostics (not part of include/swt.h): what swt_bpe_table_create decided.  0: log2 of the slots, 1: packed values,
// 2: proper (every pair ranks above the merges producing its symbols), 3: entries in the table, 4: every entry is found where
// a device lookup looks for it (its first or its second slot) and nowhere else, 5: order-equivalent (no pair listed twice and
// proper: NaiveBPE's list order, bpe.py:126-127, gives what FastBPE's lowest rank first gives, and swt_bpe_encode_naive* run the
// FastBPE path), 6: entries in the ordered table (0 for an order-equivalent table, which has none), 7: which running-text calls in
// FastBPE's order take the NARROW kernel -- 0 none (not eligible, or SWT_OPT_LANE_NARROW = 1), 1 those of a chip-full of tiles
// and more (the library's choice), 2 all (SWT_OPT_LANE_NARROW = 2), 8: eligible for it (packed and letters + merges <= 0x7FFD),
// 9: letters of its alphabet (0 when not eligible), 11: the kernel the LAST running-text launch of this handle took, written where
// the launch picks it -- 1 the narrow kernel, 0 a wide one, -1 no such launch yet, 12: the narrow kernel's rounds get the merged
// code as letters + rank (1: NarrowTable::sequential, the Seq kernels) or read it from code_of_rank (0; also when not eligible),
// 13: log2 of the slots of the table of the codes (0 when not eligible)
int swt_debug_bpe_table_info(const swt_bpe_table *t, int which) try {
  if (!t) return -1;
  if (which == 7) return !t->narrow.eligible || t->opt_lane_narrow == 1 ? 0 : t->opt_lane_narrow == 2 ? 2 : 1;
  if (which == 8) return t->narrow.eligible ? 1 : 0;
  if (which == 9) return (int)t->narrow.letters();
  if (which == 11) return t->last_lane_narrow;
  if (which == 12) return t->narrow.eligible && t->narrow.sequential ? 1 : 0;
  if (which == 13) return (int)t->narrow.bits;
  if (which == 0) return (int)t->bits;
  if (which == 1) return t->packed ? 1 : 0;
  if (which == 2) return t->proper ? 1 : 0;
  if (which == 5) return t->order_equivalent ? 1 : 0;
  if (which == 6) {
    int n = 0;
    for (const BpeSlot &sl : t->h_oslots) n += sl.key != kEmptyKey;
    return n;
  }
  uint32_t n = 0;
  bool placed = true;
  const uint32_t sh = 32u - t->bits;
  for (size_t i = 0; i < t->h_slots.size(); i++) {
    const BpeSlot &sl = t->h_slots[i];
    if (sl.key == kEmptyKey) continue;
    n++;
    const uint32_t l = (uint32_t)(sl.key >> 32), r = (uint32_t)sl.key;
    const uint32_t h1 = bpe_hash(l, r, sh, kHash1), h2 = bpe_hash(l, r, sh, kHash2);
    if (i != h1 && i != h2) placed = false;
    if (h1 != h2 && t->h_slots[i == h1 ? h2 : h1].key == sl.key) placed = false;
  }
  return which == 3 ? (int)n : (placed ? 1 : 0);
} SWT_API_CATCH

#ifdef SWT_SCAN_TRIPS
// diagnostic builds only: copies the three trip counts out (take, after a round, tail) and clears them
int swt_debug_scan_trips(unsigned long long *out) try {
  void *d = nullptr;
  SWT_HIP(hipDeviceSynchronize());
  SWT_HIP(hipGetSymbolAddress(&d, HIP_SYMBOL(g_scan_trips)));
  SWT_HIP(hipMemcpy(out, d, sizeof(unsigned long long) * 3, hipMemcpyDeviceToHost));
  SWT_HIP(hipMemset(d, 0, sizeof(unsigned long long) * 3));
  return SWT_OK;
} SWT_API_CATCH
#endif
#ifdef SWT_STAMPS
// diagnostic builds only: copies the stamps of the last Mode 0 launch out (2 * swt_debug_lane_stamp_count() values) and clears them
int swt_debug_lane_stamp_count() { return (int)kLaneStamps; }
int swt_debug_lane_stamps(unsigned long long *out) try {
  void *d = nullptr;
  SWT_HIP(hipDeviceSynchronize());
  SWT_HIP(hipGetSymbolAddress(&d, HIP_SYMBOL(g_lane_stamp)));
  SWT_HIP(hipMemcpy(out, d, sizeof(unsigned long long) * 2 * kLaneStamps, hipMemcpyDeviceToHost));
  SWT_HIP(hipMemset(d, 0, sizeof(unsigned long long) * 2 * kLaneStamps));
  return SWT_OK;
} SWT_API_CATCH
#endif

}  // extern "C"

// Two-choice cuckoo placement (see slot_lookup) of the merges i with pick[pair] == i; a table that does not settle gets twice
// the slots.  False when it cannot be placed.
static bool place_slots(const uint32_t *left, const uint32_t *right, const uint32_t *merged, uint32_t n_merges,
                        std::unordered_map<uint64_t, uint32_t> &pick, std::vector<BpeSlot> &slots, uint32_t &bits_out) {
  uint32_t bits = 4;
  while ((1ull << bits) < 2ull * n_merges + 2) bits++;
  const uint32_t bits0 = bits;
  for (;; bits++) {
    if (bits > 28 || bits > bits0 + 4) return false;
    const uint32_t sh = 32u - bits;
    slots.assign((size_t)1 << bits, BpeSlot{kEmptyKey, 0u, 0u});
    bool ok = true;
    for (uint32_t i = 0; i < n_merges && ok; i++) {
      if (pick[pair_key(left[i], right[i])] != i) continue;
      BpeSlot cur{pair_key(left[i], right[i]), i, merged[i]};
      uint32_t avoid = 0xFFFFFFFFu;
      ok = false;
      for (int kick = 0; kick < 2000; kick++) {
        const uint32_t l = (uint32_t)(cur.key >> 32), r = (uint32_t)cur.key;
        const uint32_t h1 = bpe_hash(l, r, sh, kHash1), h2 = bpe_hash(l, r, sh, kHash2);
        if (slots[h1].key == kEmptyKey) { slots[h1] = cur; ok = true; break; }
        if (slots[h2].key == kEmptyKey) { slots[h2] = cur; ok = true; break; }
        const uint32_t j = h1 == avoid ? h2 : h1;  // evict, but not from the slot this entry was just evicted from
        std::swap(cur, slots[j]);
        avoid = j;
      }
    }
    if (ok) break;
  }
  bits_out = bits;
  return true;
}

extern "C" {

int swt_bpe_table_create(const uint32_t *left, const uint32_t *right, const uint32_t *merged, uint32_t n_merges,
                         swt_bpe_table **out) try {
  if (!out || (n_merges && (!left || !right || !merged))) return fail(SWT_ERR_INVALID, "null argument");
  for (uint32_t i = 0; i < n_merges; i++)
    if ((left[i] | right[i] | merged[i]) & SWT_BPE_CONT) return fail(SWT_ERR_INVALID, "symbol id out of range at merge %u", i);
  // {pair: i} (bpe.py:257): a later duplicate overwrites, so only the LAST index of a pair goes into the table
  std::unordered_map<uint64_t, uint32_t> last;
  last.reserve((size_t)n_merges * 2 + 16);
  for (uint32_t i = 0; i < n_merges; i++) last[pair_key(left[i], right[i])] = i;
  auto *t = new swt_bpe_table();
  std::vector<BpeSlot> &slots = t->h_slots;
  if (!place_slots(left, right, merged, n_merges, last, slots, t->bits)) {
    delete t;
    return fail(SWT_ERR_UNSUPPORTED, "the rank table could not be placed (%u pairs)", n_merges);
  }
  t->n_merges = n_merges;
  // proper: every pair ranks above every merge that produces one of its symbols, so the pairs a merge creates rank above it
  // and "one occurrence of the best pair per round" equals the reference's "all occurrences" (bpe_lane_kernel)
  {
    std::unordered_map<uint32_t, uint32_t> maxprod;
    for (const auto &sl : slots)
      if (sl.key != kEmptyKey) {
        auto it = maxprod.find(sl.merged);
        if (it == maxprod.end()) maxprod[sl.merged] = sl.rank; else if (sl.rank > it->second) it->second = sl.rank;
      }
    t->proper = true;
    for (const auto &sl : slots)
      if (sl.key != kEmptyKey) {
        for (uint32_t sy : {(uint32_t)(sl.key >> 32), (uint32_t)sl.key}) {
          auto it = maxprod.find(sy);
          if (it != maxprod.end() && it->second >= sl.rank) t->proper = false;
        }
      }
  }
  t->h_merged.assign(merged, merged + n_merges);
  // packed values when every rank and every merged-symbol index fits 16 bits (any realistic table below 65k merges)
  t->packed = n_merges < 0xFFFEu;
  for (uint32_t i = 0; i < n_merges && t->packed; i++)
    if (merged[i] < SWT_SYM_BASE || merged[i] - SWT_SYM_BASE >= 0xFFFFu) t->packed = false;
  // NaiveBPE applies the list in order (bpe.py:126-127), every position of a repeated pair in its turn.  Without repeats and
  // on a proper table that is FastBPE's result and nothing more is built; otherwise the ordered form of the kernel gets the
  // first position of every pair and the chain through its later ones (ListRule::value).
  t->order_equivalent = t->proper && last.size() == n_merges;
  if (!t->order_equivalent) {
    std::unordered_map<uint64_t, uint32_t> first, seen;
    first.reserve((size_t)n_merges * 2 + 16);
    seen.reserve((size_t)n_merges * 2 + 16);
    t->h_oinfo.assign((size_t)n_merges * 2, kNoRank);
    for (uint32_t i = n_merges; i-- > 0;) {
      const uint64_t k = pair_key(left[i], right[i]);
      auto it = seen.find(k);
      t->h_oinfo[2 * (size_t)i] = merged[i];
      if (it != seen.end()) t->h_oinfo[2 * (size_t)i + 1] = it->second;
      seen[k] = i;
      first[k] = i;
    }
    if (!place_slots(left, right, merged, n_merges, first, t->h_oslots, t->obits)) {
      delete t;
      return fail(SWT_ERR_UNSUPPORTED, "the ordered rank table could not be placed (%u pairs)", n_merges);
    }
  }
  {
    std::vector<bool> live(n_merges);
    for (uint32_t i = 0; i < n_merges; i++) live[i] = last[pair_key(left[i], right[i])] == i;
    narrow_build(left, right, merged, n_merges, t->packed, live, t->narrow);
  }
  if (t->packed) {
    for (auto &sl : slots)
      if (sl.key != kEmptyKey) sl.rank = (sl.rank << 16) | (sl.merged - SWT_SYM_BASE);
    for (auto &sl : t->h_oslots)
      if (sl.key != kEmptyKey) sl.rank = (sl.rank << 16) | (sl.merged - SWT_SYM_BASE);
  }
  *out = t;
  return SWT_OK;
} SWT_API_CATCH

int swt_bpe_table_set_option(swt_bpe_table *t, int option, int value) try {
  if (!t) return fail(SWT_ERR_INVALID, "null table");
  switch (option) {
    case SWT_OPT_DEDUP:
      if (value < 0 || value > 2) return fail(SWT_ERR_INVALID, "SWT_OPT_DEDUP takes 0, 1 or 2");
      t->dd.opt_mode = value;
      return SWT_OK;
    case SWT_OPT_DEDUP_TABLE_BITS:
      if (value != 0 && (value < 4 || value > 24)) return fail(SWT_ERR_INVALID, "SWT_OPT_DEDUP_TABLE_BITS takes 0 or 4..24");
      t->dd.opt_table_bits = (uint32_t)value;
      return SWT_OK;
    case SWT_OPT_UNIQUE_TILE:
      if (value != 0 && value != 64 && value != 128 && value != 256) return fail(SWT_ERR_INVALID, "SWT_OPT_UNIQUE_TILE takes 0, 64, 128 or 256");
      t->opt_unique_tile = value;
      return SWT_OK;
    case SWT_OPT_LANE_SPAN:
      if (value < 0 || value > (int)kLaneMaxSpan) return fail(SWT_ERR_INVALID, "SWT_OPT_LANE_SPAN takes 0..%u", kLaneMaxSpan);
      t->opt_lane_span = value;
      return SWT_OK;
    case SWT_OPT_LANE_TAPER:
      if (value < 0 || ((value & ~256) > (int)kTaperMaxC8) || value == 256 || value == 257)
        return fail(SWT_ERR_INVALID, "SWT_OPT_LANE_TAPER takes 0, 1, 2..%u or 256 + 2..%u", kTaperMaxC8, kTaperMaxC8);
      t->opt_lane_taper = value;
      return SWT_OK;
    case SWT_OPT_LANE_SLOTS:
      if (value < 0 || value > (int)kTaperMaxSlots) return fail(SWT_ERR_INVALID, "SWT_OPT_LANE_SLOTS takes 0..%u", kTaperMaxSlots);
      t->opt_lane_slots = value;
      return SWT_OK;
    case SWT_OPT_LANE_NARROW:
      if (value < 0 || value > 2) return fail(SWT_ERR_INVALID, "SWT_OPT_LANE_NARROW takes 0, 1 or 2");
      t->opt_lane_narrow = value;
      return SWT_OK;
  }
  return fail(SWT_ERR_INVALID, "no such option");
} SWT_API_CATCH

void swt_bpe_table_destroy(swt_bpe_table *t) try {
  if (!t) return;
  if (t->d_slots) (void)hipFree(t->d_slots);
  if (t->d_merged) (void)hipFree(t->d_merged);
  if (t->d_oslots) (void)hipFree(t->d_oslots);
  if (t->d_oinfo) (void)hipFree(t->d_oinfo);
  if (t->d_nslots) (void)hipFree(t->d_nslots);
  if (t->d_ncodes) (void)hipFree(t->d_ncodes);
  if (t->d_ndir) (void)hipFree(t->d_ndir);
  t->ws.release();
  t->ws2.release();
  t->dd.release();
  t->stage.release();
  delete t;
} SWT_API_CATCH_VOID

// The tiled forms of the word-lane kernel: running text, or (d_rec) the unique words of the dedup path.
// cap = staged bytes per chunk (LDS footprint ~ 12 B per byte): kLaneCap for running text, less for the unique-word pass
static void launch_encode_kernel(swt_bpe_table *t, uint64_t n_tiles, const TileWorkspace &ws, const uint8_t *d_text, uint64_t n_bytes,
                                 const uint64_t *d_sent_off, const uint8_t *d_cls, const uint32_t *d_uslot, unsigned long long *d_rec,
                                 unsigned long long *d_drec, hipStream_t st, bool ordered, int cap = kLaneCap) {
  BpeView v = bpe_view(t, ordered);
  const bool narrow = !d_rec && t->d_ndir && lane_narrow(t, ordered, n_bytes);
  if (!d_rec) t->last_lane_narrow = narrow ? 1 : 0;
  if (narrow) v = BpeView{reinterpret_cast<const BpeSlot *>(t->d_nslots), reinterpret_cast<const uint32_t *>(t->d_ndir), 32u - t->narrow.bits};
  hipLaunchKernelGGL(narrow ? lane_kernel_narrow(t) : d_rec ? lane_kernel<1>(t, ordered, cap) : lane_kernel<0>(t, ordered, cap), dim3((unsigned)n_tiles), dim3(64), 0, st, d_text,
                     n_bytes, d_sent_off, ws.plan.as<uint64_t>(), d_cls, v.slots, v.sh, v.merged, ws.scratch.as<uint32_t>(),
                     ws.sent_local.as<uint32_t>(), ws.tile_tok.as<uint32_t>(), d_uslot, d_rec, d_drec, DirectOut{nullptr, nullptr, 0});
}

// Tiles per wave of the running-text form: ONE.  Longer spans were measured and lost (profiles/lane_spans.txt: K = 2 costs the
// kernel +5 %, K = 4 -- every wave of S85k resident from the start -- +10 %, K = 8 +38 %), so SWT_OPT_LANE_SPAN stays what it is
// in the header: a knob for tests and sweeps.  Why they lost is not what that file says ("the price of the dispatcher refilling a
// CU"): the residency curve (profiles/lane_taper.txt section 1) shows 23 - 24 waves per CU of the 24 that fit from 2 us to the
// last begin -- the dispatcher refills a slot as fast as it empties -- and nine tenths of the empty slot-time in the DRAIN behind
// the last begin, which lasts as long as the longest life among the waves begun last (45 us at K = 1: the two-chunk tiles).
// A span makes every life K times as long and the drain with it.  The taper below goes the other way.
static uint32_t lane_span(const swt_bpe_table *t) { return t->opt_lane_span ? (uint32_t)t->opt_lane_span : 1u; }

// Wave slots of the device for the running-text kernel this table gets: CUs x resident workgroups per CU, asked once per handle.
static uint64_t lane_slots(swt_bpe_table *t, bool ordered, bool narrow, bool dropout) {
  if (t->opt_lane_slots) return (uint64_t)t->opt_lane_slots;
  uint64_t &slots = t->lane_slots[dropout ? 3 : narrow ? 2 : ordered ? 1 : 0];
  if (!slots) {
    int per_cu = 0;
    const hipError_t e = dropout ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, lane_kernel_dropout<0>(t), 64, 0)
                                 : hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, narrow ? lane_kernel_narrow(t) : lane_kernel<0>(t, ordered), 64, 0);
    if (e != hipSuccess || per_cu < 1) {
      (void)hipGetLastError();
      per_cu = 24;  // what the stamps show resident on gfx950
    }
    slots = (uint64_t)device_cus() * (uint64_t)per_cu;
  }
  return slots;
}

// Where the tiles of a running-text call begin.  A span K > 1 (SWT_OPT_LANE_SPAN) keeps its K x kLaneTile tiles of one size; the
// library's own geometry tapers: tiles of kLaneTile bytes while the bytes still to be handed out would fill c x slots such tiles,
// then 256, 192 and 128 bytes by the same rule (tilemap_taper), so that the waves started last have short lives.  A short tile
// is dear (a wave's life is ~12 us + 0.047 us per byte), so the taper is short: c = 3/8 and no tile under 192 bytes unless
// SWT_OPT_LANE_TAPER says otherwise (profiles/lane_taper.txt section 2: c = 1 down to 128 bytes LOSES 6 us to tiles of one size).
// dropout: the call runs the dropout form, a wide kernel with wave slots of its own.
static TileMap lane_map(swt_bpe_table *t, uint64_t n_bytes, bool ordered, bool dropout = false) {
  const uint32_t span = lane_span(t);
  const bool wide = dropout || !lane_narrow_tiles(t, ordered, n_bytes);
  const uint32_t tile = wide ? (uint32_t)kLaneTile : (uint32_t)kNarrowTile;
  const int v = t->opt_lane_taper ? t->opt_lane_taper : wide ? kTaperDefault : kNarrowTaperDefault;
  if (span > 1 || v == 1 || tile <= 256) return tilemap_uniform(n_bytes, tile * span);
  const uint64_t slots = lane_slots(t, ordered, !dropout && lane_narrow(t, ordered, n_bytes), dropout);
  // The floor of the library's own choice: a text under two chip-fulls of full tiles keeps tiles of one size (2.5 MB measured
  // 2.2 us slower tapered, profiles/lane_taper.txt section 3).  An explicit SWT_OPT_LANE_TAPER tapers whatever the size.
  // The narrow kernel's tiles taper wherever the library's own choice runs it, from one chip-full of kLaneTile-byte tiles (its
  // floor, lane_narrow): tapered it gains 6 - 10 us on the parent at every size from 2.5 to 7 MB, in tiles of one size it lost 5 us
  // at 5.6 MB (profiles/lane_narrow.txt section 5).  Below that floor (SWT_OPT_LANE_NARROW = 2) its tiles are of one size.
  const uint64_t taper_floor = wide ? 2ull * (uint64_t)tile * slots : (uint64_t)kLaneTile * lane_slots(t, false, false);
  if (!t->opt_lane_taper && n_bytes < taper_floor) return tilemap_uniform(n_bytes, tile);
  return tilemap_taper(n_bytes, slots, (uint32_t)(v & ~256), wide ? kTaperSizes : kNarrowTaperSizes, (v & 256) ? 3 : 4);
}

// diagnostics (not part of include/swt.h): the tile map a running-text call of n_bytes would get under the handle's options --
// out[0] = tiles, then per segment the first byte, the first tile and the tile size (zeros for a segment that is not there)
int swt_debug_bpe_tile_map(swt_bpe_table *t, uint64_t n_bytes, uint64_t *out) try {
  if (!t || !out) return fail(SWT_ERR_INVALID, "null argument");
  int rc = bpe_upload(t);
  if (rc) return rc;
  const TileMap m = lane_map(t, n_bytes, false);
  out[0] = m.n_tiles;
  for (int k = 0; k < kTileMapSegs; k++) {
    const bool there = k < (int)m.n_segs;
    out[1 + 3 * k] = there ? m.first_byte[k] : 0;
    out[2 + 3 * k] = there ? m.first_tile[k] : 0;
    out[3 + 3 * k] = there ? m.tile_bytes[k] : 0;
  }
  return SWT_OK;
} SWT_API_CATCH

static int bpe_encode_direct(swt_bpe_table *t, TileWorkspace &ws, const uint8_t *d_text, uint64_t n_bytes, const uint64_t *d_sent_off,
                             uint64_t n_sent, uint32_t *d_out_ids, uint64_t *d_out_off, uint64_t *d_n_tokens, const uint8_t *d_cls,
                             hipStream_t st, bool ordered, const DropDraw *drop = nullptr) {
  // plan, scan and gather see a span as one tile of K * kLaneTile bytes (plan[j] of that size IS plan[j * K] of the tiles), and so
  // does the kernel: its chunk loop walks the span kLaneCap bytes at a time.  None of them learns a tile's size: the map goes to
  // the plan and everything behind it reads plan[t] and plan[t + 1].
  const TileMap map = n_bytes <= kDirectBytes && n_sent <= kDirectSents ? tilemap_uniform(n_bytes, kLaneTile) : lane_map(t, n_bytes, ordered, drop != nullptr);
  const uint64_t n_tiles = map.n_tiles;
  if (n_tiles > 0x7FFFFFFFull)
    return fail(SWT_ERR_UNSUPPORTED, "text too large for one call (%llu bytes)", (unsigned long long)n_bytes);
  int rc;
  if (n_bytes <= kDirectBytes && n_sent <= kDirectSents) {
    // a sentence or a few: one workgroup, one launch, the caller's arrays written by the kernel (DirectOut)
    if ((rc = ws.reserve(64, 0, 1))) return rc;
    const BpeView v = bpe_view(t, ordered);
    if (drop)
      hipLaunchKernelGGL(lane_kernel_dropout<2>(t), dim3(1), dim3(64), 0, st, d_text, n_bytes, d_sent_off, (const uint64_t *)nullptr, d_cls, v.slots,
                         v.sh, v.merged, d_out_ids, ws.sent_local.as<uint32_t>(), ws.tile_tok.as<uint32_t>(), (const uint32_t *)nullptr,
                         (unsigned long long *)nullptr, (unsigned long long *)nullptr, DirectDrop{{d_out_off, d_n_tokens, n_sent}, *drop});
    else
      hipLaunchKernelGGL(lane_kernel<2>(t, ordered), dim3(1), dim3(64), 0, st, d_text, n_bytes, d_sent_off, (const uint64_t *)nullptr, d_cls, v.slots,
                         v.sh, v.merged, d_out_ids, ws.sent_local.as<uint32_t>(), ws.tile_tok.as<uint32_t>(), (const uint32_t *)nullptr,
                         (unsigned long long *)nullptr, (unsigned long long *)nullptr, DirectOut{d_out_off, d_n_tokens, n_sent});
    SWT_HIP(hipGetLastError());
    return SWT_OK;
  }
  if ((rc = ws.reserve(n_bytes, n_sent, n_tiles))) return rc;
  prof_begin(st, 2);
  launch_plan(d_sent_off, n_sent, map, ws.plan.as<uint64_t>(), st);
  prof_begin(st);
  if (drop) {
    const BpeView v = bpe_view(t, false);
    hipLaunchKernelGGL(lane_kernel_dropout<0>(t), dim3((unsigned)n_tiles), dim3(64), 0, st, d_text, n_bytes, d_sent_off, ws.plan.as<uint64_t>(), d_cls,
                       v.slots, v.sh, v.merged, ws.scratch.as<uint32_t>(), ws.sent_local.as<uint32_t>(), ws.tile_tok.as<uint32_t>(),
                       (const uint32_t *)nullptr, (unsigned long long *)nullptr, (unsigned long long *)nullptr, DirectDrop{{nullptr, nullptr, 0}, *drop});
  } else
    launch_encode_kernel(t, n_tiles, ws, d_text, n_bytes, d_sent_off, d_cls, nullptr, nullptr, nullptr, st, ordered);
  prof_end(st);
  launch_scan_gather(d_sent_off, n_sent, n_tiles, ws, d_out_ids, d_out_off, d_n_tokens, st);
  prof_end(st, 2);
  SWT_HIP(hipGetLastError());
  return SWT_OK;
}

// The dedup path (swt_dedup.h): eight launches, no host round trip -- the number of unique words stays on the device, so
// the unique-word encode has a fixed number of workgroups and its tile size follows on the device (ureg_kernel writes its plan).
// Returns 1 when the batch is too large for the 32-bit fields of this path (the caller takes the direct path).
constexpr uint64_t kUMaxTiles = 8192;  // its launch size: 256 CUs x 32 single-wave workgroups
static int bpe_encode_dedup(swt_bpe_table *t, const uint8_t *d_text, uint64_t n_bytes, const uint64_t *d_sent_off, uint64_t n_sent,
                            uint32_t *d_out_ids, uint64_t *d_out_off, uint64_t *d_n_tokens, const uint8_t *d_cls, hipStream_t st,
                            bool ordered) {
  int rc;
  // tile of the unique-word pass (chunk = 2 such tiles): the kernel wants a batch of words per tile, so 256 bytes unless
  // SWT_OPT_UNIQUE_TILE says otherwise (S85k-lex: 64 -> 0.182, 128 -> 0.174, 256 -> 0.168 ms per call)
  const int ut = t->opt_unique_tile;
  const uint32_t tile2 = (ut == 64 || ut == 128) ? (uint32_t)ut : 256u;
  uint64_t n_tiles2 = tile_count(n_bytes, tile2);  // the unique words together are no longer than the text
  if (n_tiles2 > kUMaxTiles) n_tiles2 = kUMaxTiles;
  if (n_bytes > kDedupMaxBytes) return 1;
  if ((rc = t->ws2.reserve(n_bytes, n_bytes / 2 + 2, n_tiles2))) return rc;
  prof_begin(st, 2);
  if ((rc = dedup_front(t->dd, t->ws, d_text, n_bytes, d_sent_off, n_sent, d_cls, kDedupBpe, st, t->ws2.plan.as<uint64_t>(), n_tiles2, tile2)))
    return rc;
  // encode the unique words once (raw-word mode: each one is a "sentence"); their token runs stay in ws2.scratch and
  // phase F of the kernel leaves count | place in rec[slot]
  prof_begin(st);
  launch_encode_kernel(t, n_tiles2, t->ws2, t->dd.utext.as<uint8_t>(), n_bytes, t->dd.uoff.as<uint64_t>(), nullptr,
                       t->dd.uslot.as<uint32_t>(), t->dd.rec_ptr(), t->dd.drec_ptr(), st, ordered, (int)(2 * tile2));
  prof_end(st);
  rc = dedup_back(t->dd, t->ws, d_sent_off, n_sent, n_bytes, t->ws2.scratch.as<uint32_t>(), kDedupBpe, nullptr, d_out_ids, d_out_off,
                  d_n_tokens, st);
  prof_end(st, 2);
  return rc;
}

}  // extern "C"

// The three entry points, for both orders.  A call that came through swt_bpe_encode_naive* on a table that is not
// order-equivalent takes the ordered form of the kernel (bpe_ordered); every other call launches exactly what it launched before.
static bool bpe_ordered(const swt_bpe_table *t) { return t && !t->order_equivalent; }

static int bpe_encode_dev(swt_bpe_table *t, const uint8_t *d_text, uint64_t n_bytes, const uint64_t *d_sent_off,
                          uint64_t n_sent, uint32_t *d_out_ids, uint64_t *d_out_off, uint64_t *d_n_tokens, uint32_t flags,
                          void *stream, bool ordered, const DropDraw *drop = nullptr) {
  if (!t || !d_sent_off || !d_out_off || !d_n_tokens || (n_bytes && (!d_text || !d_out_ids)))
    return fail(SWT_ERR_INVALID, "null argument");
  int rc = bpe_upload(t);
  if (rc) return rc;
  if (ordered && (rc = bpe_upload_ordered(t))) return rc;
  hipStream_t st = (hipStream_t)stream;
  const uint8_t *d_cls = nullptr;
  if ((rc = device_class_table(&d_cls))) return rc;
  if (n_sent == 0) {
    SWT_HIP(hipMemsetAsync(d_out_off, 0, 8, st));
    SWT_HIP(hipMemsetAsync(d_n_tokens, 0, 8, st));
    return SWT_OK;
  }
  const bool raw = (flags & SWT_BPE_RAW_WORDS) != 0;
  // debug knob 1: bit 0 = never dedup, bit 1 = dedup whatever the batch size (tests)
  // (a dropout call never dedups: two occurrences of a word may come out differently)
  if (!drop && !raw && !(flags & SWT_BPE_NO_DEDUP) && t->dd.opt_mode != 1 &&
      (t->dd.opt_mode == 2 || (n_bytes >= kDedupMinBytes && t->dd.pays(n_bytes)))) {
    rc = bpe_encode_dedup(t, d_text, n_bytes, d_sent_off, n_sent, d_out_ids, d_out_off, d_n_tokens, d_cls, st, ordered);
    if (rc == 0 && t->dd.opt_mode == 0) t->dd.note(n_bytes, st);
    if (rc <= 0) return rc;  // done, or a real error
  }
  // raw-word mode: no classes, so nothing splits and nothing is dropped
  return bpe_encode_direct(t, t->ws, d_text, n_bytes, d_sent_off, n_sent, d_out_ids, d_out_off, d_n_tokens, raw ? nullptr : d_cls, st, ordered, drop);
}

// What the host-call layer (swt_tile.h) needs to know of this encoder, in either order.
// drop: the draws of a dropout call (copied: the encoder may outlive the caller's), null for every other.
static HostEncoder bpe_host(swt_bpe_table *t, uint32_t flags, bool ordered, const DropDraw *drop = nullptr) {
  const bool dropout = drop != nullptr;
  const DropDraw dd = drop ? *drop : DropDraw{};
  return HostEncoder{[t] { return bpe_upload(t); },
                     [t, flags, ordered, dropout, dd](const uint8_t *d_text, uint64_t n_bytes, const uint64_t *d_off, uint64_t n_sent, uint32_t *d_ids,
                                                      uint64_t *d_out_off, uint8_t *, uint64_t *d_n_tokens) {
                       return bpe_encode_dev(t, d_text, n_bytes, d_off, n_sent, d_ids, d_out_off, d_n_tokens, flags, nullptr, ordered, dropout ? &dd : nullptr);
                     },
                     kDirectBytes, kDirectSents, false};
}
static int bpe_encode_host(swt_bpe_table *t, const uint8_t *text, const uint64_t *sent_off, uint64_t n_sent, uint32_t *out_ids,
                           uint64_t out_cap, uint64_t *out_off, uint64_t *n_tokens, uint32_t flags, bool ordered, const DropDraw *drop = nullptr) {
  if (!t) return fail(SWT_ERR_INVALID, "null argument");
  return host_encode(t->stage, bpe_host(t, flags, ordered, drop), text, sent_off, n_sent, out_ids, out_cap, out_off, nullptr, n_tokens);
}
static int bpe_encode_joined(swt_bpe_table *t, const uint8_t *joined, uint64_t n_joined, uint64_t n_sent, uint32_t *out_ids, uint64_t out_cap,
                             uint64_t *out_off, uint64_t *n_tokens, uint8_t *need_host, uint32_t flags, bool ordered) {
  if (!t) return fail(SWT_ERR_INVALID, "null argument");
  return host_encode_joined(t->stage, bpe_host(t, flags, ordered), joined, n_joined, n_sent, out_ids, out_cap, out_off, nullptr, n_tokens, need_host);
}

extern "C" {

int swt_bpe_encode_dev(swt_bpe_table *t, const uint8_t *d_text, uint64_t n_bytes, const uint64_t *d_sent_off,
                       uint64_t n_sent, uint32_t *d_out_ids, uint64_t *d_out_off, uint64_t *d_n_tokens, uint32_t flags,
                       void *stream) try {
  return bpe_encode_dev(t, d_text, n_bytes, d_sent_off, n_sent, d_out_ids, d_out_off, d_n_tokens, flags, stream, false);
} SWT_API_CATCH

int swt_bpe_encode(swt_bpe_table *t, const uint8_t *text, const uint64_t *sent_off, uint64_t n_sent, uint32_t *out_ids,
                   uint64_t out_cap, uint64_t *out_off, uint64_t *n_tokens, uint32_t flags) try {
  return bpe_encode_host(t, text, sent_off, n_sent, out_ids, out_cap, out_off, n_tokens, flags, false);
} SWT_API_CATCH

int swt_bpe_encode_joined(swt_bpe_table *t, const uint8_t *joined, uint64_t n_joined, uint64_t n_sent, uint32_t *out_ids, uint64_t out_cap,
                          uint64_t *out_off, uint64_t *n_tokens, uint8_t *need_host, uint32_t flags) try {
  return bpe_encode_joined(t, joined, n_joined, n_sent, out_ids, out_cap, out_off, n_tokens, need_host, flags, false);
} SWT_API_CATCH

// BPE-dropout (include/swt.h): the encode above with every candidate merge dropped by its Philox draw.  The draws of a call, or
// the refusal of a threshold above 2^32.
static int bpe_drop_draw(uint64_t drop_below, uint64_t seed, uint32_t epoch, DropDraw &out) {
  if (drop_below > (1ull << 32)) return fail(SWT_ERR_INVALID, "drop_below is above 2^32");
  out = DropDraw{drop_below, (uint32_t)seed, (uint32_t)(seed >> 32), epoch};
  return SWT_OK;
}

int swt_bpe_encode_dropout_dev(swt_bpe_table *t, const uint8_t *d_text, uint64_t n_bytes, const uint64_t *d_sent_off,
                               uint64_t n_sent, uint32_t *d_out_ids, uint64_t *d_out_off, uint64_t *d_n_tokens, uint32_t flags,
                               uint64_t drop_below, uint64_t seed, uint32_t epoch, void *stream) try {
  DropDraw dd;
  if (int rc = bpe_drop_draw(drop_below, seed, epoch, dd)) return rc;
  return bpe_encode_dev(t, d_text, n_bytes, d_sent_off, n_sent, d_out_ids, d_out_off, d_n_tokens, flags, stream, false, &dd);
} SWT_API_CATCH

int swt_bpe_encode_dropout(swt_bpe_table *t, const uint8_t *text, const uint64_t *sent_off, uint64_t n_sent, uint32_t *out_ids,
                           uint64_t out_cap, uint64_t *out_off, uint64_t *n_tokens, uint32_t flags, uint64_t drop_below, uint64_t seed,
                           uint32_t epoch) try {
  DropDraw dd;
  if (int rc = bpe_drop_draw(drop_below, seed, epoch, dd)) return rc;
  return bpe_encode_host(t, text, sent_off, n_sent, out_ids, out_cap, out_off, n_tokens, flags, false, &dd);
} SWT_API_CATCH

// NaiveBPE.tokenize (bpe.py:136-158: the split of utils.py:26-29, then encode_word, bpe.py:114-134, per word) for a batch: the
// merges applied in list order.  Same arguments, ids and flags as the three above.
int swt_bpe_encode_naive_dev(swt_bpe_table *t, const uint8_t *d_text, uint64_t n_bytes, const uint64_t *d_sent_off,
                             uint64_t n_sent, uint32_t *d_out_ids, uint64_t *d_out_off, uint64_t *d_n_tokens, uint32_t flags,
                             void *stream) try {
  return bpe_encode_dev(t, d_text, n_bytes, d_sent_off, n_sent, d_out_ids, d_out_off, d_n_tokens, flags, stream, bpe_ordered(t));
} SWT_API_CATCH

int swt_bpe_encode_naive(swt_bpe_table *t, const uint8_t *text, const uint64_t *sent_off, uint64_t n_sent, uint32_t *out_ids,
                         uint64_t out_cap, uint64_t *out_off, uint64_t *n_tokens, uint32_t flags) try {
  return bpe_encode_host(t, text, sent_off, n_sent, out_ids, out_cap, out_off, n_tokens, flags, bpe_ordered(t));
} SWT_API_CATCH

int swt_bpe_encode_naive_joined(swt_bpe_table *t, const uint8_t *joined, uint64_t n_joined, uint64_t n_sent, uint32_t *out_ids,
                                uint64_t out_cap, uint64_t *out_off, uint64_t *n_tokens, uint8_t *need_host, uint32_t flags) try {
  return bpe_encode_joined(t, joined, n_joined, n_sent, out_ids, out_cap, out_off, n_tokens, need_host, flags, bpe_ordered(t));
} SWT_API_CATCH

}  // extern "C"
