// swt_wp.hip -- FastWP (end-to-end LinMaxMatch WordPiece) on gfx950.
//
// Replaces:
//   TrieNode / WPTrie_E2E.insert / precompute   /root/reference/source/utils.py:44-139   (host, then flattened)
//   FastWP.tokenize / matchloop / iswdbndry / ispunc   /root/reference/source/wordpiece.py:233-316
//   the NaiveWP.encode_word("##") corner               /root/reference/source/wordpiece.py:260-261, 132-159
//
// Flattened trie in HBM (L2-resident: ~1.6 MB at 20k vocab):
//   edges  open-addressing hash of packed 64-bit entries  node:21 | code point:21 | child:21  (one 8-byte load
//          per probe; key = the upper 42 bits)
//   nodes  16 bytes each {failure link, pop offset, pop count, flags}
//   pops   token ids of every failure_pops list, concatenated
// Node ids: 0 = root, 1 = root_p (detached, childless), 2.. in creation order; root_sharp is the node of "##".
#include <cstring>
#include <type_traits>
#include <unordered_map>

#include "swt_dedup.h"
#include "swt_philox.h"
#include "swt_tile.h"
#include "swt_words.h"

namespace swt {

struct alignas(16) WpNode {
  int32_t link;      // failure_link, -1 = None
  uint32_t pop_off;  // into pops[]
  uint32_t pop_cnt;
  uint32_t flags;    // bit0 is_end
};

constexpr uint32_t kWpRoot = 0, kWpRootP = 1;
constexpr uint32_t kNodeBits = 21, kMaxNodes = (1u << kNodeBits) - 2;
constexpr uint64_t kEdgeEmpty = ~0ull;
constexpr uint8_t kPySpace = 1, kPyAlnum = 2;

__host__ __device__ inline uint64_t edge_key(uint32_t node, uint32_t cp) { return ((uint64_t)node << 21) | cp; }

struct WpDev {
  const uint64_t *edges;
  uint32_t edge_bits;
  const WpNode *nodes;
  const uint32_t *pops;
  uint32_t root_sharp;
  uint32_t unk_id;        // "['UNK']"
  uint32_t corner_id;     // single id emitted for the '##' corner (token, "[UNK]" or the marker)
  uint32_t corner_nonterm;  // 1: the reference never returns from NaiveWP.encode_word("##")
  uint32_t empty_status;    // status of an empty sentence: s = " " raises IndexError iff the root has a ' ' edge
};

__device__ __forceinline__ int32_t edge_lookup(const WpDev &T, uint32_t node, uint32_t cp) {
  const uint64_t key = edge_key(node, cp);
  const uint32_t mask = (1u << T.edge_bits) - 1u;
  uint32_t h = hash_slot(key, T.edge_bits);
  for (;;) {
    const uint64_t e = T.edges[h];
    if ((e >> 21) == key) return (int32_t)(e & 0x1FFFFFu);
    if (e == kEdgeEmpty) return -1;
    h = (h + 1) & mask;
  }
}

// Character source of the walkers: UTF-8 bytes (LDS-staged chunk or global memory), decoded on the fly; classes of
// U+0000..U+03FF from the LDS copy when there is one.  [b, e) is the sentence; positions are byte offsets.
struct TxtSrc {
  const uint8_t *txt;
  const uint8_t *cls_lo;   // may be null
  const uint8_t *cls_tab;
  __device__ __forceinline__ void load(uint64_t p, uint64_t e, uint32_t &cp, uint32_t &cc, uint32_t &len) const {
    const uint8_t b = txt[p];
    int n = utf8_len(b);
    if (p + n > e) n = (int)(e - p);
    cp = b;
    if (b >= 0x80 && n > 1) {
      cp = b & (0xFF >> (n + 1));
      for (int i = 1; i < n; i++) cp = (cp << 6) | (txt[p + i] & 0x3F);
    }
    const uint8_t c = (cls_lo && cp < 1024u) ? cls_lo[cp] : (cp < kNumCodePoints ? cls_tab[cp] : (uint8_t)0);
    cc = (c >> 2) & 3;
    uint64_t q = p + n;
    while (q < e && utf8_is_cont(txt[q])) q++;  // stray continuation bytes ride with the previous char
    len = (uint32_t)(q - p);
  }
  // the bytes of the code point at p as load() counts them, without its class (the span pass)
  __device__ __forceinline__ uint32_t step(uint64_t p, uint64_t e) const {
    uint64_t q = p + utf8_len(txt[p]);
    if (q > e) q = e;
    while (q < e && utf8_is_cont(txt[q])) q++;
    return (uint32_t)(q - p);
  }
};

// ---- token spans out of the walk (swt_wp_encode_spans) ---------------------------------------------------------
// A segment of FastWP.tokenize starts at i0; matchloop leaves it at i1.  Its tokens cover a prefix of s[i0:i1], one after the
// other: the first covers len(token) code points, every later one (it begins with '##') len(token) - 2.  The "['UNK']" of an
// invalid segment covers (i0, b) with b the first iswdbndry position at or after i1; the '##' corner covers (i0, i0 + 2).  The
// word index of a token numbers the segments of its sentence that emit at least one token.
// segment() hands what it knows to a sink of this shape; WpNoSpans is the ids-only form and leaves no instruction behind.
constexpr int kSegValid = 0, kSegUnk = 1, kSegCorner = 2;
struct WpNoSpans {
  static constexpr bool on = false;
};
constexpr uint32_t kWpLenCont = 0x80000000u;  // length-table entry: the token begins with '##'
struct WpSpanTab {
  const uint32_t *len;  // code points of every vocabulary token, kWpLenCont on the '##' ones
  uint32_t n_vocab;
  uint32_t unit_cp;     // SWT_SPAN_CODEPOINTS
};
// Where the spans of ONE walker go.  The walker's positions are byte offsets in its text source; b0 is its sentence's first byte.
// sp runs parallel to the ids the segment stored (sp[k] belongs to out[k]).  The word index is either written next to the ids
// (wd: the one-lane walk in global memory, which counts as it goes) or left as a bit per first token slot in an LDS mask (emit:
// the kernel takes popcounts from the sentence start afterwards).  seq: the sink is carried from segment to segment of a
// sentence and advances itself; otherwise it serves one segment and cp0 is given.
struct WpSpanSink {
  static constexpr bool on = true;
  WpSpanTab tab;
  uint32_t *sp;    // two words per token
  uint32_t *wd;
  unsigned long long *emit;
  uint32_t slot;   // bit of sp[0] in emit
  uint64_t b0;
  uint32_t cp0;    // code points between b0 and the segment's start
  uint32_t nw;     // token-bearing segments so far
  bool seq;
  template <class Src>
  __device__ __forceinline__ void put(const Src &src, uint64_t i0, uint64_t bnd, uint64_t next, uint64_t e, int kind,
                                      const uint32_t *ids, uint32_t n) {
    uint64_t q = i0;
    uint32_t c = 0;
    const auto walk_cps = [&](uint32_t want) {  // `want` code points on from q, never past the sentence
      for (uint32_t j = 0; j < want && q < e; j++) { q += src.step(q, e); c++; }
    };
    const auto walk_to = [&](uint64_t stop) {
      while (q < stop && q < e) { q += src.step(q, e); c++; }
    };
    const auto put_span = [&](uint32_t k, uint64_t q0, uint32_t c0) {
      sp[2 * k] = tab.unit_cp ? cp0 + c0 : (uint32_t)(q0 - b0);
      sp[2 * k + 1] = tab.unit_cp ? cp0 + c : (uint32_t)(q - b0);
    };
    if (n) {
      if (kind == kSegUnk) {
        walk_to(bnd);
        put_span(0, i0, 0);
      } else if (kind == kSegCorner) {
        walk_cps(2);
        put_span(0, i0, 0);
      } else {
        for (uint32_t k = 0; k < n; k++) {
          const uint32_t id = ids[k];
          const uint32_t ent = id < tab.n_vocab ? tab.len[id] : 0u;
          uint32_t L = ent & 0xFFFFFFu;
          if (k && (ent & kWpLenCont)) L = L >= 2 ? L - 2 : 0;
          const uint64_t q0 = q;
          const uint32_t c0 = c;
          walk_cps(L);
          put_span(k, q0, c0);
        }
      }
      if (emit) atomicOr(&emit[slot >> 6], 1ull << (slot & 63));
      if (wd)
        for (uint32_t k = 0; k < n; k++) wd[k] = nw;
    }
    if (!seq) return;
    if (tab.unit_cp) {
      walk_to(next);
      cp0 += c;
    }
    sp += 2 * n;
    slot += n;
    if (wd) wd += n;
    nw += n ? 1u : 0u;
  }
};

// State of a walk through one sentence occupying bytes [b, e): i == e is the appended space (wordpiece.py:248),
// i == e + 1 is len(s).
template <class Src>
struct WpWalk {
  const Src &src;
  const WpDev &T;
  uint64_t e, i;
  uint32_t cp, cc, len;
  bool prev_punc;  // ispunc(s[i-1]); never across a sentence start
  __device__ __forceinline__ WpWalk(const Src &s, const WpDev &t, uint64_t start, uint64_t end, bool pp)
      : src(s), T(t), e(end), i(start), cp(' '), cc(kPySpace), len(1), prev_punc(pp) {
    if (i < e) src.load(i, e, cp, cc, len);
  }
  __device__ __forceinline__ void adv() {
    prev_punc = (cc & (kPySpace | kPyAlnum)) == 0;
    if (i < e) { i += len; if (i > e) i = e; }
    else i = e + 1;
    if (i < e) src.load(i, e, cp, cc, len);
    else { cp = ' '; cc = kPySpace; len = 1; }
  }
  __device__ __forceinline__ bool bndry() const {  // wordpiece.py:285
    return prev_punc || (cc & kPySpace) || (cc & (kPySpace | kPyAlnum)) == 0;
  }
  // One iteration of the loop at wordpiece.py:251-269: match a segment from i, emit its tokens to out[0..) (at most
  // `room` are stored), move i to the start of the next segment.  Returns the token count; status != OK aborts.
  // sp: where the tokens' spans go (WpSpanSink), or nowhere (WpNoSpans).
  template <class Out, class Sp>
  __device__ __forceinline__ uint32_t segment(Out out, uint32_t room, int &status, Sp &sp) {
    const uint64_t seg_i = i;
    int kind = kSegValid;
    uint32_t nt = 0;
    uint32_t node = kWpRoot;
    bool stop = false;
    while (i <= e) {  // matchloop, wordpiece.py:291-316
      int32_t child = edge_lookup(T, node, cp);
      while (child < 0) {
        const WpNode nd = T.nodes[node];
        if (nd.link < 0) { stop = true; break; }
        for (uint32_t k = 0; k < nd.pop_cnt; k++) {
          if (nt < room) out[nt] = T.pops[nd.pop_off + k];
          nt++;
        }
        node = (uint32_t)nd.link;
        child = edge_lookup(T, node, cp);
      }
      if (stop) break;
      node = (uint32_t)child;
      adv();
    }
    if (i > e) { status = SWT_WP_INDEXERROR; return 0; }  // iswdbndry indexes seq[len(seq)] (wordpiece.py:285)
    const bool root_like = node == kWpRoot || node == T.root_sharp || node == kWpRootP;
    if (!bndry() || !root_like) {  // wordpiece.py:255-257: the segment's tokens are replaced by the one literal
      for (uint32_t k = 1; k < nt && k < room; k++) out[k] = kInvalidTok;
      if (room) out[0] = T.unk_id;
      nt = 1;
      kind = kSegUnk;
    } else if (node == T.root_sharp && nt == 0) {  // wordpiece.py:260-261
      if (T.corner_nonterm) { status = SWT_WP_NONTERMINATING; return 0; }
      if (room) out[0] = T.corner_id;
      nt = 1;
      kind = kSegCorner;
    }
    while (i <= e && !bndry()) adv();          // wordpiece.py:265-266
    const uint64_t bnd_i = i;
    while (i <= e && (cc & kPySpace)) adv();   // wordpiece.py:268-269
    if (i == seg_i) { status = SWT_WP_NONTERMINATING; return 0; }  // same state again: the reference spins
    if constexpr (Sp::on) sp.put(src, seg_i, bnd_i, i, e, kind, &out[0], nt < room ? nt : room);
    return nt;
  }
};

// FastWP.tokenize on one whole sentence, segment after segment (the sequential form: sentences the parallel form
// cannot certify, and sentences longer than a chunk).  out[k] receives the k-th id.  Returns the token count
// (0 when status != OK).  wordpiece.py:248-270.
template <class Src, class Out, class Sp>
__device__ uint32_t wp_sentence(const Src &src, uint64_t b, uint64_t e, Out out, const WpDev &T, int &status, Sp &sp) {
  WpWalk<Src> w(src, T, b, e, false);
  uint32_t nt = 0;
  status = SWT_WP_OK;
  while (w.i <= e) {  // wordpiece.py:251
    nt += w.segment(out + nt, 0xFFFFFFFFu, status, sp);
    if (status != SWT_WP_OK) return 0;
  }
  return nt;
}

constexpr int kWpTile = 512;    // bytes of sentence starts per tile
constexpr int kWpCap = 1024;    // staged bytes per chunk
constexpr int kWpBlocks = kWpCap / 64;
constexpr int kWpClsLds = 1024;
constexpr uint64_t kWpDirectBytes = 2048, kWpDirectSents = 64;  // up to here one workgroup and one launch do the whole call
constexpr uint32_t kWpUTile = 256;       // smallest tile of the encode over the unique chunks (dedup path)
constexpr uint64_t kWpUMaxTiles = 8192;  // its fixed launch size

// ======================================================================================================================
// The tile skeleton of the two WordPiece kernels (wp_encode_kernel, wp_naive_kernel): one 64-lane wavefront per tile
// (workgroup = one wave), the tile's span walked in chunks of kWpCap staged bytes that end at sentence starts.  Written once:
//   wp_tile_begin   the tile's sentences and span, the LDS copy of the first 1,024 classes
//   wp_stage        A: the chunk's bytes into LDS
//   wp_mark         sentence starts -> sbits; where the chunk ends (false: one sentence is longer than the staged bytes)
//   wp_giant        that sentence, by one lane in global memory with the kernel's one-lane walker
//   wp_emit         E/F: ballot compaction of tok[] to the tile's output run, per-sentence offsets
//   wp_tile_end     the tile's total (or the caller's closing offset and count, DirectOut)
// B (classes -> candidates), C (one lane per candidate or word) and D (per-sentence status) are the kernels' own.
struct WpGiant { uint64_t end; uint32_t ntok; uint32_t nsent; };

// What both kernels keep in LDS; each puts its own masks behind it.  txt and cls_lo are moved 16 bytes at a time: they stand at
// multiples of 16 here, and the structs that begin with this one are aligned to 16.
struct WpTileLds {
  uint8_t txt[kWpCap + 16];
  uint8_t cls_lo[kWpClsLds];
  uint32_t tok[kWpCap];                      // per byte position: a token id or kInvalidTok
  uint16_t cand[kWpCap];                     // segment-start candidates / word starts, in position order
  unsigned long long sbits[kWpBlocks + 1];   // sentence-start bit per byte
  unsigned long long vmask[kWpBlocks + 1];
  WpGiant giant;
  uint32_t blkpre[kWpBlocks + 1];
};
static_assert((kWpCap + 16) % 16 == 0, "cls_lo must stand at a multiple of 16");

// What a wave carries from chunk to chunk of its tile, and what it knows about the chunk at hand.
struct WpTile {
  uint64_t s_hi;       // end of the tile's sentences
  uint64_t span_end;   // end of their bytes
  uint64_t s_next;     // first sentence whose local offset is not recorded yet
  uint64_t cb;         // first byte not encoded yet
  uint32_t *tile_out;  // the tile's run in scratch
  uint32_t run;        // tokens emitted so far
};
struct WpChunk {
  uint64_t abase;               // 16-byte aligned base of the staged bytes
  uint32_t off0, staged, nblk;  // first byte of the chunk inside the staged bytes, staged bytes, 64-byte blocks
  uint32_t ce;                  // end of the chunk: a sentence start, or staged
  bool last;                    // the tile ends with this chunk
};
// where a tile's per-sentence results go
struct WpOut {
  uint32_t *sent_local;
  uint8_t *status;
  DirectOut direct;
  __device__ __forceinline__ void off(uint64_t s, uint32_t v) const {
    if (direct.off) direct.off[s] = v; else sent_local[s] = v;
  }
};

__device__ __forceinline__ bool wbit(const unsigned long long *m, uint32_t p) { return (m[p >> 6] >> (p & 63)) & 1ull; }

// False: the tile holds no sentence (its total is written, the wave is done).
__device__ __forceinline__ bool wp_tile_begin(WpTileLds &L, WpTile &tile, const uint64_t *__restrict__ sent_off,
                                              const uint64_t *__restrict__ plan, const uint8_t *__restrict__ cls_tab,
                                              uint32_t *__restrict__ scratch, uint32_t *__restrict__ tile_tok, const DirectOut &direct,
                                              int lane) {
  const uint64_t t = blockIdx.x;
  const uint64_t s_lo = direct.off ? 0 : plan[t];
  tile.s_hi = direct.off ? direct.n_sent : plan[t + 1];
  if (s_lo == tile.s_hi) {
    if (lane == 0) tile_tok[t] = 0;
    return false;
  }
  reinterpret_cast<uint4 *>(L.cls_lo)[lane] = reinterpret_cast<const uint4 *>(cls_tab)[lane];
  const uint64_t span_base = sent_off[s_lo];
  tile.span_end = sent_off[tile.s_hi];
  tile.tile_out = scratch + span_base;
  tile.run = 0;
  tile.s_next = s_lo;
  tile.cb = span_base;
  return true;
}

// ---- A. stage [abase, abase + staged), clear the sentence-start bits.  The caller clears its own masks and synchronises.
__device__ __forceinline__ void wp_stage(WpTileLds &L, const WpTile &tile, WpChunk &ch, const uint8_t *__restrict__ text, uint64_t n_bytes,
                                         int lane) {
  ch.abase = tile.cb & ~15ull;
  ch.off0 = (uint32_t)(tile.cb - ch.abase);
  const uint64_t avail = tile.span_end - ch.abase;
  ch.last = avail <= (uint64_t)kWpCap;
  ch.staged = ch.last ? (uint32_t)avail : (uint32_t)kWpCap;
  ch.nblk = (ch.staged + 63) >> 6;
  for (uint32_t c = lane * 16; c < ch.staged; c += 64 * 16) {
    const uint64_t g = ch.abase + c;
    if (g + 16 <= n_bytes && ((reinterpret_cast<uintptr_t>(text + g) & 15) == 0)) {
      *reinterpret_cast<uint4 *>(&L.txt[c]) = *reinterpret_cast<const uint4 *>(text + g);
    } else {
      for (int i = 0; i < 16; i++) L.txt[c + i] = (g + i < n_bytes) ? text[g + i] : (uint8_t)' ';
    }
  }
  if (lane <= kWpBlocks) L.sbits[lane] = 0ull;
}

// Sentence starts inside the staged bytes -> sbits; the chunk ends at the last one that leaves its predecessor whole (ch.ce).
// False: there is none, one sentence is longer than the LDS chunk (wp_giant).
__device__ __forceinline__ bool wp_mark(WpTileLds &L, const WpTile &tile, WpChunk &ch, const uint64_t *__restrict__ sent_off, int lane) {
  int cut = -1;
  uint32_t n_in = 0;  // sentences starting in [cb, abase + staged)
  for (uint64_t s = tile.s_next + lane; s < tile.s_hi; s += 64) {
    const uint64_t o = sent_off[s];
    if (o >= ch.abase + ch.staged) break;
    atomicOr(&L.sbits[(o - ch.abase) >> 6], 1ull << ((o - ch.abase) & 63));
    if (o > tile.cb) cut = (int)(o - ch.abase);
    n_in++;
  }
  for (int d = 32; d >= 1; d >>= 1) {
    cut = max(cut, __shfl_xor(cut, d));
    n_in += __shfl_xor(n_in, d);
  }
  __syncthreads();
  ch.ce = ch.staged;
  if (ch.last) return true;
  // does a sentence start exactly at the end of the staged bytes?  then everything staged is whole
  const uint64_t s_after = tile.s_next + n_in;
  if (s_after < tile.s_hi && sent_off[s_after] == ch.abase + ch.staged) return true;
  if (cut < 0) return false;
  ch.ce = (uint32_t)cut;
  return true;
}

// One sentence longer than the LDS chunk: lane 0 walks it in global memory (walk(b, e, out, status, s) -> token count; s: the
// sentence's index in sent_off).  The empty
// sentences that also start at cb come first and get no tokens and `empty_status`.  True: the tile ends with it.
template <class Walk>
__device__ __forceinline__ bool wp_giant(WpTileLds &L, WpTile &tile, const uint64_t *__restrict__ sent_off, const WpOut &out,
                                         uint32_t empty_status, Walk walk, int lane) {
  if (lane == 0) {
    uint64_t s = tile.s_next;
    while (s + 1 < tile.s_hi && sent_off[s + 1] <= tile.cb) s++;  // the last sentence that starts at cb
    int stt;
    const uint64_t e = sent_off[s + 1];
    const uint32_t n = walk(tile.cb, e, tile.tile_out + tile.run, stt, s);
    for (uint64_t z = tile.s_next; z <= s; z++) {
      out.off(z, tile.run);
      out.status[z] = (uint8_t)empty_status;
    }
    out.status[s] = (uint8_t)stt;
    L.giant.end = e;
    L.giant.ntok = n;
    L.giant.nsent = (uint32_t)(s - tile.s_next + 1);
  }
  __syncthreads();
  tile.s_next += L.giant.nsent;
  tile.run += L.giant.ntok;
  tile.cb = L.giant.end;
  __syncthreads();
  if (tile.cb < tile.span_end) return false;
  // trailing empty sentences at the very end of the span
  for (uint64_t z = tile.s_next + lane; z < tile.s_hi; z += 64) {
    out.off(z, tile.run);
    out.status[z] = (uint8_t)empty_status;
  }
  return true;
}

// Byte p of the chunk as phase B sees it: inside the chunk (outside counts as a space), a lead byte, its code point (a
// sequence is clipped at the chunk's end).
__device__ __forceinline__ uint32_t wp_decode(const WpTileLds &L, const WpChunk &ch, uint32_t p, bool &inr, bool &lead) {
  inr = p >= ch.off0 && p < ch.ce;
  const uint8_t b = inr ? L.txt[p] : (uint8_t)' ';
  lead = !utf8_is_cont(b);
  uint32_t cp = b;
  if (b >= 0xC0) {
    int len = utf8_len(b);
    if (p + len > ch.ce) len = (int)(ch.ce - p);
    if (len > 1) {
      cp = b & (0xFF >> (len + 1));
      for (int i = 1; i < len; i++) cp = (cp << 6) | (L.txt[p + i] & 0x3F);
    }
  }
  return cp;
}

// the start of the sentence around byte p0 of the chunk
__device__ __forceinline__ uint32_t wp_sentence_start(const WpTileLds &L, const WpChunk &ch, uint32_t p0) {
  int w = (int)(p0 >> 6);
  unsigned long long m = L.sbits[w] & ((2ull << (p0 & 63)) - 1ull);
  while (!m && w > 0) m = L.sbits[--w];
  return m ? (uint32_t)(w * 64 + 63 - __builtin_clzll(m)) : ch.off0;
}

// ---- E. compaction, F. sentence offsets.  Advances the tile; true: that was its last chunk.  extra(p, k): what else travels with
// the token at byte p of the chunk to slot k of the tile's run (the span form; WpNoExtra for ids alone).
struct WpNoExtra {
  __device__ __forceinline__ void operator()(uint32_t, uint32_t) const {}
};
template <class Extra>
__device__ __forceinline__ bool wp_emit(WpTileLds &L, WpTile &tile, const WpChunk &ch, const uint64_t *__restrict__ sent_off,
                                        const WpOut &out, int lane, Extra extra) {
  const unsigned long long lt = (1ull << lane) - 1ull;
  uint32_t total = 0;
  for (uint32_t blk = 0; blk < ch.nblk; blk++) {
    const uint32_t p = blk * 64 + lane;
    const uint32_t sv = (p >= ch.off0 && p < ch.ce) ? L.tok[p] : kInvalidTok;
    const unsigned long long m = __ballot(sv != kInvalidTok);
    if (lane == 0) { L.vmask[blk] = m; L.blkpre[blk] = total; }
    if (sv != kInvalidTok) {
      const uint32_t k = tile.run + total + __popcll(m & lt);
      tile.tile_out[k] = sv;
      extra(p, k);
    }
    total += __popcll(m);
  }
  __syncthreads();
  uint32_t mine = 0;
  for (uint64_t s = tile.s_next + lane; s < tile.s_hi; s += 64) {
    const uint64_t rel = sent_off[s] - ch.abase;
    if (rel > ch.ce || (rel == ch.ce && !ch.last)) break;
    uint32_t ex = total;
    if (rel < ch.ce && (rel >> 6) < ch.nblk) ex = L.blkpre[rel >> 6] + __popcll(L.vmask[rel >> 6] & ((1ull << (rel & 63)) - 1ull));
    out.off(s, tile.run + ex);
    mine++;
  }
  for (int d = 32; d >= 1; d >>= 1) mine += __shfl_xor(mine, d);
  tile.s_next += mine;
  tile.run += total;
  if (ch.last) return true;
  tile.cb = ch.abase + ch.ce;
  __syncthreads();
  return false;
}

__device__ __forceinline__ void wp_tile_end(const WpTile &tile, uint32_t *__restrict__ tile_tok, const DirectOut &direct, int lane) {
  if (lane != 0) return;
  if (direct.off) { direct.off[tile.s_hi] = tile.run; *direct.n_tokens = tile.run; }
  else tile_tok[blockIdx.x] = tile.run;
}

struct alignas(16) WpLds : WpTileLds {
  unsigned long long ppunc[kWpBlocks + 1];   // the char before this byte (same sentence) is punctuation-class
  unsigned long long irr[kWpBlocks + 1];     // per sentence-start position: needs the sequential walk
  static constexpr bool spans = false;
};
// The span form keeps, next to tok[]: the span of the token in each byte's slot, the code-point starts (the unit of
// SWT_SPAN_CODEPOINTS), and a bit at the slot of the first token of every segment that emitted one, with its block prefix.
struct alignas(16) WpSpanLds : WpLds {
  uint32_t sp[2 * kWpCap];  // two words per token slot
  unsigned long long lead[kWpBlocks + 1];
  unsigned long long emit[kWpBlocks + 1];
  uint32_t epre[kWpBlocks + 1];
  static constexpr bool spans = true;
};
// What the span kernel is given beyond the ids kernel's arguments: the length table, the unit, and the scratch runs (or, in the
// direct form, the caller's arrays) of spans and word indices, indexed as the ids' scratch is.
struct WpSpanArgs {
  WpSpanTab tab;
  uint32_t *sp;  // two words per token: any 4-byte aligned array of the caller will do
  uint32_t *wd;
};
struct WpNoSpanArgs {};

// set bits of m[] at positions [a, b), a <= b
__device__ __forceinline__ uint32_t wp_count(const unsigned long long *m, uint32_t a, uint32_t b) {
  uint32_t n = 0;
  for (uint32_t w = a >> 6; w <= (b >> 6); w++) {
    unsigned long long x = m[w];
    if (w == (a >> 6)) x &= ~((1ull << (a & 63)) - 1ull);
    if (w == (b >> 6)) x &= (1ull << (b & 63)) - 1ull;
    n += __popcll(x);
  }
  return n;
}

// set bits of m[] below position p (pre[w] = set bits of the words before w)
__device__ __forceinline__ uint32_t wp_rank(const unsigned long long *m, const uint32_t *pre, uint32_t p) {
  return pre[p >> 6] + __popcll(m[p >> 6] & ((1ull << (p & 63)) - 1ull));
}

// The skeleton above with these phases.  Segments of a sentence depend on each other only through where the previous one
// ended (wordpiece.py:265-269), and that is almost always the next static boundary.  So:
//   B  64 bytes per step: classes (str.isspace / str.isalnum) -> ballot masks -> the positions where a segment CAN
//      start (sentence start; a non-space char after a space; either side of a punctuation-class char)
//   C  one lane per candidate walks the trie from there (matchloop + validity + skip), writing its tokens into its own
//      territory [candidate, next candidate); it certifies itself when it ended exactly at the next candidate
//   D  a sentence with an uncertified candidate (a vocabulary entry spanning a boundary, a non-terminating or raising
//      input) is redone by one lane with the sequential walker -- exactness never rests on the speculation
// Two instantiations: wp_encode_kernel<WpLds>, the ids alone -- its arguments, resources and instructions are those of the kernel
// before there was a second one -- and wp_encode_kernel<WpSpanLds, WpSpanArgs>, every token with its span and word index (one more
// argument).  In the span form every one of the four ways a token is made carries them:
//   C      the lane's sink writes sp[] next to its tok[] and marks its candidate in emit when it stored a token
//   D      the redone sentence's bits of emit are cleared and set again at the slots its segments' first tokens went to
//   E      a token's word index = the emit bits from its sentence's start up to its slot, less one: popcounts, no scan
//   giant  lane 0 writes spans and word indices next to the ids, counting as it goes
// and the direct form differs only in where the tile's run lies (the caller's arrays).
__device__ __forceinline__ WpNoSpanArgs wp_span_args() { return {}; }
__device__ __forceinline__ const WpSpanArgs &wp_span_args(const WpSpanArgs &a) { return a; }

template <class Lds, class... SpanArgs>
__global__ __launch_bounds__(64) void wp_encode_kernel(
    const uint8_t *__restrict__ text, uint64_t n_bytes, const uint64_t *__restrict__ sent_off,
    const uint64_t *__restrict__ plan, const uint8_t *__restrict__ cls_tab, WpDev T, uint32_t *__restrict__ scratch,
    uint32_t *__restrict__ sent_local, uint32_t *__restrict__ tile_tok, uint8_t *__restrict__ status, DirectOut direct,
    SpanArgs... span_args) {
  __shared__ Lds L;
  const auto sa = wp_span_args(span_args...);
  const int lane = threadIdx.x;
  const unsigned long long lt = (1ull << lane) - 1ull;
  WpTile tile;
  if (!wp_tile_begin(L, tile, sent_off, plan, cls_tab, scratch, tile_tok, direct, lane)) return;
  const WpOut out{sent_local, status, direct};
  uint32_t *tile_sp = nullptr;   // the tile's runs of spans and word indices, parallel to tile.tile_out
  uint32_t *tile_wd = nullptr;
  if constexpr (Lds::spans) {
    tile_sp = sa.sp + 2 * (tile.tile_out - scratch);
    tile_wd = sa.wd + (tile.tile_out - scratch);
  }

  for (;;) {
    WpChunk ch;
    wp_stage(L, tile, ch, text, n_bytes, lane);
    if (lane <= kWpBlocks) L.irr[lane] = 0ull;
    if constexpr (Lds::spans) {
      if (lane <= kWpBlocks) L.emit[lane] = 0ull;
    }
    __syncthreads();
    if (!wp_mark(L, tile, ch, sent_off, lane)) {
      const auto walk = [&](uint64_t b, uint64_t e, uint32_t *o, int &stt, uint64_t) {
        if constexpr (Lds::spans) {
          WpSpanSink sink{sa.tab, tile_sp + 2 * (o - tile.tile_out), tile_wd + (o - tile.tile_out), nullptr, 0, b, 0, 0, true};
          return wp_sentence(TxtSrc{text, nullptr, cls_tab}, b, e, o, T, stt, sink);
        } else {
          WpNoSpans none;
          return wp_sentence(TxtSrc{text, nullptr, cls_tab}, b, e, o, T, stt, none);
        }
      };
      if (wp_giant(L, tile, sent_off, out, T.empty_status, walk, lane)) break;
      continue;
    }

    // ---- B. classes -> masks -> candidates
    uint32_t nc = 0;
    bool prev_sp = true, prev_pu = false;  // class of the char owning the byte before this block
    for (uint32_t blk = 0; blk < ch.nblk; blk++) {
      const uint32_t p = blk * 64 + lane;
      bool inr, lead;
      const uint32_t cp = wp_decode(L, ch, p, inr, lead);
      uint8_t c = SWT_CLS_PY_SPACE;  // bytes outside the chunk behave as spaces
      if (inr && lead) c = cp < (uint32_t)kWpClsLds ? L.cls_lo[cp] : (cp < kNumCodePoints ? cls_tab[cp] : (uint8_t)0);
      const unsigned long long INR = __ballot(inr);
      const unsigned long long LEAD = __ballot(lead);
      const unsigned long long SPm = __ballot(lead && (c & SWT_CLS_PY_SPACE));
      const unsigned long long ANm = __ballot(lead && (c & SWT_CLS_PY_ALNUM));
      const unsigned long long PUm = LEAD & ~SPm & ~ANm;
      const unsigned long long CONT = ~LEAD;
      unsigned long long SPb = SPm | ((prev_sp && (CONT & 1ull)) ? 1ull : 0ull);
      unsigned long long PUb = PUm | ((prev_pu && (CONT & 1ull)) ? 1ull : 0ull);
      SPb |= (SPb << 1) & CONT; SPb |= (SPb << 1) & CONT; SPb |= (SPb << 1) & CONT;
      PUb |= (PUb << 1) & CONT; PUb |= (PUb << 1) & CONT; PUb |= (PUb << 1) & CONT;
      const unsigned long long SS = L.sbits[blk] & INR;
      const unsigned long long before_sp = ((SPb << 1) | (prev_sp ? 1ull : 0ull)) & ~SS;  // no context across a sentence start
      const unsigned long long before_pu = ((PUb << 1) | (prev_pu ? 1ull : 0ull)) & ~SS;
      const unsigned long long CAND = INR & (SS | (LEAD & ~SPm & (before_sp | before_pu | PUm)));
      if (lane == 0) L.ppunc[blk] = before_pu;
      if constexpr (Lds::spans) {
        if (lane == 0) L.lead[blk] = LEAD & INR;
      }
      if ((CAND >> lane) & 1ull) L.cand[nc + __popcll(CAND & lt)] = (uint16_t)p;
      nc += __popcll(CAND);
      L.tok[p] = kInvalidTok;
      prev_sp = (SPb >> 63) & 1ull;
      prev_pu = (PUb >> 63) & 1ull;
    }
    __syncthreads();

    // ---- C. one lane per candidate
    for (uint32_t k = lane; k < nc; k += 64) {
      const uint32_t p0 = L.cand[k];
      // the sentence around p0: [s0, e)
      const uint32_t s0 = wp_sentence_start(L, ch, p0);
      uint32_t e;
      {
        int w = (int)(p0 >> 6);
        unsigned long long m = (p0 & 63) == 63 ? 0ull : (L.sbits[w] & ~((2ull << (p0 & 63)) - 1ull));
        while (!m && w + 1 < (int)ch.nblk) m = L.sbits[++w];
        e = m ? (uint32_t)(w * 64 + __builtin_ctzll(m)) : ch.ce;
        if (e > ch.ce) e = ch.ce;
      }
      const bool has_succ = k + 1 < nc && L.cand[k + 1] < e;
      const uint32_t terr_end = has_succ ? L.cand[k + 1] : e;
      const uint64_t want_next = has_succ ? L.cand[k + 1] : (uint64_t)e + 1;
      TxtSrc src{L.txt, L.cls_lo, cls_tab};
      WpWalk<TxtSrc> w(src, T, p0, e, p0 != s0 && wbit(L.ppunc, p0));
      int stt = SWT_WP_OK;
      uint32_t n;
      if constexpr (Lds::spans) {
        uint32_t cp0 = 0;  // code points of the sentence in front of the candidate
        if (sa.tab.unit_cp) cp0 = wp_count(L.lead, s0, p0);
        WpSpanSink sink{sa.tab, &L.sp[2 * p0], nullptr, L.emit, p0, s0, cp0, 0, false};
        n = w.segment(&L.tok[p0], terr_end - p0, stt, sink);
      } else {
        WpNoSpans none;
        n = w.segment(&L.tok[p0], terr_end - p0, stt, none);
      }
      if (stt != SWT_WP_OK || w.i != want_next || n > terr_end - p0) atomicOr(&L.irr[s0 >> 6], 1ull << (s0 & 63));
    }
    __syncthreads();

    // ---- D. per sentence: status; the sequential walk where the speculation was not certified
    for (uint64_t s = tile.s_next + lane; s < tile.s_hi; s += 64) {
      const uint64_t rel = sent_off[s] - ch.abase;
      if (rel > ch.ce || (rel == ch.ce && !ch.last)) break;
      const uint64_t e = sent_off[s + 1] - ch.abase;  // <= ce: chunks end at sentence starts
      int stt = T.empty_status;
      if (rel < e) {
        stt = SWT_WP_OK;
        if (wbit(L.irr, (uint32_t)rel)) {
          TxtSrc src{L.txt, L.cls_lo, cls_tab};
          // the walker only reads L.txt, so the sentence's own bytes of L.tok are free to take its tokens
          uint32_t n;
          if constexpr (Lds::spans) {
            // what the candidates of this sentence left in emit goes; the redone segments mark their first slots
            for (uint32_t wq = (uint32_t)rel >> 6; wq <= ((uint32_t)e - 1) >> 6; wq++) {
              unsigned long long keep = 0ull;
              if (wq == (uint32_t)rel >> 6) keep |= (1ull << (rel & 63)) - 1ull;
              if (wq == (uint32_t)e >> 6) keep |= ~((1ull << (e & 63)) - 1ull);
              atomicAnd(&L.emit[wq], keep);
            }
            WpSpanSink sink{sa.tab, &L.sp[2 * rel], nullptr, L.emit, (uint32_t)rel, rel, 0, 0, true};
            n = wp_sentence(src, rel, e, &L.tok[rel], T, stt, sink);
          } else {
            WpNoSpans none;
            n = wp_sentence(src, rel, e, &L.tok[rel], T, stt, none);
          }
          for (uint64_t q = rel + n; q < e; q++) L.tok[q] = kInvalidTok;
        }
      }
      status[s] = (uint8_t)stt;
    }
    __syncthreads();

    if constexpr (Lds::spans) {
      if (lane <= kWpBlocks) {
        uint32_t before = 0;
        for (int wq = 0; wq < lane; wq++) before += __popcll(L.emit[wq]);
        L.epre[lane] = before;
      }
      __syncthreads();
      const auto extra = [&](uint32_t p, uint32_t k) {
        const uint32_t s0 = wp_sentence_start(L, ch, p);
        tile_sp[2 * k] = L.sp[2 * p];
        tile_sp[2 * k + 1] = L.sp[2 * p + 1];
        tile_wd[k] = wp_rank(L.emit, L.epre, p + 1) - wp_rank(L.emit, L.epre, s0) - 1u;
      };
      if (wp_emit(L, tile, ch, sent_off, out, lane, extra)) break;
    } else {
      if (wp_emit(L, tile, ch, sent_off, out, lane, WpNoExtra{})) break;
    }
  }
  wp_tile_end(tile, tile_tok, direct, lane);
}

// ---- host: trie build (utils.py:75-139) and flattening -------------------------------------------

struct HostTrie {
  std::vector<uint32_t> ch;
  std::vector<uint8_t> is_end;
  std::vector<int32_t> tok, link, parent;
  std::vector<std::vector<uint32_t>> pops, kids;
  std::unordered_map<uint64_t, uint32_t> edges;
  uint32_t root = 0, root_p = 1, root_sharp = 0;
  uint32_t n_vocab = 0;
  std::vector<uint32_t> corner;
  bool corner_nonterm = false;
  uint32_t sharp_depth = 0;   // length of the longest path of '#' edges from the root
  bool naive_excess = false;  // a token "###..." + other chars: NaiveWP.encode_word can emit more tokens than its word has bytes

  uint32_t new_node(uint32_t c, int32_t par) {
    ch.push_back(c); is_end.push_back(0); tok.push_back(-1); link.push_back(-1); parent.push_back(par);
    pops.emplace_back(); kids.emplace_back();
    return (uint32_t)ch.size() - 1;
  }
  int32_t child(uint32_t node, uint32_t c) const {
    auto it = edges.find(edge_key(node, c));
    return it == edges.end() ? -1 : (int32_t)it->second;
  }
  // utils.py:87-105
  uint32_t insert(const uint32_t *s, uint64_t n) {
    uint32_t node = root;
    for (uint64_t i = 0; i < n; i++) {
      int32_t c = child(node, s[i]);
      if (c < 0) {
        c = (int32_t)new_node(s[i], (int32_t)node);
        edges.emplace(edge_key(node, s[i]), (uint32_t)c);
        kids[node].push_back((uint32_t)c);
      }
      node = (uint32_t)c;
    }
    is_end[node] = 1;
    return node;
  }
};

static int build_trie(HostTrie &H, const uint32_t *blob, const uint64_t *off, uint32_t n_vocab) {
  const uint8_t *cls = host_class_table();
  H.n_vocab = n_vocab;
  H.root = H.new_node(0, -1);    // utils.py:77
  H.root_p = H.new_node(0, -1);  // utils.py:79
  const uint32_t sharp[2] = {'#', '#'};
  H.root_sharp = H.insert(sharp, 2);  // utils.py:81
  for (uint32_t v = 0; v < n_vocab; v++) {  // utils.py:83-84
    for (uint64_t i = off[v]; i < off[v + 1]; i++)
      if (blob[i] >= kNumCodePoints) return fail(SWT_ERR_INVALID, "vocab entry %u holds an invalid code point", v);
    const uint32_t node = H.insert(blob + off[v], off[v + 1] - off[v]);
    if (H.tok[node] < 0) H.tok[node] = (int32_t)v;
    uint64_t lead = 0;
    while (off[v] + lead < off[v + 1] && blob[off[v] + lead] == '#') lead++;
    if (lead >= 3 && off[v] + lead < off[v + 1]) H.naive_excess = true;
    if (H.ch.size() > kMaxNodes) return fail(SWT_ERR_UNSUPPORTED, "trie larger than %u nodes", kMaxNodes);
  }
  // utils.py:108-139: BFS from [root, root_sharp]
  std::vector<uint32_t> queue{H.root, H.root_sharp};
  for (size_t qh = 0; qh < queue.size(); qh++) {
    const uint32_t u = queue[qh];
    for (uint32_t c : H.kids[u]) {
      if (c == H.root_sharp) continue;  // :119-120
      const uint32_t chr = H.ch[c];
      if (H.is_end[c]) {  // :121-123
        H.link[c] = (int32_t)H.root_sharp;
        H.pops[c] = {(uint32_t)H.tok[c]};
      } else {  // :124-132
        int32_t f = H.link[u];
        std::vector<uint32_t> acc;
        while (f >= 0 && H.child((uint32_t)f, chr) < 0) {
          acc.insert(acc.end(), H.pops[f].begin(), H.pops[f].end());
          f = H.link[f];
        }
        if (f >= 0) {
          H.link[c] = H.child((uint32_t)f, chr);
          H.pops[c] = H.pops[u];
          H.pops[c].insert(H.pops[c].end(), acc.begin(), acc.end());
        }
      }
      if (!(cls[chr] & SWT_CLS_PY_ALNUM)) H.link[c] = (int32_t)H.root_p;  // :136-137
      queue.push_back(c);
    }
  }
  // NaiveWP.encode_word("##") (wordpiece.py:144-159): the word is a run of '#'; state = its length L
  {
    std::vector<uint32_t> chain{H.root};
    for (;;) {
      const int32_t c = H.child(chain.back(), '#');
      if (c < 0) break;
      chain.push_back((uint32_t)c);
    }
    const uint64_t D = chain.size() - 1;
    H.sharp_depth = (uint32_t)D;
    uint64_t L = 2, guard = 0;
    std::vector<uint8_t> visited(D + 8, 0);
    for (;;) {
      uint64_t i = L < D ? L : D;
      while (i > 0 && !(H.is_end[chain[i]] && H.tok[chain[i]] >= 0)) i--;
      if (i == 0) { H.corner = {n_vocab + 1}; break; }  // :148-149 ["[UNK]"]
      H.corner.push_back((uint32_t)H.tok[chain[i]]);
      L -= i;
      if (L == 0) break;
      L += 2;  // :155-156
      if (L < D + 8) {
        if (visited[L]) { H.corner_nonterm = true; break; }
        visited[L] = 1;
      }
      if (++guard > 1000000) { H.corner_nonterm = true; break; }
    }
    if (H.corner_nonterm) H.corner.clear();
  }
  return SWT_OK;
}

// After the encode over the unique chunks (every chunk a "sentence" of that launch): each chunk's token run -- its place in
// the launch's scratch and its length, or kRecFailed when the reference never returns on it -- goes to its table slot.
__global__ __launch_bounds__(64) void wp_urec_kernel(const uint64_t *__restrict__ uoff, const uint64_t *__restrict__ plan,
                                                     const uint32_t *__restrict__ sent_local, const uint32_t *__restrict__ tile_tok,
                                                     const uint8_t *__restrict__ status, const uint32_t *__restrict__ uslot,
                                                     unsigned long long *__restrict__ rec, unsigned long long *__restrict__ drec) {
  const uint64_t t = blockIdx.x;
  const uint64_t s_lo = plan[t], s_hi = plan[t + 1];
  if (s_lo == s_hi) return;
  const uint64_t span_base = uoff[s_lo];
  const uint32_t total = tile_tok[t];
  for (uint64_t s = s_lo + threadIdx.x; s < s_hi; s += 64) {
    const uint32_t a = sent_local[s], b = s + 1 < s_hi ? sent_local[s + 1] : total;
    const uint32_t cnt = status[s] != SWT_WP_OK ? kRecFailed : b - a;
    drec[s] = (span_base + a) | ((unsigned long long)cnt << 32);  // dense, for the last pass
    rec[uslot[s]] = s | ((unsigned long long)cnt << 32);           // the counting pass finds the unique index here
  }
}

// ---- NaiveWP encode: SubwordTokenizer.preprocessing (utils.py:15-29) + NaiveWP.encode_word (wordpiece.py:132-159) ----------
//
// The state of encode_word is the string "#" * L + word[p:] (L leading '#' that no character of the word stands for: the "##"
// put in front of every remainder, wordpiece.py:155-156).  A step matches the longest prefix of that string that is a
// vocabulary token (tok[] of the node, not is_end: root_sharp is marked whether "##" is a token or not).  A match that ends
// inside the leading '#' leaves p where it is and sets L = L - m + 2.  At a fixed p at most sharp_depth + 1 values of L can
// occur before the walk either leaves p or cannot come back (L beyond the '#' chain of the trie, where every match is the same
// run of '#', grows or stays): so more than sharp_depth + 2 steps at one p mean the reference never returns.
struct WpNaiveDev {
  WpDev T;             // edges only
  const int32_t *tok;  // node -> vocabulary id, -1 for none
  uint32_t unk_id;     // "[UNK]"
  uint32_t max_steps;  // sharp_depth + 2
};

// ---- MaxMatch-Dropout (include/swt.h, swt_wp_encode_naive_dropout): the same walk with a vocabulary match
// thrown away when its draw says so.  A candidate that takes c >= 2 code points of the word from byte a of sentence i is dropped
// when word c & 3 of Philox at the counter (c >> 2, a, i, epoch) is below drop_below: one call serves four consecutive c.  The
// candidates of one step come in rising c, so the last call's four words are all that is kept.
// Termination: the draws at one p are functions of (a, c) alone, the same in every step there, so the steps at a fixed p are the
// plain steps over a vocabulary with some tokens removed -- never a '#'-only one (c = 0), never a single code point (c = 1).  The
// bound above speaks of the '#' chain of the trie alone, which is whole: more than sharp_depth + 2 steps at one p still mean that
// the (thinned) reference walk never returns.  And a word that terminates still makes no step inside the leading '#' (such a step
// from L = 2 comes back to L = 2 at the same p or never below it), so its tokens are at most its code points: room is not passed.
struct WpDrawArgs {  // what a dropout launch draws with: arguments of the dropout kernel, and of no other
  unsigned long long drop_below;  // 0 .. 2^32
  uint32_t key0, key1, epoch;
};
struct WpNoDraw {
  static constexpr bool on = false;
};
struct WpDraw {
  static constexpr bool on = true;
  const WpDrawArgs &d;
  const uint32_t i, a0;  // the word's sentence in the call's sent_off; the byte offset of the word in that sentence (both mod 2^32)
  uint32_t group = 0xFFFFFFFFu, at = 0;  // c >> 2 and a of the call `x` holds (c counts code points of a text: no group is all ones)
  Philox x{};
  __device__ __forceinline__ WpDraw(const WpDrawArgs &args, uint32_t sent, uint32_t word_at) : d(args), i(sent), a0(word_at) {}
  __device__ __forceinline__ bool dropped(uint32_t a, uint32_t c) {
    if ((c >> 2) != group || a != at) {
      group = c >> 2;
      at = a;
      x = philox4x32_10(group, a, i, d.epoch, d.key0, d.key1);
    }
    const uint32_t q = c & 3u;
    const uint32_t v = q == 0u ? x.x[0] : q == 1u ? x.x[1] : q == 2u ? x.x[2] : x.x[3];
    return v < d.drop_below;
  }
};

// One word [wb, we) of txt: its ids to out[0..room), the count returned.  nonterm = true: the reference never returns (count 0).
// draw: WpNoDraw, the plain walk and not an instruction more, or the word's WpDraw.
template <class Draw>
__device__ uint32_t naive_word(const uint8_t *txt, uint64_t wb, uint64_t we, const WpNaiveDev &N, uint32_t *out, uint32_t room,
                               bool &nonterm, Draw &draw) {
  uint32_t nt = 0, L = 0, steps = 0;
  uint64_t p = wb;
  for (;;) {
    uint32_t node = kWpRoot, best_sh = 0;
    int32_t best = -1;
    uint64_t best_end = p;
    uint32_t k = 0;
    [[maybe_unused]] uint32_t taken = 0;  // code points of the word that the candidate at hand takes (c of the rule)
    for (; k < L; k++) {
      const int32_t c = edge_lookup(N.T, node, '#');
      if (c < 0) break;
      node = (uint32_t)c;
      const int32_t v = N.tok[node];
      if (v >= 0) { best = v; best_sh = k + 1; }
    }
    if (k == L) {
      for (uint64_t q = p; q < we;) {
        const uint8_t b = txt[q];
        int n = utf8_len(b);
        if (q + n > we) n = (int)(we - q);
        uint32_t cp = b;
        if (b >= 0x80 && n > 1) {
          cp = b & (0xFF >> (n + 1));
          for (int i = 1; i < n; i++) cp = (cp << 6) | (txt[q + i] & 0x3F);
        }
        q += n;
        while (q < we && utf8_is_cont(txt[q])) q++;
        const int32_t c = edge_lookup(N.T, node, cp);
        if (c < 0) break;
        node = (uint32_t)c;
        const int32_t v = N.tok[node];
        if constexpr (Draw::on) {
          taken++;
          if (v >= 0 && taken >= 2 && draw.dropped(draw.a0 + (uint32_t)(p - wb), taken)) continue;
        }
        if (v >= 0) { best = v; best_sh = L; best_end = q; }
      }
    }
    if (best < 0) {  // wordpiece.py:148-149: the whole word is one "[UNK]", the pieces stored so far are dropped
      for (uint32_t k = 1; k < nt && k < room; k++) out[k] = kInvalidTok;
      out[0] = N.unk_id;
      return 1;
    }
    if (nt < room) out[nt] = (uint32_t)best;
    nt++;
    if (best_sh == L && best_end == we) return nt;  // nothing left
    if (best_end > p) {
      p = best_end;
      L = 2;
      steps = 0;
    } else {
      L = L - best_sh + 2;
      if (++steps > N.max_steps) { nonterm = true; return 0; }
    }
  }
}

__device__ __forceinline__ uint8_t bert_class(const uint8_t *cls_tab, uint32_t cp) {
  return cp < kNumCodePoints ? (uint8_t)(cls_tab[cp] & (SWT_CLS_BERT_WS | SWT_CLS_BERT_PUNCT)) : (uint8_t)0;
}

// A whole sentence [b, e) by one lane (sentences longer than a chunk): split as SubwordTokenizer._split, each word's tokens
// within that word's bytes of out.  Returns the count (0 when status != OK).  Dropout: the sentence is number i of the call, and
// its words draw by their offsets from b -- the key the tiled walk gives the same word.
template <bool Dropout>
using WpDrawOf = std::conditional_t<Dropout, WpDrawArgs, WpNoDraw>;
template <bool Dropout>
__device__ uint32_t naive_sentence(const uint8_t *txt, const uint8_t *cls_tab, uint64_t b, uint64_t e, uint32_t *out,
                                   const WpNaiveDev &N, int &status, [[maybe_unused]] const WpDrawOf<Dropout> &args,
                                   [[maybe_unused]] uint64_t i) {
  TxtSrc src{txt, nullptr, cls_tab};
  uint32_t nt = 0;
  status = SWT_WP_OK;
  uint64_t p = b;
  while (p < e) {
    uint32_t cp, cc, len;
    src.load(p, e, cp, cc, len);
    const uint8_t c = bert_class(cls_tab, cp);
    if (c & SWT_CLS_BERT_WS) { p += len; continue; }
    uint64_t q = p + len;
    if (!(c & SWT_CLS_BERT_PUNCT)) {
      while (q < e) {
        src.load(q, e, cp, cc, len);
        if (bert_class(cls_tab, cp)) break;
        q += len;
      }
    }
    bool nonterm = false;
    if constexpr (Dropout) {
      WpDraw draw(args, (uint32_t)i, (uint32_t)(p - b));
      nt += naive_word(txt, p, q, N, out + nt, (uint32_t)(q - p), nonterm, draw);
    } else {
      WpNoDraw none;
      nt += naive_word(txt, p, q, N, out + nt, (uint32_t)(q - p), nonterm, none);
    }
    if (nonterm) { status = SWT_WP_NONTERMINATING; return 0; }
    p = q;
  }
  return nt;
}

struct alignas(16) WpNaiveLds : WpTileLds {
  unsigned long long stop[kWpBlocks + 1];    // a word ends before this byte: white space, punctuation, a sentence start, outside
  unsigned long long pbits[kWpBlocks + 1];   // a punctuation character (a word of its own) starts here
  unsigned long long nonterm[kWpBlocks + 1]; // per sentence-start position: a word of the sentence never returns
};

// The skeleton of wp_encode_kernel (wp_tile_begin .. wp_tile_end) with these phases.  Word boundaries do not depend on the
// vocabulary here, so there is nothing to speculate about:
//   B  64 bytes per step: BERT white-space / punctuation ballots -> word starts and word ends
//   C  one lane per word runs the MaxMatch walk, writing its ids into the word's own bytes of tok[] (a terminating word of n
//      bytes has at most n tokens: swt_wp_encode_naive_dev refuses the vocabularies for which that does not hold)
//   D  a sentence with a word that never returns gets status SWT_WP_NONTERMINATING and no tokens
// Two instantiations: wp_naive_kernel<false>, the plain walk with the arguments, resources and instructions it always had, and
// wp_naive_kernel<true>, MaxMatch-Dropout (swt_wp_encode_naive_dropout*): the draws travel behind the DirectOut in the last
// argument, and in C every lane looks up the key of its word -- a = its offset from wp_sentence_start, i = the last sentence of
// sent_off[s_next .. s_hi) that starts at or before it (empty sentences share their offset with the next one that has bytes, and
// that one it is).  The one-lane walk in global memory has both at hand and draws by the same key.
struct WpDirectDrop : DirectOut { WpDrawArgs draw; };
template <bool Dropout>
__global__ __launch_bounds__(64) void wp_naive_kernel(
    const uint8_t *__restrict__ text, uint64_t n_bytes, const uint64_t *__restrict__ sent_off,
    const uint64_t *__restrict__ plan, const uint8_t *__restrict__ cls_tab, WpNaiveDev N, uint32_t *__restrict__ scratch,
    uint32_t *__restrict__ sent_local, uint32_t *__restrict__ tile_tok, uint8_t *__restrict__ status,
    std::conditional_t<Dropout, WpDirectDrop, DirectOut> direct) {
  WpDrawOf<Dropout> draw_args{};
  if constexpr (Dropout) draw_args = direct.draw;
  __shared__ WpNaiveLds L;
  const int lane = threadIdx.x;
  const unsigned long long lt = (1ull << lane) - 1ull;
  WpTile tile;
  if (!wp_tile_begin(L, tile, sent_off, plan, cls_tab, scratch, tile_tok, direct, lane)) return;
  const WpOut out{sent_local, status, direct};

  for (;;) {
    WpChunk ch;
    wp_stage(L, tile, ch, text, n_bytes, lane);
    if (lane <= kWpBlocks) L.nonterm[lane] = 0ull;
    __syncthreads();
    if (!wp_mark(L, tile, ch, sent_off, lane)) {
      const auto walk = [&](uint64_t b, uint64_t e, uint32_t *o, int &stt, uint64_t s) {
        return naive_sentence<Dropout>(text, cls_tab, b, e, o, N, stt, draw_args, s);
      };
      if (wp_giant(L, tile, sent_off, out, SWT_WP_OK, walk, lane)) break;
      continue;
    }

    // ---- B. classes -> word starts and ends
    uint32_t nc = 0;
    bool prev_stop = true;  // the char owning the byte before this block is white space or punctuation
    for (uint32_t blk = 0; blk < ch.nblk; blk++) {
      const uint32_t p = blk * 64 + lane;
      bool inr, lead;
      const uint32_t cp = wp_decode(L, ch, p, inr, lead);
      uint8_t c = SWT_CLS_BERT_WS;  // bytes outside the chunk behave as white space
      if (inr && lead) c = cp < (uint32_t)kWpClsLds ? (uint8_t)(L.cls_lo[cp] & (SWT_CLS_BERT_WS | SWT_CLS_BERT_PUNCT)) : bert_class(cls_tab, cp);
      const unsigned long long INR = __ballot(inr);
      const unsigned long long LEAD = __ballot(lead);
      const unsigned long long WSm = __ballot(lead && (c & SWT_CLS_BERT_WS));
      const unsigned long long PUm = __ballot(lead && (c & SWT_CLS_BERT_PUNCT) && !(c & SWT_CLS_BERT_WS));
      const unsigned long long CONT = ~LEAD;
      unsigned long long STb = WSm | PUm | ((prev_stop && (CONT & 1ull)) ? 1ull : 0ull);
      STb |= (STb << 1) & CONT; STb |= (STb << 1) & CONT; STb |= (STb << 1) & CONT;
      const unsigned long long SS = L.sbits[blk] & INR;
      const unsigned long long before = ((STb << 1) | (prev_stop ? 1ull : 0ull)) & ~SS;  // no context across a sentence start
      const unsigned long long CAND = INR & LEAD & ~WSm & (SS | before | PUm);
      if (lane == 0) { L.stop[blk] = WSm | PUm | SS | ~INR; L.pbits[blk] = PUm & INR; }
      if ((CAND >> lane) & 1ull) L.cand[nc + __popcll(CAND & lt)] = (uint16_t)p;
      nc += __popcll(CAND);
      L.tok[p] = kInvalidTok;
      prev_stop = (STb >> 63) & 1ull;
    }
    __syncthreads();

    // ---- C. one lane per word
    for (uint32_t k = lane; k < nc; k += 64) {
      const uint32_t p0 = L.cand[k];
      uint32_t we;
      if (wbit(L.pbits, p0)) {
        we = p0 + 1;
        while (we < ch.ce && utf8_is_cont(L.txt[we])) we++;
      } else {
        int w = (int)(p0 >> 6);
        unsigned long long m = (p0 & 63) == 63 ? 0ull : (L.stop[w] & ~((2ull << (p0 & 63)) - 1ull));
        while (!m && w + 1 < (int)ch.nblk) m = L.stop[++w];
        we = m ? (uint32_t)(w * 64 + __builtin_ctzll(m)) : ch.ce;
        if (we > ch.ce) we = ch.ce;
      }
      bool nt_word = false;
      if constexpr (Dropout) {
        const uint32_t s0 = wp_sentence_start(L, ch, p0);
        const uint64_t g = ch.abase + p0;
        uint64_t lo = tile.s_next, hi = tile.s_hi;  // sent_off[lo] <= g (the chunk begins at a sentence start) < sent_off[hi]
        while (hi - lo > 1) {
          const uint64_t mid = lo + ((hi - lo) >> 1);
          if (sent_off[mid] <= g) lo = mid; else hi = mid;
        }
        WpDraw draw(draw_args, (uint32_t)lo, p0 - s0);
        naive_word(L.txt, p0, we, N, &L.tok[p0], we - p0, nt_word, draw);
      } else {
        WpNoDraw none;
        naive_word(L.txt, p0, we, N, &L.tok[p0], we - p0, nt_word, none);
      }
      if (nt_word) {
        const uint32_t s0 = wp_sentence_start(L, ch, p0);
        atomicOr(&L.nonterm[s0 >> 6], 1ull << (s0 & 63));
      }
    }
    __syncthreads();

    // ---- D. per sentence: status; a sentence that never returns keeps no tokens
    for (uint64_t s = tile.s_next + lane; s < tile.s_hi; s += 64) {
      const uint64_t rel = sent_off[s] - ch.abase;
      if (rel > ch.ce || (rel == ch.ce && !ch.last)) break;
      const uint64_t e = sent_off[s + 1] - ch.abase;
      int stt = SWT_WP_OK;
      if (rel < e && wbit(L.nonterm, (uint32_t)rel)) {
        stt = SWT_WP_NONTERMINATING;
        for (uint64_t q = rel; q < e; q++) L.tok[q] = kInvalidTok;
      }
      status[s] = (uint8_t)stt;
    }
    __syncthreads();

    if (wp_emit(L, tile, ch, sent_off, out, lane, WpNoExtra{})) break;
  }
  wp_tile_end(tile, tile_tok, direct, lane);
}

}  // namespace swt

using namespace swt;

struct swt_wp_trie {
  HostTrie H;
  // flattened
  std::vector<uint64_t> h_edges;
  std::vector<WpNode> h_nodes;
  std::vector<uint32_t> h_pops;
  uint32_t edge_bits = 0;
  // device (uploaded on first encode)
  uint64_t *d_edges = nullptr;
  WpNode *d_nodes = nullptr;
  uint32_t *d_pops = nullptr;
  int32_t *d_tok = nullptr;  // node -> vocabulary id (NaiveWP encode), uploaded on its first call
  TileWorkspace ws;
  HostStage stage;  // the host entry points (host_encode*, swt_tile.h)
  // word-level dedup inside one call (swt_dedup.h): possible when no vocabulary token holds a str.isspace character
  bool dedup_ok = false;
  DedupEngine dd;
  TileWorkspace ws2;  // the encode over the unique chunks
  DevBuf u_status;
  // token spans (swt_wp_encode_spans): code points of every vocabulary token with kWpLenCont on the '##' ones, built with the
  // trie and uploaded by the first spans call; the scratch runs of spans (8 bytes per text byte) and word indices (4), grow-only
  std::vector<uint32_t> h_len;
  uint32_t *d_len = nullptr;
  DevBuf sp_scratch, wd_scratch;
};

static WpDev wp_dev(const swt_wp_trie *t) {
  WpDev T;
  T.edges = t->d_edges;
  T.edge_bits = t->edge_bits;
  T.nodes = t->d_nodes;
  T.pops = t->d_pops;
  T.root_sharp = t->H.root_sharp;
  T.unk_id = t->H.n_vocab;
  T.corner_nonterm = t->H.corner_nonterm ? 1u : 0u;
  T.empty_status = t->H.child(t->H.root, ' ') >= 0 ? SWT_WP_INDEXERROR : SWT_WP_OK;
  T.corner_id = t->H.corner.size() == 1 ? t->H.corner[0] : t->H.n_vocab + 2;
  return T;
}

static int wp_upload(swt_wp_trie *t) {
  if (t->d_edges) return SWT_OK;
  int rc = ensure_device();
  if (rc) return rc;
  SWT_HIP(hipMalloc((void **)&t->d_edges, t->h_edges.size() * 8));
  SWT_HIP(hipMemcpy(t->d_edges, t->h_edges.data(), t->h_edges.size() * 8, hipMemcpyHostToDevice));
  SWT_HIP(hipMalloc((void **)&t->d_nodes, t->h_nodes.size() * sizeof(WpNode)));
  SWT_HIP(hipMemcpy(t->d_nodes, t->h_nodes.data(), t->h_nodes.size() * sizeof(WpNode), hipMemcpyHostToDevice));
  SWT_HIP(hipMalloc((void **)&t->d_pops, (t->h_pops.size() + 1) * 4));
  if (!t->h_pops.empty())
    SWT_HIP(hipMemcpy(t->d_pops, t->h_pops.data(), t->h_pops.size() * 4, hipMemcpyHostToDevice));
  return SWT_OK;
}

static int wp_upload_naive(swt_wp_trie *t) {
  int rc = wp_upload(t);
  if (rc || t->d_tok) return rc;
  SWT_HIP(hipMalloc((void **)&t->d_tok, t->H.tok.size() * 4));
  SWT_HIP(hipMemcpy(t->d_tok, t->H.tok.data(), t->H.tok.size() * 4, hipMemcpyHostToDevice));
  return SWT_OK;
}

static int wp_upload_spans(swt_wp_trie *t) {
  int rc = wp_upload(t);
  if (rc || t->d_len) return rc;
  SWT_HIP(hipMalloc((void **)&t->d_len, (t->h_len.size() + 1) * 4));
  if (!t->h_len.empty()) SWT_HIP(hipMemcpy(t->d_len, t->h_len.data(), t->h_len.size() * 4, hipMemcpyHostToDevice));
  return SWT_OK;
}

extern "C" {

int swt_wp_trie_create(const uint32_t *vocab_cps, const uint64_t *vocab_off, uint32_t n_vocab, swt_wp_trie **out) try {
  if (!out || !vocab_off || (n_vocab && vocab_off[n_vocab] && !vocab_cps)) return fail(SWT_ERR_INVALID, "null argument");
  if (n_vocab > 0x7FFFFFF0u) return fail(SWT_ERR_INVALID, "vocabulary too large");
  auto *t = new swt_wp_trie();
  int rc = build_trie(t->H, vocab_cps, vocab_off, n_vocab);
  if (rc) { delete t; return rc; }
  const HostTrie &H = t->H;
  const size_t n_nodes = H.ch.size();
  // the length table of the spans call: the strings are at hand here and only here
  t->h_len.resize(n_vocab);
  for (uint32_t v = 0; v < n_vocab; v++) {
    const uint64_t a = vocab_off[v], n = vocab_off[v + 1] - a;
    const bool cont = n >= 2 && vocab_cps[a] == '#' && vocab_cps[a + 1] == '#';
    t->h_len[v] = (uint32_t)(n < 0xFFFFFFu ? n : 0xFFFFFFu) | (cont ? kWpLenCont : 0u);
  }
  // flatten: nodes + pops
  t->h_nodes.resize(n_nodes);
  for (size_t k = 0; k < n_nodes; k++) {
    WpNode &nd = t->h_nodes[k];
    nd.link = H.link[k];
    nd.pop_off = (uint32_t)t->h_pops.size();
    nd.pop_cnt = (uint32_t)H.pops[k].size();
    nd.flags = H.is_end[k];
    t->h_pops.insert(t->h_pops.end(), H.pops[k].begin(), H.pops[k].end());
  }
  // edges
  uint32_t bits = 4;
  while ((1ull << bits) < 2ull * H.edges.size() + 2) bits++;
  t->edge_bits = bits;
  t->h_edges.assign((size_t)1 << bits, kEdgeEmpty);
  const uint32_t mask = (1u << bits) - 1;
  for (const auto &kv : H.edges) {
    uint32_t h = hash_slot(kv.first, bits);
    while (t->h_edges[h] != kEdgeEmpty) h = (h + 1) & mask;
    t->h_edges[h] = (kv.first << 21) | kv.second;
  }
  // A segment of FastWP.tokenize never reads past the whitespace that ends its chunk unless the trie has an edge labelled
  // with a whitespace character (wordpiece.py:291-316 follows edges only): then, and only then, chunks are independent.
  t->dedup_ok = true;
  for (const auto &kv : H.edges) {
    const uint32_t cp = (uint32_t)(kv.first & ((1u << 21) - 1u));
    if (cp < kNumCodePoints && (host_class_table()[cp] & SWT_CLS_PY_SPACE)) t->dedup_ok = false;
  }
  *out = t;
  return SWT_OK;
} SWT_API_CATCH

int swt_wp_trie_set_option(swt_wp_trie *t, int option, int value) try {
  if (!t) return fail(SWT_ERR_INVALID, "null trie");
  switch (option) {
    case SWT_OPT_DEDUP:
      if (value < 0 || value > 2) return fail(SWT_ERR_INVALID, "SWT_OPT_DEDUP takes 0, 1 or 2");
      t->dd.opt_mode = value;
      return SWT_OK;
    case SWT_OPT_DEDUP_TABLE_BITS:
      if (value != 0 && (value < 4 || value > 24)) return fail(SWT_ERR_INVALID, "SWT_OPT_DEDUP_TABLE_BITS takes 0 or 4..24");
      t->dd.opt_table_bits = (uint32_t)value;
      return SWT_OK;
  }
  return fail(SWT_ERR_INVALID, "no such option");
} SWT_API_CATCH

void swt_wp_trie_destroy(swt_wp_trie *t) try {
  if (!t) return;
  if (t->d_edges) (void)hipFree(t->d_edges);
  if (t->d_nodes) (void)hipFree(t->d_nodes);
  if (t->d_pops) (void)hipFree(t->d_pops);
  if (t->d_tok) (void)hipFree(t->d_tok);
  if (t->d_len) (void)hipFree(t->d_len);
  t->sp_scratch.release();
  t->wd_scratch.release();
  t->ws.release();
  t->ws2.release();
  t->dd.release();
  t->stage.release();
  t->u_status.release();
  delete t;
} SWT_API_CATCH_VOID

int swt_wp_trie_stats(const swt_wp_trie *t, uint32_t *n_nodes, uint32_t *n_edges, uint32_t *n_pops) try {
  if (!t) return fail(SWT_ERR_INVALID, "null trie");
  if (n_nodes) *n_nodes = (uint32_t)t->H.ch.size();
  if (n_edges) *n_edges = (uint32_t)t->H.edges.size();
  if (n_pops) *n_pops = (uint32_t)t->h_pops.size();
  return SWT_OK;
} SWT_API_CATCH

int64_t swt_wp_trie_corner(const swt_wp_trie *t, uint32_t *out, uint64_t cap) try {
  if (!t) return -2;
  if (t->H.corner_nonterm) return -1;
  for (size_t k = 0; k < t->H.corner.size() && k < cap; k++) out[k] = t->H.corner[k];
  return (int64_t)t->H.corner.size();
} SWT_API_CATCH

int swt_wp_trie_node(const swt_wp_trie *t, const uint32_t *path, uint64_t path_len, uint32_t *node_id, int32_t *link,
                     uint8_t *is_end, uint32_t *pops, uint32_t pops_cap, uint32_t *n_pops) try {
  if (!t) return fail(SWT_ERR_INVALID, "null trie");
  uint32_t node = t->H.root;
  for (uint64_t i = 0; i < path_len; i++) {
    const int32_t c = t->H.child(node, path[i]);
    if (c < 0) return fail(SWT_ERR_INVALID, "no such trie path");
    node = (uint32_t)c;
  }
  if (node_id) *node_id = node;
  if (link) *link = t->H.link[node];
  if (is_end) *is_end = t->H.is_end[node];
  if (n_pops) *n_pops = (uint32_t)t->H.pops[node].size();
  for (size_t k = 0; k < t->H.pops[node].size() && k < pops_cap; k++) pops[k] = t->H.pops[node][k];
  return SWT_OK;
} SWT_API_CATCH

int swt_wp_trie_node_path(const swt_wp_trie *t, uint32_t node_id, uint32_t *out, uint64_t cap, uint64_t *len) try {
  if (!t || node_id >= t->H.ch.size()) return fail(SWT_ERR_INVALID, "bad node id");
  std::vector<uint32_t> rev;
  for (int32_t n = (int32_t)node_id; n >= 0 && t->H.parent[n] >= 0; n = t->H.parent[n]) rev.push_back(t->H.ch[n]);
  if (len) *len = rev.size();
  for (size_t k = 0; k < rev.size() && k < cap; k++) out[k] = rev[rev.size() - 1 - k];
  return SWT_OK;
} SWT_API_CATCH

int swt_wp_encode_dev(swt_wp_trie *t, const uint8_t *d_text, uint64_t n_bytes, const uint64_t *d_sent_off, uint64_t n_sent,
                      uint32_t *d_out_ids, uint64_t *d_out_off, uint8_t *d_status, uint64_t *d_n_tokens, void *stream) try {
  if (!t || !d_sent_off || !d_out_off || !d_n_tokens || (n_sent && !d_status) || (n_bytes && (!d_text || !d_out_ids)))
    return fail(SWT_ERR_INVALID, "null argument");
  int rc = wp_upload(t);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const uint8_t *d_cls = nullptr;
  if ((rc = device_class_table(&d_cls))) return rc;
  const uint64_t n_tiles = tile_count(n_bytes, kWpTile);
  if (n_tiles > 0x7FFFFFFFull)
    return fail(SWT_ERR_UNSUPPORTED, "text too large for one call (%llu bytes)", (unsigned long long)n_bytes);
  if ((rc = t->ws.reserve(n_bytes, n_sent, n_tiles))) return rc;
  if (n_sent == 0) {
    SWT_HIP(hipMemsetAsync(d_out_off, 0, 8, st));
    SWT_HIP(hipMemsetAsync(d_n_tokens, 0, 8, st));
    return SWT_OK;
  }
  const WpDev T = wp_dev(t);
  if (n_bytes <= kWpDirectBytes && n_sent <= kWpDirectSents && t->dd.opt_mode != 2) {
    // a sentence or a few: one workgroup, one launch, the caller's arrays written by the kernel (DirectOut, swt_tile.h)
    hipLaunchKernelGGL((wp_encode_kernel<WpLds>), dim3(1), dim3(64), 0, st, d_text, n_bytes, d_sent_off, (const uint64_t *)nullptr, d_cls, T,
                       d_out_ids, t->ws.sent_local.as<uint32_t>(), t->ws.tile_tok.as<uint32_t>(), d_status,
                       DirectOut{d_out_off, d_n_tokens, n_sent});
    SWT_HIP(hipGetLastError());
    return SWT_OK;
  }
  // debug knob 1: bit 0 = never dedup, bit 1 = dedup whatever the batch size (tests)
  if (t->dedup_ok && T.empty_status == SWT_WP_OK && n_bytes <= kDedupMaxBytes && t->dd.opt_mode != 1 &&
      (n_bytes >= kDedupMinBytesWp || t->dd.opt_mode == 2)) {
    // Word-level dedup (swt_dedup.h): the chunks between whitespace are encoded once per call.  The encode over the unique
    // chunks is this same kernel with every chunk as a "sentence"; its launch size is fixed and the tile size follows on
    // the device (the number of unique chunks never reaches the host).
    const uint64_t max_uniq = n_bytes + 2;
    uint64_t n_tiles2 = tile_count(n_bytes, kWpUTile);
    if (n_tiles2 > kWpUMaxTiles) n_tiles2 = kWpUMaxTiles;
    if ((rc = t->ws2.reserve(n_bytes, max_uniq, n_tiles2)) || (rc = t->u_status.reserve(max_uniq + 2))) return rc;
    prof_begin(st, 2);
    if ((rc = dedup_front(t->dd, t->ws, d_text, n_bytes, d_sent_off, n_sent, d_cls, kDedupWp, st, t->ws2.plan.as<uint64_t>(), n_tiles2,
                          kWpUTile)))
      return rc;
    prof_begin(st);
    hipLaunchKernelGGL((wp_encode_kernel<WpLds>), dim3((unsigned)n_tiles2), dim3(64), 0, st, t->dd.utext.as<uint8_t>(), n_bytes,
                       t->dd.uoff.as<uint64_t>(), t->ws2.plan.as<uint64_t>(), d_cls, T, t->ws2.scratch.as<uint32_t>(),
                       t->ws2.sent_local.as<uint32_t>(), t->ws2.tile_tok.as<uint32_t>(), t->u_status.as<uint8_t>(),
                       DirectOut{nullptr, nullptr, 0});
    prof_end(st);
    hipLaunchKernelGGL(wp_urec_kernel, dim3((unsigned)n_tiles2), dim3(64), 0, st, t->dd.uoff.as<uint64_t>(), t->ws2.plan.as<uint64_t>(),
                       t->ws2.sent_local.as<uint32_t>(), t->ws2.tile_tok.as<uint32_t>(), t->u_status.as<uint8_t>(),
                       t->dd.uslot.as<uint32_t>(), t->dd.rec_ptr(), t->dd.drec_ptr());
    rc = dedup_back(t->dd, t->ws, d_sent_off, n_sent, n_bytes, t->ws2.scratch.as<uint32_t>(), kDedupWp, d_status, d_out_ids, d_out_off,
                    d_n_tokens, st);
    prof_end(st, 2);
    return rc;
  }
  prof_begin(st, 2);
  launch_plan(d_sent_off, n_sent, n_tiles, kWpTile, t->ws.plan.as<uint64_t>(), st);
  prof_begin(st);
  hipLaunchKernelGGL((wp_encode_kernel<WpLds>), dim3((unsigned)n_tiles), dim3(64), 0, st, d_text, n_bytes, d_sent_off,
                     t->ws.plan.as<uint64_t>(), d_cls, T, t->ws.scratch.as<uint32_t>(), t->ws.sent_local.as<uint32_t>(),
                     t->ws.tile_tok.as<uint32_t>(), d_status, DirectOut{nullptr, nullptr, 0});
  prof_end(st);
  launch_scan_gather(d_sent_off, n_sent, n_tiles, t->ws, d_out_ids, d_out_off, d_n_tokens, st);
  prof_end(st, 2);
  SWT_HIP(hipGetLastError());
  return SWT_OK;
} SWT_API_CATCH

}  // extern "C"

// swt_wp_encode_naive_dev, and with `draw` swt_wp_encode_naive_dropout_dev: the same routes with the dropout instantiation
static int wp_naive_dev(swt_wp_trie *t, const uint8_t *d_text, uint64_t n_bytes, const uint64_t *d_sent_off, uint64_t n_sent,
                        uint32_t *d_out_ids, uint64_t *d_out_off, uint8_t *d_status, uint64_t *d_n_tokens, const WpDrawArgs *draw,
                        void *stream) {
  if (!t || !d_sent_off || !d_out_off || !d_n_tokens || (n_sent && !d_status) || (n_bytes && (!d_text || !d_out_ids)))
    return fail(SWT_ERR_INVALID, "null argument");
  if (t->H.naive_excess)
    return fail(SWT_ERR_UNSUPPORTED, "a vocabulary token starts with three or more '#' and goes on: NaiveWP.encode_word could emit "
                                     "more tokens than its word has bytes");
  int rc = wp_upload_naive(t);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const uint8_t *d_cls = nullptr;
  if ((rc = device_class_table(&d_cls))) return rc;
  const uint64_t n_tiles = tile_count(n_bytes, kWpTile);
  if (n_tiles > 0x7FFFFFFFull)
    return fail(SWT_ERR_UNSUPPORTED, "text too large for one call (%llu bytes)", (unsigned long long)n_bytes);
  if ((rc = t->ws.reserve(n_bytes, n_sent, n_tiles))) return rc;
  if (n_sent == 0) {
    SWT_HIP(hipMemsetAsync(d_out_off, 0, 8, st));
    SWT_HIP(hipMemsetAsync(d_n_tokens, 0, 8, st));
    return SWT_OK;
  }
  WpNaiveDev N;
  N.T = WpDev{};
  N.T.edges = t->d_edges;
  N.T.edge_bits = t->edge_bits;
  N.tok = t->d_tok;
  N.unk_id = t->H.n_vocab + 1;
  N.max_steps = t->H.sharp_depth + 2;
  const auto launch = [&](unsigned blocks, const uint64_t *plan, uint32_t *ids, const DirectOut &direct) {
    if (draw)
      hipLaunchKernelGGL(wp_naive_kernel<true>, dim3(blocks), dim3(64), 0, st, d_text, n_bytes, d_sent_off, plan, d_cls, N, ids,
                         t->ws.sent_local.as<uint32_t>(), t->ws.tile_tok.as<uint32_t>(), d_status, WpDirectDrop{direct, *draw});
    else
      hipLaunchKernelGGL(wp_naive_kernel<false>, dim3(blocks), dim3(64), 0, st, d_text, n_bytes, d_sent_off, plan, d_cls, N, ids,
                         t->ws.sent_local.as<uint32_t>(), t->ws.tile_tok.as<uint32_t>(), d_status, direct);
  };
  if (n_bytes <= kWpDirectBytes && n_sent <= kWpDirectSents) {
    // one workgroup, one launch, the caller's arrays written by the kernel (DirectOut, swt_tile.h)
    launch(1, nullptr, d_out_ids, DirectOut{d_out_off, d_n_tokens, n_sent});
    SWT_HIP(hipGetLastError());
    return SWT_OK;
  }
  prof_begin(st, 2);
  launch_plan(d_sent_off, n_sent, n_tiles, kWpTile, t->ws.plan.as<uint64_t>(), st);
  prof_begin(st);
  launch((unsigned)n_tiles, t->ws.plan.as<uint64_t>(), t->ws.scratch.as<uint32_t>(), DirectOut{nullptr, nullptr, 0});
  prof_end(st);
  launch_scan_gather(d_sent_off, n_sent, n_tiles, t->ws, d_out_ids, d_out_off, d_n_tokens, st);
  prof_end(st, 2);
  SWT_HIP(hipGetLastError());
  return SWT_OK;
}

// the draw of a dropout call from its three arguments
static int wp_draw_args(uint64_t drop_below, uint64_t seed, uint32_t epoch, WpDrawArgs &d) {
  if (drop_below > (1ull << 32)) return fail(SWT_ERR_INVALID, "drop_below lies in [0, 2^32] (round(p * 2^32))");
  d = WpDrawArgs{drop_below, (uint32_t)seed, (uint32_t)(seed >> 32), epoch};
  return SWT_OK;
}

extern "C" {

int swt_wp_encode_naive_dev(swt_wp_trie *t, const uint8_t *d_text, uint64_t n_bytes, const uint64_t *d_sent_off, uint64_t n_sent,
                            uint32_t *d_out_ids, uint64_t *d_out_off, uint8_t *d_status, uint64_t *d_n_tokens, void *stream) try {
  return wp_naive_dev(t, d_text, n_bytes, d_sent_off, n_sent, d_out_ids, d_out_off, d_status, d_n_tokens, nullptr, stream);
} SWT_API_CATCH

int swt_wp_encode_naive_dropout_dev(swt_wp_trie *t, const uint8_t *d_text, uint64_t n_bytes, const uint64_t *d_sent_off, uint64_t n_sent,
                                    uint32_t *d_out_ids, uint64_t *d_out_off, uint8_t *d_status, uint64_t *d_n_tokens, uint64_t drop_below,
                                    uint64_t seed, uint32_t epoch, void *stream) try {
  WpDrawArgs d;
  if (int rc = wp_draw_args(drop_below, seed, epoch, d)) return rc;
  return wp_naive_dev(t, d_text, n_bytes, d_sent_off, n_sent, d_out_ids, d_out_off, d_status, d_n_tokens, &d, stream);
} SWT_API_CATCH

// FastWP with token spans: swt_wp_encode_dev's direct and tiled paths with the span instantiation of the kernel, the spans and
// word indices through their own scratch runs and launch_gather_spans.  The word-level dedup pipeline is never taken, whatever
// the batch size and SWT_OPT_DEDUP say: a unique chunk is encoded once for all its occurrences and has no position.
int swt_wp_encode_spans_dev(swt_wp_trie *t, const uint8_t *d_text, uint64_t n_bytes, const uint64_t *d_sent_off, uint64_t n_sent,
                            uint32_t *d_out_ids, uint64_t *d_out_off, uint8_t *d_status, uint64_t *d_n_tokens, uint32_t flags,
                            uint32_t *d_spans, uint32_t *d_word, void *stream) try {
  if (!t || !d_sent_off || !d_out_off || !d_n_tokens || !d_spans || (n_sent && !d_status) || (n_bytes && (!d_text || !d_out_ids)))
    return fail(SWT_ERR_INVALID, "null argument");
  if (flags & ~SWT_SPAN_CODEPOINTS) return fail(SWT_ERR_INVALID, "unknown flag");
  int rc = wp_upload_spans(t);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const uint8_t *d_cls = nullptr;
  if ((rc = device_class_table(&d_cls))) return rc;
  const uint64_t n_tiles = tile_count(n_bytes, kWpTile);
  if (n_tiles > 0x7FFFFFFFull)
    return fail(SWT_ERR_UNSUPPORTED, "text too large for one call (%llu bytes)", (unsigned long long)n_bytes);
  if ((rc = t->ws.reserve(n_bytes, n_sent, n_tiles)) || (rc = t->sp_scratch.reserve((n_bytes + 64) * 8)) ||
      (rc = t->wd_scratch.reserve((n_bytes + 64) * 4)))
    return rc;
  if (n_sent == 0) {
    SWT_HIP(hipMemsetAsync(d_out_off, 0, 8, st));
    SWT_HIP(hipMemsetAsync(d_n_tokens, 0, 8, st));
    return SWT_OK;
  }
  const WpDev T = wp_dev(t);
  const WpSpanTab tab{t->d_len, t->H.n_vocab, flags & SWT_SPAN_CODEPOINTS};
  if (n_bytes <= kWpDirectBytes && n_sent <= kWpDirectSents) {
    hipLaunchKernelGGL((wp_encode_kernel<WpSpanLds, WpSpanArgs>), dim3(1), dim3(64), 0, st, d_text, n_bytes, d_sent_off, (const uint64_t *)nullptr, d_cls, T,
                       d_out_ids, t->ws.sent_local.as<uint32_t>(), t->ws.tile_tok.as<uint32_t>(), d_status,
                       DirectOut{d_out_off, d_n_tokens, n_sent}, WpSpanArgs{tab, d_spans, d_word ? d_word : t->wd_scratch.as<uint32_t>()});
    SWT_HIP(hipGetLastError());
    return SWT_OK;
  }
  prof_begin(st, 2);
  launch_plan(d_sent_off, n_sent, n_tiles, kWpTile, t->ws.plan.as<uint64_t>(), st);
  prof_begin(st);
  hipLaunchKernelGGL((wp_encode_kernel<WpSpanLds, WpSpanArgs>), dim3((unsigned)n_tiles), dim3(64), 0, st, d_text, n_bytes, d_sent_off,
                     t->ws.plan.as<uint64_t>(), d_cls, T, t->ws.scratch.as<uint32_t>(), t->ws.sent_local.as<uint32_t>(),
                     t->ws.tile_tok.as<uint32_t>(), d_status, DirectOut{nullptr, nullptr, 0},
                     WpSpanArgs{tab, t->sp_scratch.as<uint32_t>(), t->wd_scratch.as<uint32_t>()});
  prof_end(st);
  launch_scan_gather(d_sent_off, n_sent, n_tiles, t->ws, d_out_ids, d_out_off, d_n_tokens, st);
  launch_gather_spans(d_sent_off, n_tiles, t->ws, t->sp_scratch.as<uint32_t>(), t->wd_scratch.as<uint32_t>(), d_spans, d_word, st);
  prof_end(st, 2);
  SWT_HIP(hipGetLastError());
  return SWT_OK;
} SWT_API_CATCH

int swt_wp_encode_spans_capacity(uint32_t *block, uint32_t *chunk, uint32_t *tile, uint32_t *direct_bytes, uint32_t *direct_sents) try {
  if (block) *block = 64;
  if (chunk) *chunk = kWpCap;
  if (tile) *tile = kWpTile;
  if (direct_bytes) *direct_bytes = (uint32_t)kWpDirectBytes;
  if (direct_sents) *direct_sents = (uint32_t)kWpDirectSents;
  return SWT_OK;
} SWT_API_CATCH

// What the host-call layer (swt_tile.h) needs to know of FastWP (swt_wp_encode_dev) or NaiveWP (swt_wp_encode_naive_dev).
typedef int (*WpEncodeDev)(swt_wp_trie *, const uint8_t *, uint64_t, const uint64_t *, uint64_t, uint32_t *, uint64_t *, uint8_t *,
                           uint64_t *, void *);
static HostEncoder wp_host(swt_wp_trie *t, WpEncodeDev dev) {
  return HostEncoder{[t] { return wp_upload(t); },
                     [t, dev](const uint8_t *d_text, uint64_t n_bytes, const uint64_t *d_off, uint64_t n_sent, uint32_t *d_ids,
                              uint64_t *d_out_off, uint8_t *d_status, uint64_t *d_n_tokens) {
                       return dev(t, d_text, n_bytes, d_off, n_sent, d_ids, d_out_off, d_status, d_n_tokens, nullptr);
                     },
                     kWpDirectBytes, kWpDirectSents, true};
}
static int wp_encode_host(WpEncodeDev dev, swt_wp_trie *t, const uint8_t *text, const uint64_t *sent_off, uint64_t n_sent,
                          uint32_t *out_ids, uint64_t out_cap, uint64_t *out_off, uint8_t *status, uint64_t *n_tokens) {
  if (!t) return fail(SWT_ERR_INVALID, "null argument");
  return host_encode(t->stage, wp_host(t, dev), text, sent_off, n_sent, out_ids, out_cap, out_off, status, n_tokens);
}
static int wp_encode_joined(WpEncodeDev dev, swt_wp_trie *t, const uint8_t *joined, uint64_t n_joined, uint64_t n_sent, uint32_t *out_ids,
                            uint64_t out_cap, uint64_t *out_off, uint8_t *status, uint64_t *n_tokens, uint8_t *need_host) {
  if (!t) return fail(SWT_ERR_INVALID, "null argument");
  return host_encode_joined(t->stage, wp_host(t, dev), joined, n_joined, n_sent, out_ids, out_cap, out_off, status, n_tokens, need_host);
}

int swt_wp_encode(swt_wp_trie *t, const uint8_t *text, const uint64_t *sent_off, uint64_t n_sent, uint32_t *out_ids,
                  uint64_t out_cap, uint64_t *out_off, uint8_t *status, uint64_t *n_tokens) try {
  return wp_encode_host(swt_wp_encode_dev, t, text, sent_off, n_sent, out_ids, out_cap, out_off, status, n_tokens);
} SWT_API_CATCH

// FastWP with token spans, host buffers: the one host-call layer with its optional extra outputs (HostExtra, swt_tile.h).
int swt_wp_encode_spans(swt_wp_trie *t, const uint8_t *text, const uint64_t *sent_off, uint64_t n_sent, uint32_t *out_ids,
                        uint64_t out_cap, uint64_t *out_off, uint8_t *status, uint64_t *n_tokens, uint32_t flags, uint32_t *spans,
                        uint32_t *word) try {
  if (!t || !spans) return fail(SWT_ERR_INVALID, "null argument");
  if (flags & ~SWT_SPAN_CODEPOINTS) return fail(SWT_ERR_INVALID, "unknown flag");
  HostEncoder enc = wp_host(t, swt_wp_encode_dev);
  enc.upload = [t] { return wp_upload_spans(t); };
  enc.dev_extra = [t, flags](const uint8_t *d_text, uint64_t n_bytes, const uint64_t *d_off, uint64_t n, uint32_t *d_ids,
                             uint64_t *d_out_off, uint8_t *d_status, uint64_t *d_n_tokens, uint32_t *d_spans, uint32_t *d_word) {
    return swt_wp_encode_spans_dev(t, d_text, n_bytes, d_off, n, d_ids, d_out_off, d_status, d_n_tokens, flags, d_spans, d_word, nullptr);
  };
  const HostExtra extra{spans, word};
  return host_encode(t->stage, enc, text, sent_off, n_sent, out_ids, out_cap, out_off, status, n_tokens, &extra);
} SWT_API_CATCH

int swt_wp_encode_naive(swt_wp_trie *t, const uint8_t *text, const uint64_t *sent_off, uint64_t n_sent, uint32_t *out_ids,
                        uint64_t out_cap, uint64_t *out_off, uint8_t *status, uint64_t *n_tokens) try {
  return wp_encode_host(swt_wp_encode_naive_dev, t, text, sent_off, n_sent, out_ids, out_cap, out_off, status, n_tokens);
} SWT_API_CATCH

// MaxMatch-Dropout, host buffers: the one host-call layer with the dropout `_dev` form behind it.  No joined form: a draw goes by
// a byte offset in the text the call is given.
int swt_wp_encode_naive_dropout(swt_wp_trie *t, const uint8_t *text, const uint64_t *sent_off, uint64_t n_sent, uint32_t *out_ids,
                                uint64_t out_cap, uint64_t *out_off, uint8_t *status, uint64_t *n_tokens, uint64_t drop_below,
                                uint64_t seed, uint32_t epoch) try {
  if (!t) return fail(SWT_ERR_INVALID, "null argument");
  WpDrawArgs d;
  if (int rc = wp_draw_args(drop_below, seed, epoch, d)) return rc;
  HostEncoder enc = wp_host(t, swt_wp_encode_naive_dev);
  enc.dev = [t, d](const uint8_t *d_text, uint64_t n_bytes, const uint64_t *d_off, uint64_t n, uint32_t *d_ids, uint64_t *d_out_off,
                   uint8_t *d_status, uint64_t *d_n_tokens) {
    return wp_naive_dev(t, d_text, n_bytes, d_off, n, d_ids, d_out_off, d_status, d_n_tokens, &d, nullptr);
  };
  return host_encode(t->stage, enc, text, sent_off, n_sent, out_ids, out_cap, out_off, status, n_tokens);
} SWT_API_CATCH

// list[str] joined with U+0000 -> ids, the prepared text staying on the device (see swt_bpe_encode_joined).
// *n_tokens = UINT64_MAX on return: a sentence needs the host's str.lower() and nothing was encoded.
int swt_wp_encode_joined(swt_wp_trie *t, const uint8_t *joined, uint64_t n_joined, uint64_t n_sent, uint32_t *out_ids, uint64_t out_cap,
                         uint64_t *out_off, uint8_t *status, uint64_t *n_tokens, uint8_t *need_host) try {
  return wp_encode_joined(swt_wp_encode_dev, t, joined, n_joined, n_sent, out_ids, out_cap, out_off, status, n_tokens, need_host);
} SWT_API_CATCH

int swt_wp_encode_naive_joined(swt_wp_trie *t, const uint8_t *joined, uint64_t n_joined, uint64_t n_sent, uint32_t *out_ids,
                               uint64_t out_cap, uint64_t *out_off, uint8_t *status, uint64_t *n_tokens, uint8_t *need_host) try {
  return wp_encode_joined(swt_wp_encode_naive_dev, t, joined, n_joined, n_sent, out_ids, out_cap, out_off, status, n_tokens, need_host);
} SWT_API_CATCH

}  // extern "C"
