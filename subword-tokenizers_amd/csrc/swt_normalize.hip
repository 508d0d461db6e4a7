// swt_normalize.hip -- the BERT normalizer on the device: clean_text, handle_chinese_chars, strip_accents, lowercase over raw
// UTF-8, with the alignment of every output code point back to its source.  Semantics: include/swt.h ("The normalizer");
// tests/normalizer_cases.py holds them in Python; the tables: tools/gen_normalize_table.py; the design and its measurements:
// DESIGN.md 4.18.
//
// A stream compaction and expansion: a code point may vanish (a control character, a mark), shrink ('é' -> 'e'), grow ('İ' ->
// 'i' + U+0307, a Hangul syllable -> its jamo) or gain neighbours (an ideograph -> ' c ').  Two passes over tiles of 1 KiB, one
// WAVE per tile, sixteen bytes per lane from one 128-bit load:
//   plan   norm_kernel<false, *>: every lane expands the code points whose lead byte it holds and counts output bytes, output
//          code points and source code points; a wave reduction leaves the tile's counts, two scans make bases of them
//   rows   norm_kernel<true, kAlign>: the same decode (the tile is read a second time, out of L2 when the text is of that size), a
//          wave-wide exclusive scan of the lanes' counts gives every lane its place, the bytes are staged in LDS at the
//          place's offset plus the output address's low four bits, so that the wave then stores whole aligned 16-byte chunks;
//          only the first and the last chunk of a tile go byte by byte.  The sentences that start in the tile get their new byte
//          offset and, with kAlign, their code-point offsets from the owner lane's counts, which travel by shuffle as nibbles.
// A lane sees a window of 24 bytes -- four before its sixteen and four behind, from its neighbours by shuffle -- so that a code
// point that straddles a lane or a tile is decoded by the lane of its lead byte alone and nobody else emits its bytes.
// The four flags become masks before the launch (NormArgs: m_flags, m_kind, form): the lanes branch on data, not on flags.
#include <mutex>

#include "swt_batch.h"
#include "unicode_lower.inc"
#include "unicode_normalize.inc"

namespace swt {

constexpr uint32_t kNmTile = 1024, kNmLane = 16, kNmWaves = 4, kNmThreads = 64 * kNmWaves;
// what one tile can emit: every whole code point at most SWT_NORM_MAX_BYTE_RATIO bytes per source byte, and the one whose lead
// byte is the tile's last; 16 more for the shift to the output's alignment, rounded to whole chunks
constexpr uint32_t kNmStage = (SWT_NORM_MAX_BYTE_RATIO * kNmTile + SWT_NORM_MAX_BYTES + 16 + 15) / 16 * 16;
constexpr uint32_t kNmSeq = 3;  // code points of one expansion, the spaces around an ideograph apart
static_assert(SWT_NORM_MAX_CPS <= kNmSeq && SWT_NORM_MAX_BYTES <= 15 && kNmSeq + 2 <= 15, "a lane keeps a code point's counts in a nibble");
static_assert(kNmLane * 15 < 256, "the nibbles of a lane are summed in bytes");
static_assert(SWT_NORM_MAX_CP_RATIO == 1, "out_align is sized for n_bytes + 2 code points");

// a table entry: the flags of steps 1 to 3, a kind, and 21 bits of payload
constexpr uint32_t kNmDrop = 1, kNmSpace = 2, kNmCjk = 4, kNmMark = 8;
constexpr uint32_t kNmKindShift = 4, kNmLower = 1, kNmRecord = 2, kNmPayload = 8;
constexpr uint32_t kNmFlagsAll = SWT_NORMALIZE_CLEAN_TEXT | SWT_NORMALIZE_CHINESE_CHARS | SWT_NORMALIZE_STRIP_ACCENTS | SWT_NORMALIZE_LOWERCASE;

static std::vector<uint32_t> g_norm;
static std::once_flag g_norm_once;
static uint32_t *g_norm_dev = nullptr, *g_norm_seq_dev = nullptr;
static std::mutex g_norm_mu;

static const uint32_t *host_norm_table() {
  std::call_once(g_norm_once, [] {
    g_norm.assign(kNumCodePoints, 0u);
    auto mark = [](const unsigned int (*r)[2], unsigned int n, uint32_t bit) {
      for (unsigned int i = 0; i < n; i++)
        for (uint32_t c = r[i][0]; c <= r[i][1] && c < kNumCodePoints; c++) g_norm[c] |= bit;
    };
    mark(SWT_NORM_DROP, SWT_NORM_DROP_N, kNmDrop);
    mark(SWT_NORM_SPACE, SWT_NORM_SPACE_N, kNmSpace);
    mark(SWT_NORM_CJK, SWT_NORM_CJK_N, kNmCjk);
    mark(SWT_NORM_MARK, SWT_NORM_MARK_N, kNmMark);
    for (unsigned int i = 0; i < SWT_LOWER_NPAIRS; i++)
      g_norm[SWT_LOWER_PAIRS[i][0]] |= kNmLower << kNmKindShift | SWT_LOWER_PAIRS[i][1] << kNmPayload;
    for (unsigned int i = 0; i < SWT_NORM_SEQ_CP_N; i++) {  // a record speaks for all three forms, the lowercase pair included
      uint32_t &e = g_norm[SWT_NORM_SEQ_CP[i][0]];
      e = (e & 15u) | kNmRecord << kNmKindShift | SWT_NORM_SEQ_CP[i][1] << kNmPayload;
    }
  });
  return g_norm.data();
}

static int device_norm_table(const uint32_t **d, const uint32_t **d_seq) {
  std::lock_guard<std::mutex> lk(g_norm_mu);
  if (!g_norm_dev) {
    const uint32_t *h = host_norm_table();
    uint32_t *tab = nullptr, *seq = nullptr;
    SWT_HIP(hipMalloc((void **)&tab, (size_t)kNumCodePoints * 4));
    SWT_HIP(hipMalloc((void **)&seq, (size_t)SWT_NORM_SEQ_N * 4 + 16));
    SWT_HIP(hipMemcpy(tab, h, (size_t)kNumCodePoints * 4, hipMemcpyHostToDevice));
    SWT_HIP(hipMemcpy(seq, SWT_NORM_SEQ, (size_t)SWT_NORM_SEQ_N * 4, hipMemcpyHostToDevice));
    g_norm_seq_dev = seq;
    g_norm_dev = tab;
  }
  *d = g_norm_dev;
  *d_seq = g_norm_seq_dev;
  return SWT_OK;
}

struct NormArgs {
  const uint8_t *text;
  uint64_t n_bytes;
  const uint64_t *sent_off;
  uint64_t n_sent, n_tiles;
  const uint32_t *table, *seq;
  // the call's flags as masks: the entry flags that act, the kinds that act (none when neither strip_accents nor lowercase is
  // set), and where a record keeps the form asked for: its length's shift in the header, and which lengths lie before it
  uint32_t m_flags, m_kind, lower, hangul, len_shift, skip1, skip2;
  // plan: the tile's output bytes; its output code points << 32 | its source code points
  uint32_t *tile_bytes;
  unsigned long long *tile_cps;
  // rows: the scans of both (local to a group of 1024 tiles, and the groups' bases), tile -> first sentence
  const uint32_t *byte_local;
  const unsigned long long *byte_base, *cp_local, *cp_base;
  const uint64_t *plan;
  uint8_t *out_text;
  uint64_t text_cap;
  uint64_t *out_off, *out_cp_off, *src_cp_off;
  uint32_t *out_align;
  uint64_t align_cap;
};

// the lane's window: byte k of its sixteen for k in [-4, 20)
__device__ __forceinline__ uint32_t nm_byte(const uint32_t (&w)[6], int k) { return (w[(k + 4) >> 2] >> (((k + 4) & 3) * 8)) & 0xFFu; }

__device__ __forceinline__ uint32_t nm_u8len(uint32_t c) { return c < 0x80u ? 1u : c < 0x800u ? 2u : c < 0x10000u ? 3u : 4u; }

struct NormStage {  // where a lane's bytes go (rows)
  uint8_t *bytes;
  uint32_t pos;
  __device__ __forceinline__ void put(uint32_t b) {
    if (pos < kNmStage) bytes[pos] = (uint8_t)b;
    pos++;
  }
  __device__ __forceinline__ void put_cp(uint32_t c) {
    if (c < 0x80u) { put(c); return; }
    if (c < 0x800u) { put(0xC0u | (c >> 6)); put(0x80u | (c & 0x3Fu)); return; }
    if (c < 0x10000u) { put(0xE0u | (c >> 12)); put(0x80u | ((c >> 6) & 0x3Fu)); put(0x80u | (c & 0x3Fu)); return; }
    put(0xF0u | (c >> 18)); put(0x80u | ((c >> 12) & 0x3Fu)); put(0x80u | ((c >> 6) & 0x3Fu)); put(0x80u | (c & 0x3Fu));
  }
};

// What byte i of the lane's sixteen emits: (output code points, output bytes); with kEmit the bytes go to the stage.
//   a continuation byte that a lead byte up to three before it claims (its length says so): nothing, the lead's lane emits it
//   any other continuation byte: itself, no code point
//   a lead byte without all its continuation bytes, 0xF8.., a value past U+10FFFF, an overlong form: the bytes as they are, one
//   code point (a surrogate's three bytes decode and are looked up like any code point: category Cs)
//   a code point: its expansion under the masks
template <bool kEmit>
__device__ __forceinline__ uint2 norm_unit(const uint32_t (&w)[6], int i, const NormArgs &A, NormStage &st) {
  const uint32_t b = nm_byte(w, i);
  if ((b & 0xC0u) == 0x80u) {
    bool claimed = false;
#pragma unroll
    for (int k = 3; k >= 1; k--) {  // the nearest byte before that is no continuation byte decides
      const uint32_t p = nm_byte(w, i - k);
      if ((p & 0xC0u) != 0x80u) claimed = (uint32_t)utf8_len((uint8_t)p) > (uint32_t)k;
    }
    if (claimed) return make_uint2(0, 0);
    if constexpr (kEmit) st.put(b);
    return make_uint2(0, 1);
  }
  const uint32_t len = (uint32_t)utf8_len((uint8_t)b);
  uint32_t run = 0, cp = b & (0xFFu >> (len > 1 ? len + 1 : 0));
#pragma unroll
  for (int k = 1; k <= 3; k++) {
    const uint32_t c = nm_byte(w, i + k);
    if ((uint32_t)k < len && run == (uint32_t)(k - 1) && (c & 0xC0u) == 0x80u) {
      run = k;
      cp = (cp << 6) | (c & 0x3Fu);
    }
  }
  const uint32_t least = len == 2 ? 0x80u : len == 3 ? 0x800u : len == 4 ? 0x10000u : 0u;  // below it the form is overlong
  if (run + 1 != len || b >= 0xF8u || cp >= kNumCodePoints || cp < least) {
    if constexpr (kEmit) {
      st.put(b);
#pragma unroll
      for (int k = 1; k <= 3; k++)
        if ((uint32_t)k <= run) st.put(nm_byte(w, i + k));
    }
    return make_uint2(1, 1 + run);
  }
  const uint32_t e = A.table[cp], f = e & A.m_flags;
  if (f & (kNmDrop | kNmMark)) return make_uint2(0, 0);
  uint32_t seq[kNmSeq] = {cp, 0, 0}, n = 1;
  if (f & kNmSpace) {
    seq[0] = 0x20u;
  } else {
    const uint32_t kind = (e >> kNmKindShift) & A.m_kind;
    if (kind == kNmLower) {
      if (A.lower) seq[0] = e >> kNmPayload;
    } else if (kind == kNmRecord) {
      const uint32_t r = e >> kNmPayload, hdr = A.seq[r];
      const uint32_t first = r + 1 + ((hdr & 0xFFu) & A.skip1) + (((hdr >> 8) & 0xFFu) & A.skip2);
      n = (hdr >> A.len_shift) & 0xFFu;
      if (n > kNmSeq) n = kNmSeq;
#pragma unroll
      for (uint32_t k = 0; k < kNmSeq; k++)
        if (k < n) seq[k] = A.seq[first + k];
    } else if (A.hangul && cp - 0xAC00u < 11172u) {  // a syllable -> its jamo, computed (no jamo is a mark or has a lowercase)
      const uint32_t s = cp - 0xAC00u, t = s % 28u;
      seq[0] = 0x1100u + s / 588u;
      seq[1] = 0x1161u + (s % 588u) / 28u;
      seq[2] = 0x11A7u + t;
      n = t ? 3u : 2u;
    }
  }
  const uint32_t wrap = (f & kNmCjk) ? 1u : 0u;
  uint32_t bytes = 2 * wrap;
#pragma unroll
  for (uint32_t k = 0; k < kNmSeq; k++)
    if (k < n) bytes += nm_u8len(seq[k]);
  if constexpr (kEmit) {
    if (wrap) st.put(0x20u);
#pragma unroll
    for (uint32_t k = 0; k < kNmSeq; k++)
      if (k < n) st.put_cp(seq[k]);
    if (wrap) st.put(0x20u);
  }
  return make_uint2(n + 2 * wrap, bytes);
}

// the sum of the nibbles of x below nibble i (i <= 16; every nibble at most 15, so a byte of the fold at most 30 and the sum
// at most 240)
__device__ __forceinline__ uint32_t nm_nibbles_below(unsigned long long x, uint32_t i) {
  x &= i >= 16 ? ~0ull : ((1ull << (4 * i)) - 1ull);
  x = (x & 0x0F0F0F0F0F0F0F0Full) + ((x >> 4) & 0x0F0F0F0F0F0F0F0Full);
  return (uint32_t)((x * 0x0101010101010101ull) >> 56);
}

template <bool kRows, bool kAlign>
__global__ __launch_bounds__(kNmThreads) void norm_kernel(NormArgs A) {
  __shared__ uint4 s_stage[kRows ? kNmWaves : 1][kRows ? kNmStage / 16 : 1];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t t = (uint64_t)blockIdx.x * kNmWaves + wave;
  if (t >= A.n_tiles) return;  // the whole wave: nothing below crosses waves
  const uint64_t base = t * kNmTile, g0 = base + (uint64_t)lane * kNmLane;
  const int avail = g0 >= A.n_bytes ? 0 : (A.n_bytes - g0 < kNmLane ? (int)(A.n_bytes - g0) : (int)kNmLane);

  // the window: bytes past the text's end and before its start read as zero, which is no continuation byte
  uint32_t w[6] = {0, 0, 0, 0, 0, 0};
  if (avail == (int)kNmLane && (reinterpret_cast<uintptr_t>(A.text + g0) & 15) == 0) {
    const uint4 v = *reinterpret_cast<const uint4 *>(A.text + g0);
    w[1] = v.x; w[2] = v.y; w[3] = v.z; w[4] = v.w;
  } else {
    for (int k = 0; k < avail; k++) w[1 + (k >> 2)] |= (uint32_t)A.text[g0 + k] << ((k & 3) * 8);
  }
  w[0] = __shfl_up(w[4], 1, 64);
  w[5] = __shfl_down(w[1], 1, 64);
  if (lane == 0) {
    w[0] = 0;
    for (int k = 1; k <= 3; k++)
      if (g0 >= (uint64_t)k && g0 - k < A.n_bytes) w[0] |= (uint32_t)A.text[g0 - k] << ((4 - k) * 8);
  }
  if (lane == 63) {
    w[5] = 0;
    for (int k = 0; k < 3; k++)
      if (g0 + kNmLane + k < A.n_bytes) w[5] |= (uint32_t)A.text[g0 + kNmLane + k] << (k * 8);
  }

  // the counts of the lane's sixteen bytes: a nibble each of output bytes and output code points, a bit for a source code point
  unsigned long long nib_bytes = 0, nib_cps = 0;
  uint32_t leads = 0, n_bytes = 0, n_cps = 0;
  NormStage none{nullptr, kNmStage};
#pragma unroll
  for (int i = 0; i < (int)kNmLane; i++) {
    if (i >= avail) continue;
    const uint2 u = norm_unit<false>(w, i, A, none);
    nib_cps |= (unsigned long long)u.x << (4 * i);
    nib_bytes |= (unsigned long long)u.y << (4 * i);
    if ((nm_byte(w, i) & 0xC0u) != 0x80u) leads |= 1u << i;
    n_cps += u.x;
    n_bytes += u.y;
  }
  // bytes | output code points << 21 | source code points << 42: a tile has at most kNmStage, kNmTile + 2 and kNmTile of them
  const unsigned long long mine = (unsigned long long)n_bytes | (unsigned long long)n_cps << 21 | (unsigned long long)__popc(leads) << 42;
  unsigned long long incl = mine;
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long y = __shfl_up(incl, d, 64);
    if (lane >= (uint32_t)d) incl += y;
  }
  const unsigned long long total = __shfl(incl, 63, 64);
  const uint32_t tile_bytes = (uint32_t)(total & 0x1FFFFFu), tile_cps = (uint32_t)((total >> 21) & 0x1FFFFFu), tile_src = (uint32_t)(total >> 42);
  if constexpr (!kRows) {
    if (lane == 0) {
      A.tile_bytes[t] = tile_bytes;
      A.tile_cps[t] = (unsigned long long)tile_cps << 32 | tile_src;
    }
    return;
  } else {
    const unsigned long long excl = incl - mine;
    const uint64_t out_base = A.byte_base[t >> 10] + A.byte_local[t];
    const unsigned long long cps = A.cp_base[t >> 10] + A.cp_local[t];
    const uint64_t cp_base = cps >> 32, src_base = cps & 0xFFFFFFFFull;
    // the stage holds the tile's bytes from the 16-byte boundary below their first address on
    uint8_t *stage = reinterpret_cast<uint8_t *>(s_stage[wave]);
    const uint32_t shift = (uint32_t)(reinterpret_cast<uintptr_t>(A.out_text + out_base) & 15);
    NormStage st{stage, shift + (uint32_t)(excl & 0x1FFFFFu)};
    uint64_t cp_at = cp_base + ((excl >> 21) & 0x1FFFFFu), src_at = src_base + (excl >> 42);
#pragma unroll
    for (int i = 0; i < (int)kNmLane; i++) {
      if (i >= avail) continue;
      const uint2 u = norm_unit<true>(w, i, A, st);
      if constexpr (kAlign) {
        for (uint32_t k = 0; k < u.x; k++)
          if (cp_at + k < A.align_cap) A.out_align[cp_at + k] = (uint32_t)src_at;
        cp_at += u.x;
        src_at += (leads >> i) & 1u;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // whole chunks leave as 16-byte stores; the chunks that hold the tile's first and last bytes go byte by byte
    uint8_t *const out0 = A.out_text + out_base - shift;  // the address of the stage's byte 0
    const uint32_t end = shift + tile_bytes < kNmStage ? shift + tile_bytes : kNmStage;
    for (uint32_t c = lane * 16; c < end; c += 64 * 16) {
      if (c >= shift && c + 16 <= end && out_base + c + 16 - shift <= A.text_cap) {
        *reinterpret_cast<uint4 *>(out0 + c) = s_stage[wave][c >> 4];
      } else {
        for (uint32_t k = c < shift ? shift : c; k < c + 16 && k < end; k++)
          if (out_base + k - shift < A.text_cap) out0[k] = stage[k];
      }
    }
    // the sentences that start in this tile: the counts before their first byte, from the lane that holds it
    const uint64_t s_lo = A.plan[t], s_hi = A.plan[t + 1];
    for (uint64_t s0 = s_lo; s0 < s_hi; s0 += 64) {  // uniform over the wave: every lane meets every shuffle
      const uint64_t s = s0 + lane;
      const uint64_t g = s < s_hi ? A.sent_off[s] : base;
      const uint32_t rel = g < base ? 0u : (g - base > kNmTile ? kNmTile : (uint32_t)(g - base));
      const uint32_t owner = rel >> 4 > 63 ? 63 : rel >> 4, i = rel - owner * 16;  // rel == kNmTile: all of lane 63
      const unsigned long long e = __shfl(excl, owner, 64), nb = __shfl(nib_bytes, owner, 64), nc = __shfl(nib_cps, owner, 64);
      const uint32_t ld = __shfl(leads, owner, 64);
      if (s < s_hi) {
        A.out_off[s] = out_base + (e & 0x1FFFFFu) + nm_nibbles_below(nb, i);
        if constexpr (kAlign) {
          A.out_cp_off[s] = cp_base + ((e >> 21) & 0x1FFFFFu) + nm_nibbles_below(nc, i);
          A.src_cp_off[s] = src_base + (e >> 42) + __popc(ld & ((1u << i) - 1u));
        }
      }
    }
    if (t == A.n_tiles - 1 && lane == 0) {
      A.out_off[A.n_sent] = out_base + tile_bytes;
      if constexpr (kAlign) {
        A.out_cp_off[A.n_sent] = cp_base + tile_cps;
        A.src_cp_off[A.n_sent] = src_base + tile_src;
      }
    }
  }
}

// the totals of the plan: info[0] is the byte scan's own; this splits the packed total of the other scan
__global__ void norm_info_kernel(const unsigned long long *__restrict__ packed, uint64_t *__restrict__ info) {
  info[1] = *packed >> 32;
  info[2] = *packed & 0xFFFFFFFFull;
}

__global__ void norm_zero_kernel(uint64_t *__restrict__ p, uint64_t n) {  // (no hipMemsetAsync: a caller may capture the stream)
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = 0;
}

// One thread per token: the token's span from code points of the normalised text to code points of the original.
__global__ __launch_bounds__(256) void norm_spans_kernel(uint32_t *__restrict__ spans, uint64_t n_cap, const uint64_t *__restrict__ tok_off,
                                                         uint64_t n_sent, const uint32_t *__restrict__ align,
                                                         const uint64_t *__restrict__ cp_off, const uint64_t *__restrict__ src_cp_off) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_cap || k >= tok_off[n_sent]) return;
  uint64_t lo = 0, hi = n_sent;  // the text of token k: the last one whose first token is at or before k
  while (lo + 1 < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if (tok_off[mid] <= k) lo = mid; else hi = mid;
  }
  const uint64_t first = cp_off[lo], n = cp_off[lo + 1] - first, src = src_cp_off[lo], n_src = src_cp_off[lo + 1] - src;
  uint64_t a = spans[2 * k], b = spans[2 * k + 1];
  if (b > n) b = n;
  if (a > b) a = b;
  const uint32_t na = a < n ? (uint32_t)(align[first + a] - src) : (uint32_t)n_src;
  spans[2 * k] = na;
  spans[2 * k + 1] = b > a ? (uint32_t)(align[first + b - 1] - src) + 1u : na;
}

// Between a plan and its rows: the tiles' counts and their scans, and the arguments the plan was made for.  Grow-only and shared
// by all calls of the process, as the scan workspace of the row kernels.
struct NormWorkspace {
  TileWorkspace tiles;  // plan = tile -> first sentence, tile_tok = the byte counts, tile_base / blk = their scan
  DevBuf cps, cp_local, cp_blk, total;
  const void *text = nullptr, *sent_off = nullptr;
  uint64_t n_bytes = 0, n_sent = 0;
  uint32_t flags = 0;
  int reserve(uint64_t n_tiles) {
    int rc;
    if ((rc = tiles.reserve(0, 0, n_tiles))) return rc;
    if ((rc = cps.reserve((n_tiles + 1) * 8)) || (rc = cp_local.reserve((n_tiles + 1) * 8)) || (rc = total.reserve(16))) return rc;
    const void *before = cp_blk.p;
    if ((rc = cp_blk.reserve((2 * ((n_tiles + 1023) / 1024) + 4) * 8))) return rc;
    if (cp_blk.p != before) {  // the ticket of a new buffer, as TileWorkspace::reserve
      SWT_HIP(hipMemset(cp_blk.p, 0, 8));
      SWT_HIP(hipDeviceSynchronize());
    }
    return SWT_OK;
  }
};
static NormWorkspace g_norm_ws;

static int norm_args(NormArgs &A, const uint8_t *d_text, uint64_t n_bytes, const uint64_t *d_sent_off, uint64_t n_sent, uint32_t flags) {
  if (flags & ~(kNmFlagsAll | SWT_NORMALIZE_ALIGN)) return fail(SWT_ERR_INVALID, "flags: unknown flag");
  if (!d_sent_off) return fail(SWT_ERR_INVALID, "null argument: sent_off");
  if (n_bytes && !d_text) return fail(SWT_ERR_INVALID, "null argument: text");
  if (n_bytes > 0x7FFFFFFFull) return fail(SWT_ERR_UNSUPPORTED, "n_bytes: 2^31 bytes or more in one call");
  if (n_sent + 1 > 0x7FFFFFFFull) return fail(SWT_ERR_UNSUPPORTED, "too many sentences for one call");
  if (!bt_aligned(8, {d_sent_off})) return fail(SWT_ERR_INVALID, "an array is not aligned to its element type");
  int rc = ensure_device();
  if (rc) return rc;
  A = NormArgs{};
  A.text = d_text; A.n_bytes = n_bytes; A.sent_off = d_sent_off; A.n_sent = n_sent;
  A.n_tiles = (n_bytes + kNmTile - 1) / kNmTile;
  if ((rc = device_norm_table(&A.table, &A.seq))) return rc;
  const bool strip = flags & SWT_NORMALIZE_STRIP_ACCENTS, lower = flags & SWT_NORMALIZE_LOWERCASE;
  const uint32_t form = (strip ? 2u : 0u) | (lower ? 1u : 0u);
  A.m_flags = ((flags & SWT_NORMALIZE_CLEAN_TEXT) ? kNmDrop | kNmSpace : 0u) | ((flags & SWT_NORMALIZE_CHINESE_CHARS) ? kNmCjk : 0u) |
              (strip ? kNmMark : 0u);
  A.m_kind = form ? 3u : 0u;
  A.lower = lower;
  A.hangul = strip;
  A.len_shift = form ? 8 * (form - 1) : 0;
  A.skip1 = form > 1 ? 0xFFu : 0u;
  A.skip2 = form > 2 ? 0xFFu : 0u;
  return SWT_OK;
}

}  // namespace swt

using namespace swt;

extern "C" {

int swt_normalize_capacity(uint32_t *tile_bytes, uint32_t *lane_bytes, uint32_t *max_cps, uint32_t *max_bytes) try {
  if (tile_bytes) *tile_bytes = kNmTile;
  if (lane_bytes) *lane_bytes = kNmLane;
  if (max_cps) *max_cps = SWT_NORM_MAX_CPS;
  if (max_bytes) *max_bytes = SWT_NORM_MAX_BYTES;
  return SWT_OK;
} SWT_API_CATCH

int swt_normalize_plan_dev(const uint8_t *d_text, uint64_t n_bytes, const uint64_t *d_sent_off, uint64_t n_sent, uint32_t flags,
                           uint64_t *d_info, void *stream) try {
  NormArgs A;
  int rc = norm_args(A, d_text, n_bytes, d_sent_off, n_sent, flags);
  if (rc) return rc;
  if (!d_info) return fail(SWT_ERR_INVALID, "null argument: info");
  if (flags & SWT_NORMALIZE_ALIGN) return fail(SWT_ERR_INVALID, "flags: SWT_NORMALIZE_ALIGN is a flag of the rows");
  hipStream_t st = (hipStream_t)stream;
  NormWorkspace &W = g_norm_ws;
  W.text = nullptr;  // no plan stands until this one is enqueued
  if (!n_bytes) {
    hipLaunchKernelGGL(norm_zero_kernel, dim3(1), dim3(64), 0, st, d_info, (uint64_t)3);
  } else {
    if ((rc = W.reserve(A.n_tiles))) return rc;
    A.tile_bytes = W.tiles.tile_tok.as<uint32_t>();
    A.tile_cps = W.cps.as<unsigned long long>();
    hipLaunchKernelGGL((norm_kernel<false, false>), dim3((unsigned)((A.n_tiles + kNmWaves - 1) / kNmWaves)), dim3(kNmThreads), 0, st, A);
    launch_scan_only(A.n_tiles, W.tiles, d_info, st);
    launch_scan_u64(A.n_tiles, A.tile_cps, W.cp_local.as<unsigned long long>(), W.cp_blk.as<unsigned long long>(), W.total.as<uint64_t>(), st);
    hipLaunchKernelGGL(norm_info_kernel, dim3(1), dim3(1), 0, st, W.total.as<unsigned long long>(), d_info);
    launch_plan(d_sent_off, n_sent, A.n_tiles, kNmTile, W.tiles.plan.as<uint64_t>(), st);
  }
  SWT_HIP(hipGetLastError());
  W.text = d_text; W.sent_off = d_sent_off; W.n_bytes = n_bytes; W.n_sent = n_sent; W.flags = flags & kNmFlagsAll;
  return SWT_OK;
} SWT_API_CATCH

int swt_normalize_rows_dev(const uint8_t *d_text, uint64_t n_bytes, const uint64_t *d_sent_off, uint64_t n_sent, uint32_t flags,
                           uint8_t *d_out_text, uint64_t text_cap, uint64_t *d_out_off, uint64_t *d_out_cp_off, uint64_t *d_src_cp_off,
                           uint32_t *d_out_align, uint64_t align_cap, void *stream) try {
  NormArgs A;
  int rc = norm_args(A, d_text, n_bytes, d_sent_off, n_sent, flags);
  if (rc) return rc;
  const bool align = flags & SWT_NORMALIZE_ALIGN;
  if (!d_out_off) return fail(SWT_ERR_INVALID, "null argument: out_off");
  if (text_cap && !d_out_text) return fail(SWT_ERR_INVALID, "null argument: out_text");
  if (align && (!d_out_cp_off || !d_src_cp_off || (align_cap && !d_out_align))) return fail(SWT_ERR_INVALID, "null argument: an output of SWT_NORMALIZE_ALIGN");
  if (!bt_aligned(8, {d_out_off, d_out_cp_off, d_src_cp_off}) || !bt_aligned(4, {d_out_align}))
    return fail(SWT_ERR_INVALID, "an array is not aligned to its element type");
  NormWorkspace &W = g_norm_ws;
  if (W.text != d_text || W.sent_off != d_sent_off || W.n_bytes != n_bytes || W.n_sent != n_sent || W.flags != (flags & kNmFlagsAll))
    return fail(SWT_ERR_INVALID, "the last swt_normalize_plan_dev was not made for these arguments");
  hipStream_t st = (hipStream_t)stream;
  if (!n_bytes) {
    const unsigned grid = (unsigned)((n_sent + 1 + 255) / 256);
    hipLaunchKernelGGL(norm_zero_kernel, dim3(grid), dim3(256), 0, st, d_out_off, n_sent + 1);
    if (align) {
      hipLaunchKernelGGL(norm_zero_kernel, dim3(grid), dim3(256), 0, st, d_out_cp_off, n_sent + 1);
      hipLaunchKernelGGL(norm_zero_kernel, dim3(grid), dim3(256), 0, st, d_src_cp_off, n_sent + 1);
    }
  } else {
    const uint64_t nb = (A.n_tiles + 1023) / 1024;
    A.byte_local = W.tiles.tile_base.as<uint32_t>();
    A.byte_base = W.tiles.blk.as<unsigned long long>() + 1 + nb;
    A.cp_local = W.cp_local.as<unsigned long long>();
    A.cp_base = W.cp_blk.as<unsigned long long>() + 1 + nb;
    A.plan = W.tiles.plan.as<uint64_t>();
    A.out_text = d_out_text; A.text_cap = text_cap; A.out_off = d_out_off;
    A.out_cp_off = d_out_cp_off; A.src_cp_off = d_src_cp_off; A.out_align = d_out_align; A.align_cap = align_cap;
    const dim3 grid((unsigned)((A.n_tiles + kNmWaves - 1) / kNmWaves));
    if (align) hipLaunchKernelGGL((norm_kernel<true, true>), grid, dim3(kNmThreads), 0, st, A);
    else hipLaunchKernelGGL((norm_kernel<true, false>), grid, dim3(kNmThreads), 0, st, A);
  }
  SWT_HIP(hipGetLastError());
  return SWT_OK;
} SWT_API_CATCH

int swt_normalize_spans_dev(uint32_t *d_spans, uint64_t n_cap, const uint64_t *d_tok_off, uint64_t n_sent, const uint32_t *d_align,
                            const uint64_t *d_cp_off, const uint64_t *d_src_cp_off, void *stream) try {
  if (!d_tok_off || !d_cp_off || !d_src_cp_off) return fail(SWT_ERR_INVALID, "null argument: an offset array");
  if (n_cap && (!d_spans || !d_align)) return fail(SWT_ERR_INVALID, "null argument: spans or align");
  if (!bt_aligned(8, {d_tok_off, d_cp_off, d_src_cp_off}) || !bt_aligned(4, {d_spans, d_align}))
    return fail(SWT_ERR_INVALID, "an array is not aligned to its element type");
  if (n_cap > 0xFFFFFFFFull * 256) return fail(SWT_ERR_UNSUPPORTED, "n_cap: too many tokens for one call");
  int rc = ensure_device();
  if (rc) return rc;
  if (!n_cap || !n_sent) return SWT_OK;
  hipLaunchKernelGGL(norm_spans_kernel, dim3((unsigned)((n_cap + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_spans, n_cap, d_tok_off,
                     n_sent, d_align, d_cp_off, d_src_cp_off);
  SWT_HIP(hipGetLastError());
  return SWT_OK;
} SWT_API_CATCH

static int norm_check_host(const uint8_t *text, const uint64_t *sent_off, uint64_t n_sent) {
  if (!sent_off) return fail(SWT_ERR_INVALID, "null argument: sent_off");
  if (sent_off[0] != 0) return fail(SWT_ERR_INVALID, "sent_off[0] must be 0");
  for (uint64_t s = 0; s < n_sent; s++)
    if (sent_off[s] > sent_off[s + 1]) return fail(SWT_ERR_INVALID, "sentence offsets must be non-decreasing");
  if (sent_off[n_sent] && !text) return fail(SWT_ERR_INVALID, "null argument: text");
  return SWT_OK;
}

int swt_normalize_plan(const uint8_t *text, const uint64_t *sent_off, uint64_t n_sent, uint32_t flags, uint64_t *info) try {
  int rc = norm_check_host(text, sent_off, n_sent);
  if (rc) return rc;
  if (!info) return fail(SWT_ERR_INVALID, "null argument: info");
  const uint64_t n_bytes = sent_off[n_sent];
  BatchStage s;
  const uint8_t *d_text = s.in(text, n_bytes);
  const uint64_t *d_off = s.in(sent_off, (size_t)(n_sent + 1) * 8);
  uint64_t *d_info = s.out(info, 24);
  if (s.rc) return s.rc;
  if ((rc = swt_normalize_plan_dev(d_text, n_bytes, d_off, n_sent, flags, d_info, nullptr))) return rc;
  rc = s.fetch();
  g_norm_ws.text = nullptr;  // the staged text goes with this call: no rows call may lean on its plan
  return rc;
} SWT_API_CATCH

int swt_normalize_rows(const uint8_t *text, const uint64_t *sent_off, uint64_t n_sent, uint32_t flags, uint8_t *out_text, uint64_t text_cap,
                       uint64_t *out_off, uint64_t *out_cp_off, uint64_t *src_cp_off, uint32_t *out_align, uint64_t align_cap) try {
  int rc = norm_check_host(text, sent_off, n_sent);
  if (rc) return rc;
  const bool align = flags & SWT_NORMALIZE_ALIGN;
  if (!out_off) return fail(SWT_ERR_INVALID, "null argument: out_off");
  if (align && (!out_cp_off || !src_cp_off)) return fail(SWT_ERR_INVALID, "null argument: an output of SWT_NORMALIZE_ALIGN");
  const uint64_t n_bytes = sent_off[n_sent];
  BatchStage s;
  const uint8_t *d_text = s.in(text, n_bytes);
  const uint64_t *d_off = s.in(sent_off, (size_t)(n_sent + 1) * 8);
  uint64_t info[3] = {0, 0, 0};
  uint64_t *d_info = static_cast<uint64_t *>(s.room(24));
  if (s.rc) return s.rc;
  if ((rc = swt_normalize_plan_dev(d_text, n_bytes, d_off, n_sent, flags & ~SWT_NORMALIZE_ALIGN, d_info, nullptr))) return rc;
  SWT_HIP(hipMemcpy(info, d_info, 24, hipMemcpyDeviceToHost));
  if (info[0] > text_cap || (align && info[1] > align_cap)) {
    g_norm_ws.text = nullptr;
    return fail(SWT_ERR_CAPACITY, "the text normalises to %llu bytes and %llu code points: more than the outputs hold", (unsigned long long)info[0],
                (unsigned long long)info[1]);
  }
  if (info[0] && !out_text) return fail(SWT_ERR_INVALID, "null argument: out_text");
  if (align && info[1] && !out_align) return fail(SWT_ERR_INVALID, "null argument: out_align");
  uint8_t *d_out = s.out(out_text, info[0]);
  uint64_t *d_out_off = s.out(out_off, (size_t)(n_sent + 1) * 8);
  uint64_t *d_cp_off = align ? s.out(out_cp_off, (size_t)(n_sent + 1) * 8) : nullptr;
  uint64_t *d_src_off = align ? s.out(src_cp_off, (size_t)(n_sent + 1) * 8) : nullptr;
  uint32_t *d_align = align ? s.out(out_align, (size_t)info[1] * 4) : nullptr;
  if (s.rc) return s.rc;
  rc = swt_normalize_rows_dev(d_text, n_bytes, d_off, n_sent, flags, d_out, info[0], d_out_off, d_cp_off, d_src_off, d_align, info[1], nullptr);
  g_norm_ws.text = nullptr;
  if (rc) return rc;
  return s.fetch();
} SWT_API_CATCH

int swt_normalize_spans(uint32_t *spans, const uint64_t *tok_off, uint64_t n_sent, const uint32_t *align, const uint64_t *cp_off,
                        const uint64_t *src_cp_off) try {
  if (!tok_off || !cp_off || !src_cp_off) return fail(SWT_ERR_INVALID, "null argument: an offset array");
  for (uint64_t s = 0; s < n_sent; s++)
    if (tok_off[s] > tok_off[s + 1] || cp_off[s] > cp_off[s + 1] || src_cp_off[s] > src_cp_off[s + 1])
      return fail(SWT_ERR_INVALID, "offsets must be non-decreasing");
  const uint64_t n_tok = tok_off[n_sent] - tok_off[0], n_cps = cp_off[n_sent];
  if (tok_off[0]) return fail(SWT_ERR_INVALID, "tok_off[0] must be 0");
  if (!n_tok || !n_sent) return SWT_OK;
  if (!spans || (n_cps && !align)) return fail(SWT_ERR_INVALID, "null argument: spans or align");
  BatchStage s;
  uint32_t *d_spans = s.out(spans, (size_t)n_tok * 8);
  const uint64_t *d_tok_off = s.in(tok_off, (size_t)(n_sent + 1) * 8);
  const uint32_t *d_align = s.in(align, (size_t)n_cps * 4, true);
  const uint64_t *d_cp_off = s.in(cp_off, (size_t)(n_sent + 1) * 8), *d_src_off = s.in(src_cp_off, (size_t)(n_sent + 1) * 8);
  if (s.rc) return s.rc;
  if ((s.rc = s.copy(d_spans, spans, (size_t)n_tok * 8, hipMemcpyHostToDevice))) return s.rc;
  int rc = swt_normalize_spans_dev(d_spans, n_tok, d_tok_off, n_sent, d_align, d_cp_off, d_src_off, nullptr);
  if (rc) return rc;
  return s.fetch();
} SWT_API_CATCH

}  // extern "C"
