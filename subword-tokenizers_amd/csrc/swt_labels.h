// swt_labels.h -- what the calls over the finished rows of a batch share (swt_labels.hip: the fine-tuning labels; swt_tags.hip:
// token-classification inference): the rows of a call and which of their columns are token columns, the loads of a lane's four
// columns, the launch shape, and what the forms refuse from the arguments alone.
#pragma once

#include "swt_batch.h"

namespace swt {

constexpr int kLbThreads = 256;
constexpr int kLbWaves = kLbThreads / 64;
constexpr uint32_t kLbNone = 0xFFFFFFFFu;

// The rows of a call and which of their columns are token columns.
struct LbRows {
  const uint32_t *word;    // null where seq decides and the call needs no word
  const int8_t *seq;       // null: a token column has word != kLbNone
  const uint32_t *sample;  // null: row r is text r
  uint32_t side;
  uint64_t rows, n_samples;
  uint32_t width;
  int vec_word, vec_seq;  // the wide loads: the width is a multiple of four and the pointer is aligned
  uint32_t group;         // lanes per row: a power of two, 1 .. 64
  uint32_t sets;          // sets of rows a wavefront walks
};

// The lane's quad at column c0 of the row at `at`: -> bit j set where column c0 + j is a token column; w: the words (kLbNone
// where the column does not exist, or where nobody needs them: kWord says the kernel does).  A column past the width, and a
// row past the last, is no token column.
template <bool kWord>
__device__ inline uint32_t lb_load_cols(const LbRows &R, uint64_t at, uint64_t c0, bool live, uint32_t (&w)[kBtQuad]) {
  const bool whole = live && c0 + kBtQuad <= R.width;
#pragma unroll
  for (uint32_t j = 0; j < kBtQuad; j++) w[j] = kLbNone;
  if (kWord || !R.seq) {
    if (R.vec_word) {
      if (whole) {
        const uint4 q = *reinterpret_cast<const uint4 *>(R.word + at + c0);
        w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
      }
    } else {
#pragma unroll
      for (uint32_t j = 0; j < kBtQuad; j++)
        if (live && c0 + j < R.width) w[j] = R.word[at + c0 + j];
    }
  }
  uint32_t tok = 0;
  if (R.seq) {
    uint32_t sq = 0xFFFFFFFFu;  // -1 four times: no side
    if (R.vec_seq) {
      if (whole) sq = *reinterpret_cast<const uint32_t *>(R.seq + at + c0);
    } else {
#pragma unroll
      for (uint32_t j = 0; j < kBtQuad; j++)
        if (live && c0 + j < R.width) sq = (sq & ~(0xFFu << (8 * j))) | ((uint32_t)(uint8_t)R.seq[at + c0 + j] << (8 * j));
    }
#pragma unroll
    for (uint32_t j = 0; j < kBtQuad; j++)
      if (((sq >> (8 * j)) & 0xFFu) == R.side) tok |= 1u << j;
  } else {
#pragma unroll
    for (uint32_t j = 0; j < kBtQuad; j++)
      if (w[j] != kLbNone) tok |= 1u << j;
  }
  return tok;
}

__device__ inline bool lb_is_token(const LbRows &R, uint64_t cell) {
  return R.seq ? (uint32_t)(uint8_t)R.seq[cell] == R.side : R.word[cell] != kLbNone;
}

// ---- what the forms refuse, from the arguments alone

struct LbArg {
  const char *name;
  const void *p;
  size_t bytes, align;
  bool required, output;
};

static int lb_check_null(std::initializer_list<LbArg> args) {
  for (const LbArg &a : args)
    if (a.required && !a.p) return fail(SWT_ERR_INVALID, "null argument: %s", a.name);
  return SWT_OK;
}

// every array aligned to its element type, no output sharing a byte with another array
static int lb_check_layout(std::initializer_list<LbArg> args) {
  for (const LbArg &a : args)
    if (reinterpret_cast<uintptr_t>(a.p) & (a.align - 1)) return fail(SWT_ERR_INVALID, "%s is not aligned to its element type", a.name);
  for (const LbArg &o : args) {
    if (!o.output || !o.p || !o.bytes) continue;
    const uintptr_t x = reinterpret_cast<uintptr_t>(o.p);
    for (const LbArg &i : args) {
      const uintptr_t y = reinterpret_cast<uintptr_t>(i.p);
      if (&i == &o || !i.p || !i.bytes) continue;
      if (x < y + i.bytes && y < x + o.bytes) return fail(SWT_ERR_INVALID, "%s overlaps %s: outputs share no byte with another array", o.name, i.name);
    }
  }
  return SWT_OK;
}

static int lb_check_rows(uint64_t rows, uint32_t width, uint64_t n_samples, const void *seq, int32_t side) {
  if (int rc = bt_check_shape(rows, width)) return rc;
  if (n_samples > 0xFFFFFFFFull) return fail(SWT_ERR_INVALID, "n_samples: 2^32 texts or more");
  if (seq && side != 0 && side != 1) return fail(SWT_ERR_INVALID, "side is 0 or 1");
  return SWT_OK;
}

// The lanes of a row, the sets of a wavefront, the wide loads of the token columns; -> the workgroups of the launch.
static unsigned lb_shape(LbRows &R) {
  R.vec_word = R.width % kBtQuad == 0 && bt_aligned(16, {R.word});
  R.vec_seq = R.width % kBtQuad == 0 && bt_aligned(4, {R.seq});
  R.group = bt_group(R.width);
  const RowShape shape = bt_shape(R.rows, R.group, kLbWaves);
  R.sets = (uint32_t)shape.sets;
  return shape.grid;
}

static size_t lb_round(size_t bytes) { return (bytes + 15) & ~(size_t)15; }

}  // namespace swt
