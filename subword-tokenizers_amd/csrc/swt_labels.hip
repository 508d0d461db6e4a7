// swt_labels.hip -- fine-tuning labels on the device, over the finished rows of the batch calls (word_ids, offset_mapping,
// sequence_ids, overflow_to_sample_mapping, length): word labels onto token rows (token classification), answer character spans
// to start and end columns (extractive QA, training), the best span per row and per text from start and end logits (extractive
// QA, evaluation).  Semantics: include/swt.h; tests/label_cases.py holds them in NumPy; the design: DESIGN.md 4.14.
//
// The answer positions are the recipe of the usual QA preprocessing with its two scans confined to the context's columns.  The
// recipe's own first loop runs on into [SEP] and the padding, whose offsets are (0, 0), when the answer starts in the window's
// last token; that quirk is NOT reproduced here: a column that is no token column of the side is never a position.
//
// Three row kernels of the family of mlm_kernel and decode_kernel: ROW-major, a group of g lanes per row (swt_rows.h), so that
// narrow rows share a wavefront; a row wider than 4 g columns takes several steps; a lane takes four columns a step, with wide
// loads and stores when the width is a multiple of four and the pointer is aligned, column by column otherwise.
//   label_words_kernel<T>  a column is the FIRST of its word by its left neighbour's word and token-ness: the quad's first column
//                          asks the lane to its left, the group's first lane the carry of the step before (as mlm_kernel takes
//                          the left class)
//   answer_pos_kernel      per row a max and three more folds over the lanes of the group, the lane's own values carried over the
//                          steps: the first and last token column with their tests, the last start <= a, the first end >= e
//   answer_best_kernel     a lane owns four end columns j and walks the start columns of the band behind them, at most
//                          max_len + 3 of them; the start logits and their token-ness are read through L1 (the window is
//                          contiguous, and neighbouring lanes walk overlapping windows): staging them in LDS would need the
//                          wavefront's barrier in a loop whose trip count differs by lane, or a window as wide as max_len, which
//                          has no bound below the width.  The lane's best is carried over the steps and folded over the group
//                          under the TOTAL order (higher score, smaller i, smaller j), so the shape of the fold does not matter
//   answer_text_kernel     one lane per row; the lane of a text's first row walks forward while `sample` stays the same: no
//                          atomics, no initialisation.  answer_defaults_kernel writes the "nothing" record of every text first
// The loops over the steps and the sets are uniform over the wavefront (the width and the sets are the launch's), a row beyond
// `rows` is masked, not skipped: every lane meets every shuffle.  The walk of answer_best_kernel differs by lane and holds no
// shuffle.  Counts are stored per workgroup; launch_counts_sum sums them into info.  No atomic anywhere.
#include <climits>
#include <cmath>

#include "swt_labels.h"

namespace swt {

constexpr uint32_t kLwFlags = SWT_LABEL_ALL_TOKENS | SWT_LABEL_IDS64;
constexpr uint32_t kApFlags = SWT_ANSWER_CLS | SWT_ANSWER_PAD_LEFT | SWT_LABEL_IDS64;
constexpr uint32_t kAbFlags = SWT_ANSWER_CLS | SWT_ANSWER_PAD_LEFT;
constexpr uint32_t kLwCounts = 4, kApCounts = 3;

template <class T> __device__ inline void lb_store_quad(T *p, const T (&v)[kBtQuad]);
template <> __device__ inline void lb_store_quad<int32_t>(int32_t *p, const int32_t (&v)[kBtQuad]) {
  *reinterpret_cast<int4 *>(p) = make_int4(v[0], v[1], v[2], v[3]);
}
template <> __device__ inline void lb_store_quad<int64_t>(int64_t *p, const int64_t (&v)[kBtQuad]) {
  reinterpret_cast<longlong2 *>(p)[0] = make_longlong2(v[0], v[1]);
  reinterpret_cast<longlong2 *>(p)[1] = make_longlong2(v[2], v[3]);
}

// ---- 1. word labels onto token rows

struct LabelArgs {
  LbRows R;
  const unsigned long long *lab_off;
  const int32_t *lab, *inside;
  uint32_t n_inside;
  int32_t ignore;
  uint32_t all_tokens;
  void *out;
  uint8_t *status;
  unsigned long long *part;  // the counts of every workgroup, kLwCounts each; null: nobody asked for info
  int vec_out;
};

template <class T>
__global__ __launch_bounds__(kLbThreads) void label_words_kernel(LabelArgs A) {
  __shared__ unsigned long long counts[kLbWaves][kLwCounts];
  const LbRows &R = A.R;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t g = R.group, sub = lane & (g - 1), per_wave = 64 / g;
  const uint32_t group_last = lane | (g - 1);  // the last lane of this lane's group
  T *out = reinterpret_cast<T *>(A.out);
  uint32_t n[kLwCounts] = {0, 0, 0, 0};  // labelled, left at ignore as non-first, words without a label, rows of no text
  const uint64_t b0 = ((uint64_t)blockIdx.x * kLbWaves + wave) * per_wave * R.sets + lane / g;
  for (uint32_t it = 0; it < R.sets; it++) {
    const uint64_t b = b0 + (uint64_t)it * per_wave;
    const bool live = b < R.rows;
    const uint64_t at = live ? b * R.width : 0;
    uint64_t lo = 0, n_lab = 0;  // the text's labels: lab[lo, lo + n_lab)
    bool known = false;
    if (live) {
      const uint64_t s = R.sample ? R.sample[b] : b;
      known = s < R.n_samples;
      if (known) {
        lo = A.lab_off[s];
        const uint64_t hi = A.lab_off[s + 1];
        n_lab = hi > lo ? hi - lo : 0;
      } else if (!sub) {
        n[3]++;
      }
    }
    uint32_t carry_word = kLbNone, carry_tok = 0;  // the last column of the step before; none: no token column
    uint32_t missing = 0;
    for (uint64_t base = 0; base < R.width; base += (uint64_t)g * kBtQuad) {
      const uint64_t c0 = base + (uint64_t)sub * kBtQuad;
      const bool whole = live && c0 + kBtQuad <= R.width;
      uint32_t w[kBtQuad];
      const uint32_t tok = lb_load_cols<true>(R, at, c0, live, w);
      // the column to the left of the quad: the lane before, and for the group's first lane the step before
      const uint32_t before_word = __shfl_up(w[kBtQuad - 1], 1, 64), before_tok = __shfl_up(tok >> (kBtQuad - 1), 1, 64);
      uint32_t left_word = sub ? before_word : carry_word, left_tok = sub ? before_tok : carry_tok;
      carry_word = __shfl(w[kBtQuad - 1], group_last, 64);
      carry_tok = __shfl(tok >> (kBtQuad - 1), group_last, 64);
      T v[kBtQuad];
#pragma unroll
      for (uint32_t j = 0; j < kBtQuad; j++) {
        v[j] = (T)A.ignore;
        const uint32_t t = (tok >> j) & 1u, k = w[j];
        if (t && known) {
          if (k >= n_lab) {
            n[2]++;
            missing = 1;
          } else {
            const bool first = !left_tok || left_word != k;
            if (first || A.all_tokens) {
              int32_t l = A.lab[lo + k];
              if (!first && A.inside && l >= 0 && (uint32_t)l < A.n_inside) l = A.inside[l];
              v[j] = (T)l;
              n[0]++;
            } else {
              n[1]++;
            }
          }
        }
        left_tok = t;
        left_word = k;
      }
      if (A.vec_out) {
        if (whole) lb_store_quad<T>(out + at + c0, v);
      } else {
#pragma unroll
        for (uint32_t j = 0; j < kBtQuad; j++)
          if (live && c0 + j < R.width) out[at + c0 + j] = v[j];
      }
    }
    if (A.status) {  // uniform over the launch
      for (uint32_t d = 1; d < g; d <<= 1) missing |= __shfl_xor(missing, d, 64);  // stays inside the group: g is a power of two
      if (live && !sub) A.status[b] = (uint8_t)missing;
    }
  }
  if (!A.part) return;  // uniform over the workgroup
  const unsigned long long sum = bt_fold_counts(n, counts);
  if (threadIdx.x < kLwCounts) A.part[(uint64_t)blockIdx.x * kLwCounts + threadIdx.x] = sum;
}

// ---- 2. answer character spans to start and end columns

struct AnswerArgs {
  LbRows R;
  const uint32_t *spans, *ans, *len;
  int32_t ignore;
  uint32_t use_cls, pad_left, ids64;
  void *start, *end;
  uint8_t *has, *hit;
  unsigned long long *part;  // kApCounts each; null: nobody asked for info
  int vec_spans;
};

// The [CLS] column of row b: 0, or with left padding the first column of the row's content.
__device__ inline uint32_t lb_cls_col(const uint32_t *len, uint32_t pad_left, uint64_t b, uint32_t width) {
  if (!pad_left) return 0;
  const uint32_t n = len[b];
  return n && n <= width ? width - n : 0;  // a length that names no column of the row: column 0
}

__device__ inline void lb_store_pos(void *out, uint64_t r, uint32_t ids64, int32_t v) {
  if (ids64) reinterpret_cast<int64_t *>(out)[r] = v;
  else reinterpret_cast<int32_t *>(out)[r] = v;
}

__global__ __launch_bounds__(kLbThreads) void answer_pos_kernel(AnswerArgs A) {
  __shared__ unsigned long long counts[kLbWaves][kApCounts];
  const LbRows &R = A.R;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t g = R.group, sub = lane & (g - 1), per_wave = 64 / g;
  uint32_t n[kApCounts] = {0, 0, 0};  // rows that hold their answer, rows that do not, rows of no text
  const uint64_t b0 = ((uint64_t)blockIdx.x * kLbWaves + wave) * per_wave * R.sets + lane / g;
  for (uint32_t it = 0; it < R.sets; it++) {
    const uint64_t b = b0 + (uint64_t)it * per_wave;
    const bool live = b < R.rows;
    const uint64_t at = live ? b * R.width : 0;
    uint64_t s = 0;
    uint32_t a = kLbNone, e = 0;
    bool known = false;
    if (live) {
      s = R.sample ? R.sample[b] : b;
      known = s < R.n_samples;
      if (known) {
        a = A.ans[2 * s];
        e = A.ans[2 * s + 1];
      }
    }
    // a column is below 2^31: (column << 1 | test) lies below kLbNone.  first: the least token column with "its start <= a",
    // last: the greatest with "its end >= e"; from: one past the last token column whose start <= a, to: the first whose end >= e
    uint32_t first = kLbNone, last = 0, from = 0, to = kLbNone;
    for (uint64_t base = 0; base < R.width; base += (uint64_t)g * kBtQuad) {
      const uint64_t c0 = base + (uint64_t)sub * kBtQuad;
      uint32_t w[kBtQuad], sp[2 * kBtQuad];
      const uint32_t tok = lb_load_cols<false>(R, at, c0, live, w);
      if (!tok) continue;  // no shuffle in the step: a lane may leave it
      if (A.vec_spans) {   // a token column of a width that is a multiple of four: the quad is whole
        const uint4 p = reinterpret_cast<const uint4 *>(A.spans + (at + c0) * 2)[0], q = reinterpret_cast<const uint4 *>(A.spans + (at + c0) * 2)[1];
        sp[0] = p.x; sp[1] = p.y; sp[2] = p.z; sp[3] = p.w; sp[4] = q.x; sp[5] = q.y; sp[6] = q.z; sp[7] = q.w;
      } else {
#pragma unroll
        for (uint32_t j = 0; j < kBtQuad; j++) {
          sp[2 * j] = sp[2 * j + 1] = 0;
          if ((tok >> j) & 1u) {
            sp[2 * j] = A.spans[(at + c0 + j) * 2];
            sp[2 * j + 1] = A.spans[(at + c0 + j) * 2 + 1];
          }
        }
      }
#pragma unroll
      for (uint32_t j = 0; j < kBtQuad; j++) {
        if (!((tok >> j) & 1u)) continue;
        const uint32_t c = (uint32_t)(c0 + j), starts = sp[2 * j] <= a, ends = sp[2 * j + 1] >= e;
        const uint32_t f = (c << 1) | starts, l = (c << 1) | ends;
        if (f < first) first = f;
        if (l > last) last = l;
        if (starts && c + 1 > from) from = c + 1;
        if (ends && c < to) to = c;
      }
    }
    for (uint32_t d = 1; d < g; d <<= 1) {  // stays inside the group: g is a power of two
      const uint32_t f = __shfl_xor(first, d, 64), l = __shfl_xor(last, d, 64), x = __shfl_xor(from, d, 64), y = __shfl_xor(to, d, 64);
      if (f < first) first = f;
      if (l > last) last = l;
      if (x > from) from = x;
      if (y < to) to = y;
    }
    if (live && !sub) {
      const bool holds = known && a != kLbNone && a < e && first != kLbNone && (first & 1u) && (last & 1u);
      const int32_t nothing = A.use_cls ? (int32_t)lb_cls_col(A.len, A.pad_left, b, R.width) : A.ignore;
      lb_store_pos(A.start, b, A.ids64, holds ? (int32_t)(from - 1) : nothing);
      lb_store_pos(A.end, b, A.ids64, holds ? (int32_t)to : nothing);
      if (A.has) A.has[b] = holds;
      if (holds && A.hit) A.hit[s] = 1;  // the same value from every row of the text: a plain store
      n[0] += holds;
      n[1] += !holds && known;
      n[2] += !known;
    }
  }
  if (!A.part) return;  // uniform over the workgroup
  const unsigned long long sum = bt_fold_counts(n, counts);
  if (threadIdx.x < kApCounts) A.part[(uint64_t)blockIdx.x * kApCounts + threadIdx.x] = sum;
}

// ---- 3. the best span per row and per text

struct BestArgs {
  LbRows R;
  const float *start_logit, *end_logit;
  const uint32_t *len;
  uint32_t max_len;  // 1 .. width
  uint32_t use_cls, pad_left;
  float *row_score, *row_null;
  int32_t *row_start, *row_end;
  unsigned long long *part;  // one count each
  int vec_end;
};

struct LbBest {
  float s;
  int32_t i, j;
};

// (s, i, j) comes before b: higher score, then smaller i, then smaller j.  Total on scores that are no NaN.
__device__ inline bool lb_before(float s, int32_t i, int32_t j, const LbBest &b) {
  return s > b.s || (s == b.s && (i < b.i || (i == b.i && j < b.j)));
}

__global__ __launch_bounds__(kLbThreads) void answer_best_kernel(BestArgs A) {
  __shared__ unsigned long long counts[kLbWaves][1];
  const LbRows &R = A.R;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t g = R.group, sub = lane & (g - 1), per_wave = 64 / g;
  uint32_t n[1] = {0};  // rows with a candidate
  const uint64_t b0 = ((uint64_t)blockIdx.x * kLbWaves + wave) * per_wave * R.sets + lane / g;
  for (uint32_t it = 0; it < R.sets; it++) {
    const uint64_t b = b0 + (uint64_t)it * per_wave;
    const bool live = b < R.rows;
    const uint64_t at = live ? b * R.width : 0;
    const bool known = live && (R.sample ? R.sample[b] : b) < R.n_samples;
    LbBest best{-INFINITY, INT_MAX, INT_MAX};
    for (uint64_t base = 0; base < R.width; base += (uint64_t)g * kBtQuad) {
      const uint64_t c0 = base + (uint64_t)sub * kBtQuad;
      uint32_t w[kBtQuad];
      const uint32_t tok = lb_load_cols<false>(R, at, c0, known, w);
      if (!tok) continue;  // no shuffle in the step: a lane may leave it
      float ej[kBtQuad] = {0.f, 0.f, 0.f, 0.f};
      if (A.vec_end) {  // a token column of a width that is a multiple of four: the quad is whole
        const float4 q = *reinterpret_cast<const float4 *>(A.end_logit + at + c0);
        ej[0] = q.x; ej[1] = q.y; ej[2] = q.z; ej[3] = q.w;
      } else {
#pragma unroll
        for (uint32_t j = 0; j < kBtQuad; j++)
          if ((tok >> j) & 1u) ej[j] = A.end_logit[at + c0 + j];
      }
      // the start columns of the band behind the lane's four end columns: [c0 - (max_len - 1), c0 + 3], inside the row
      const uint64_t reach = A.max_len - 1, lo = c0 > reach ? c0 - reach : 0;
      const uint64_t hi = c0 + kBtQuad <= R.width ? c0 + kBtQuad - 1 : R.width - 1;
      for (uint64_t i = lo; i <= hi; i++) {
        if (!lb_is_token(R, at + i)) continue;
        const float si = A.start_logit[at + i];
#pragma unroll
        for (uint32_t j = 0; j < kBtQuad; j++) {
          const uint64_t c = c0 + j;
          if (!((tok >> j) & 1u) || i > c || c - i >= A.max_len) continue;
          const float score = __fadd_rn(si, ej[j]);  // one IEEE add
          if (score == score && lb_before(score, (int32_t)i, (int32_t)c, best)) best = LbBest{score, (int32_t)i, (int32_t)c};
        }
      }
    }
    for (uint32_t d = 1; d < g; d <<= 1) {  // stays inside the group: g is a power of two
      const float s = __shfl_xor(best.s, d, 64);
      const int32_t i = __shfl_xor(best.i, d, 64), j = __shfl_xor(best.j, d, 64);
      if (lb_before(s, i, j, best)) best = LbBest{s, i, j};
    }
    if (live && !sub) {
      const bool any = best.i != INT_MAX;
      A.row_score[b] = best.s;  // -inf without a candidate
      A.row_start[b] = any ? best.i : -1;
      A.row_end[b] = any ? best.j : -1;
      float null_score = INFINITY;
      if (A.use_cls && known) {
        const uint64_t cls = at + lb_cls_col(A.len, A.pad_left, b, R.width);
        null_score = __fadd_rn(A.start_logit[cls], A.end_logit[cls]);
      }
      A.row_null[b] = null_score;
      n[0] += any;
    }
  }
  if (!A.part) return;  // uniform over the workgroup
  const unsigned long long sum = bt_fold_counts(n, counts);
  if (threadIdx.x < 1) A.part[blockIdx.x] = sum;
}

struct TextArgs {
  const uint32_t *sample;
  uint64_t rows, n_samples;
  uint32_t width;
  const uint32_t *spans;
  const float *row_score, *row_null;
  const int32_t *row_start, *row_end;
  float *score, *null_score;
  int32_t *row, *start_col, *end_col;
  uint32_t *char_start, *char_end;
  unsigned long long *part;  // one count each
};

// the record of a text with no row or no candidate
__global__ __launch_bounds__(kLbThreads) void answer_defaults_kernel(TextArgs A) {
  const uint64_t s = (uint64_t)blockIdx.x * kLbThreads + threadIdx.x;
  if (s >= A.n_samples) return;
  A.score[s] = -INFINITY;
  A.null_score[s] = INFINITY;
  A.row[s] = A.start_col[s] = A.end_col[s] = -1;
  A.char_start[s] = A.char_end[s] = 0;
}

// One lane per row; the lane of a text's first row takes the first of the text's rows in the order (higher score, smaller row)
// and the least null score that is no NaN.
__global__ __launch_bounds__(kLbThreads) void answer_text_kernel(TextArgs A) {
  __shared__ unsigned long long counts[kLbWaves][1];
  const uint64_t r = (uint64_t)blockIdx.x * kLbThreads + threadIdx.x;
  uint32_t n[1] = {0};  // texts with a candidate
  if (r < A.rows) {
    const uint64_t s = A.sample ? A.sample[r] : r;
    if (s < A.n_samples && (!r || !A.sample || A.sample[r - 1] != s)) {
      float top = -INFINITY, null_score = INFINITY;
      int64_t at = -1;
      for (uint64_t k = r; k < A.rows && (k == r || (A.sample && A.sample[k] == s)); k++) {
        if (A.row_start[k] >= 0 && (at < 0 || A.row_score[k] > top)) {
          top = A.row_score[k];
          at = (int64_t)k;
        }
        const float z = A.row_null[k];
        if (z < null_score) null_score = z;  // false for a NaN
      }
      A.null_score[s] = null_score;
      if (at >= 0) {
        const int32_t i = A.row_start[at], j = A.row_end[at];
        A.score[s] = top;
        A.row[s] = (int32_t)at;
        A.start_col[s] = i;
        A.end_col[s] = j;
        A.char_start[s] = A.spans[((uint64_t)at * A.width + (uint32_t)i) * 2];
        A.char_end[s] = A.spans[((uint64_t)at * A.width + (uint32_t)j) * 2 + 1];
        n[0] = 1;
      }
    }
  }
  if (!A.part) return;  // uniform over the launch
  const unsigned long long sum = bt_fold_counts(n, counts);
  if (threadIdx.x < 1) A.part[blockIdx.x] = sum;
}

// the workgroups' counts between the launches of a call and, for the best spans, the rows' results nobody asked for: grow-only
// and shared by all calls of the process (the calls carry no handle), as the scan workspace of the plans and under the same rule
static DevBuf g_label_ws;

struct LabelCall {
  const uint32_t *word;
  const int8_t *seq;
  int32_t side;
  const uint32_t *sample;
  uint64_t rows;
  uint32_t width;
  const uint64_t *lab_off;
  const int32_t *lab;
  uint64_t n_lab, n_samples;
  const int32_t *inside;
  uint32_t n_inside;
  uint32_t flags;
  void *out;
  uint8_t *status;
  uint64_t *info;
};

static int label_check(const LabelCall &c) {
  const std::initializer_list<LbArg> nulls = {{"word", c.word, 0, 4, true, false}, {"lab_off", c.lab_off, 0, 8, true, false},
                                              {"out_labels", c.out, 0, 4, true, true}};
  if (int rc = lb_check_null(nulls)) return rc;
  if (!c.lab && c.n_lab) return fail(SWT_ERR_INVALID, "null argument: lab");
  if (!c.inside && c.n_inside) return fail(SWT_ERR_INVALID, "null argument: inside");
  if (int rc = lb_check_rows(c.rows, c.width, c.n_samples, c.seq, c.side)) return rc;
  if (c.flags & ~kLwFlags) return fail(SWT_ERR_INVALID, "flags: unknown flag");
  const size_t cells = (size_t)c.rows * c.width, t = (c.flags & SWT_LABEL_IDS64) ? 8 : 4;
  return lb_check_layout({{"word", c.word, cells * 4, 4, true, false}, {"seq", c.seq, cells, 1, false, false},
                          {"sample", c.sample, (size_t)c.rows * 4, 4, false, false},
                          {"lab_off", c.lab_off, ((size_t)c.n_samples + 1) * 8, 8, true, false}, {"lab", c.lab, (size_t)c.n_lab * 4, 4, false, false},
                          {"inside", c.inside, (size_t)c.n_inside * 4, 4, false, false}, {"out_labels", c.out, cells * t, t, true, true},
                          {"out_status", c.status, (size_t)c.rows, 1, false, true}, {"info", c.info, kLwCounts * 8, 8, false, true}});
}

struct AnswerCall {
  const uint32_t *spans, *word;
  const int8_t *seq;
  int32_t side;
  const uint32_t *sample;
  uint64_t rows;
  uint32_t width;
  const uint32_t *ans;
  uint64_t n_samples;
  const uint32_t *len;
  uint32_t flags;
  void *start, *end;
  uint8_t *has, *hit;
  uint64_t *info;
};

static int answer_check(const AnswerCall &c) {
  if (int rc = lb_check_null({{"spans", c.spans, 0, 4, true, false}, {"out_start", c.start, 0, 4, true, true}, {"out_end", c.end, 0, 4, true, true}}))
    return rc;
  if (!c.word && !c.seq) return fail(SWT_ERR_INVALID, "null argument: word, with no seq to name the token columns");
  if (!c.ans && c.n_samples) return fail(SWT_ERR_INVALID, "null argument: ans");
  if (int rc = lb_check_rows(c.rows, c.width, c.n_samples, c.seq, c.side)) return rc;
  if (c.flags & ~kApFlags) return fail(SWT_ERR_INVALID, "flags: unknown flag");
  if ((c.flags & SWT_ANSWER_PAD_LEFT) && !c.len) return fail(SWT_ERR_INVALID, "null argument: len, with SWT_ANSWER_PAD_LEFT");
  const size_t cells = (size_t)c.rows * c.width, t = (c.flags & SWT_LABEL_IDS64) ? 8 : 4;
  return lb_check_layout({{"spans", c.spans, cells * 8, 4, true, false}, {"word", c.word, cells * 4, 4, false, false},
                          {"seq", c.seq, cells, 1, false, false}, {"sample", c.sample, (size_t)c.rows * 4, 4, false, false},
                          {"ans", c.ans, (size_t)c.n_samples * 8, 4, false, false}, {"len", c.len, (size_t)c.rows * 4, 4, false, false},
                          {"out_start", c.start, (size_t)c.rows * t, t, true, true}, {"out_end", c.end, (size_t)c.rows * t, t, true, true},
                          {"out_has", c.has, (size_t)c.rows, 1, false, true}, {"out_hit", c.hit, (size_t)c.n_samples, 1, false, true},
                          {"info", c.info, kApCounts * 8, 8, false, true}});
}

struct BestCall {
  const float *start_logit, *end_logit;
  const uint32_t *spans, *word;
  const int8_t *seq;
  int32_t side;
  const uint32_t *sample;
  uint64_t rows;
  uint32_t width;
  uint64_t n_samples;
  uint32_t max_len;
  const uint32_t *len;
  uint32_t flags;
  float *score, *null_score;
  int32_t *row, *start_col, *end_col;
  uint32_t *char_start, *char_end;
  float *row_score;
  int32_t *row_start, *row_end;
  uint64_t *info;
};

static int best_check(const BestCall &c) {
  if (int rc = lb_check_null({{"start_logit", c.start_logit, 0, 4, true, false}, {"end_logit", c.end_logit, 0, 4, true, false},
                              {"spans", c.spans, 0, 4, true, false}}))
    return rc;
  if (!c.word && !c.seq) return fail(SWT_ERR_INVALID, "null argument: word, with no seq to name the token columns");
  if (c.n_samples)
    if (int rc = lb_check_null({{"out_score", c.score, 0, 4, true, true}, {"out_null_score", c.null_score, 0, 4, true, true},
                                {"out_row", c.row, 0, 4, true, true}, {"out_start_col", c.start_col, 0, 4, true, true},
                                {"out_end_col", c.end_col, 0, 4, true, true}, {"out_char_start", c.char_start, 0, 4, true, true},
                                {"out_char_end", c.char_end, 0, 4, true, true}}))
      return rc;
  if (int rc = lb_check_rows(c.rows, c.width, c.n_samples, c.seq, c.side)) return rc;
  if (c.rows > 0x7FFFFFFFull) return fail(SWT_ERR_INVALID, "rows: 2^31 rows or more");
  if (c.flags & ~kAbFlags) return fail(SWT_ERR_INVALID, "flags: unknown flag");
  if ((c.flags & SWT_ANSWER_PAD_LEFT) && !c.len) return fail(SWT_ERR_INVALID, "null argument: len, with SWT_ANSWER_PAD_LEFT");
  if (!c.max_len) return fail(SWT_ERR_INVALID, "max_len: a span of no column");
  const size_t cells = (size_t)c.rows * c.width, ns = (size_t)c.n_samples * 4, nr = (size_t)c.rows * 4;
  return lb_check_layout({{"start_logit", c.start_logit, cells * 4, 4, true, false}, {"end_logit", c.end_logit, cells * 4, 4, true, false},
                          {"spans", c.spans, cells * 8, 4, true, false}, {"word", c.word, cells * 4, 4, false, false},
                          {"seq", c.seq, cells, 1, false, false}, {"sample", c.sample, nr, 4, false, false}, {"len", c.len, nr, 4, false, false},
                          {"out_score", c.score, ns, 4, false, true}, {"out_null_score", c.null_score, ns, 4, false, true},
                          {"out_row", c.row, ns, 4, false, true}, {"out_start_col", c.start_col, ns, 4, false, true},
                          {"out_end_col", c.end_col, ns, 4, false, true}, {"out_char_start", c.char_start, ns, 4, false, true},
                          {"out_char_end", c.char_end, ns, 4, false, true}, {"out_row_score", c.row_score, nr, 4, false, true},
                          {"out_row_start", c.row_start, nr, 4, false, true}, {"out_row_end", c.row_end, nr, 4, false, true},
                          {"info", c.info, 16, 8, false, true}});
}

}  // namespace swt

using namespace swt;

extern "C" {

int swt_label_capacity(uint32_t *cols_per_step, uint32_t *scan_rows) try {
  if (cols_per_step) *cols_per_step = kBtCols;
  if (scan_rows) *scan_rows = kLbThreads;
  return SWT_OK;
} SWT_API_CATCH

int swt_label_words_dev(const uint32_t *d_word, const int8_t *d_seq, int32_t side, const uint32_t *d_sample, uint64_t rows, uint32_t width,
                        const uint64_t *d_lab_off, const int32_t *d_lab, uint64_t n_lab, uint64_t n_samples, const int32_t *d_inside,
                        uint32_t n_inside, int32_t ignore, uint32_t flags, void *d_out_labels, uint8_t *d_out_status, uint64_t *d_info,
                        void *stream) try {
  int rc = label_check({d_word, d_seq, side, d_sample, rows, width, d_lab_off, d_lab, n_lab, n_samples, d_inside, n_inside, flags, d_out_labels,
                        d_out_status, d_info});
  if (rc) return rc;
  if ((rc = ensure_device())) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (!rows) {
    if (d_info) SWT_HIP(hipMemsetAsync(d_info, 0, kLwCounts * 8, st));
    return SWT_OK;
  }
  LabelArgs A{{d_word, d_seq, d_sample, (uint32_t)side, rows, n_samples, width, 0, 0, 1, 1},
              reinterpret_cast<const unsigned long long *>(d_lab_off), d_lab, d_inside, n_inside, ignore,
              (flags & SWT_LABEL_ALL_TOKENS) ? 1u : 0u, d_out_labels, d_out_status, nullptr, 0};
  const unsigned grid = lb_shape(A.R);
  A.vec_out = width % kBtQuad == 0 && bt_aligned(16, {d_out_labels});
  if (d_info) {
    if ((rc = g_label_ws.reserve((size_t)grid * kLwCounts * 8))) return rc;
    A.part = g_label_ws.as<unsigned long long>();
  }
  if (flags & SWT_LABEL_IDS64) hipLaunchKernelGGL(label_words_kernel<int64_t>, dim3(grid), dim3(kLbThreads), 0, st, A);
  else hipLaunchKernelGGL(label_words_kernel<int32_t>, dim3(grid), dim3(kLbThreads), 0, st, A);
  if (d_info) launch_counts_sum(A.part, grid, kLwCounts, reinterpret_cast<unsigned long long *>(d_info), st);
  SWT_HIP(hipGetLastError());
  return SWT_OK;
} SWT_API_CATCH

int swt_label_words(const uint32_t *word, const int8_t *seq, int32_t side, const uint32_t *sample, uint64_t rows, uint32_t width,
                    const uint64_t *lab_off, const int32_t *lab, uint64_t n_lab, uint64_t n_samples, const int32_t *inside, uint32_t n_inside,
                    int32_t ignore, uint32_t flags, void *out_labels, uint8_t *out_status, uint64_t *info) try {
  int rc = label_check({word, seq, side, sample, rows, width, lab_off, lab, n_lab, n_samples, inside, n_inside, flags, out_labels, out_status, info});
  if (rc) return rc;
  for (uint64_t s = 0; s < n_samples; s++)
    if (lab_off[s] > lab_off[s + 1]) return fail(SWT_ERR_INVALID, "lab_off: offsets must not decrease");
  if (lab_off[n_samples] > n_lab) return fail(SWT_ERR_INVALID, "lab_off runs past the n_lab labels");
  if (info)
    for (uint32_t k = 0; k < kLwCounts; k++) info[k] = 0;
  if (!rows) return SWT_OK;
  if ((rc = ensure_device())) return rc;
  const size_t cells = (size_t)rows * width;
  BatchStage s;
  const uint32_t *d_word = s.in(word, cells * 4), *d_sample = s.in(sample, (size_t)rows * 4);
  const int8_t *d_seq = s.in(seq, cells);
  const uint64_t *d_off = s.in(lab_off, ((size_t)n_samples + 1) * 8);
  const int32_t *d_lab = s.in(lab, (size_t)n_lab * 4), *d_inside = s.in(inside, (size_t)n_inside * 4);
  void *d_out = s.out(static_cast<uint8_t *>(out_labels), cells * ((flags & SWT_LABEL_IDS64) ? 8 : 4));
  uint8_t *d_status = s.out(out_status, (size_t)rows);
  uint64_t *d_info = s.out(info, kLwCounts * 8);
  if (s.rc) return s.rc;
  if ((rc = swt_label_words_dev(d_word, d_seq, side, d_sample, rows, width, d_off, d_lab, n_lab, n_samples, d_inside, n_inside, ignore, flags, d_out,
                                d_status, d_info, nullptr)))
    return rc;
  return s.fetch();
} SWT_API_CATCH

int swt_answer_positions_dev(const uint32_t *d_spans, const uint32_t *d_word, const int8_t *d_seq, int32_t side, const uint32_t *d_sample,
                             uint64_t rows, uint32_t width, const uint32_t *d_ans, uint64_t n_samples, const uint32_t *d_len, int32_t ignore,
                             uint32_t flags, void *d_out_start, void *d_out_end, uint8_t *d_out_has, uint8_t *d_out_hit, uint64_t *d_info,
                             void *stream) try {
  int rc = answer_check({d_spans, d_word, d_seq, side, d_sample, rows, width, d_ans, n_samples, d_len, flags, d_out_start, d_out_end, d_out_has,
                         d_out_hit, d_info});
  if (rc) return rc;
  if ((rc = ensure_device())) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (d_out_hit && n_samples) SWT_HIP(hipMemsetAsync(d_out_hit, 0, n_samples, st));
  if (!rows) {
    if (d_info) SWT_HIP(hipMemsetAsync(d_info, 0, kApCounts * 8, st));
    return SWT_OK;
  }
  AnswerArgs A{{d_word, d_seq, d_sample, (uint32_t)side, rows, n_samples, width, 0, 0, 1, 1}, d_spans, d_ans, d_len, ignore,
               (flags & SWT_ANSWER_CLS) ? 1u : 0u, (flags & SWT_ANSWER_PAD_LEFT) ? 1u : 0u, (flags & SWT_LABEL_IDS64) ? 1u : 0u,
               d_out_start, d_out_end, d_out_has, d_out_hit, nullptr, 0};
  const unsigned grid = lb_shape(A.R);
  A.vec_spans = width % kBtQuad == 0 && bt_aligned(16, {d_spans});
  if (d_info) {
    if ((rc = g_label_ws.reserve((size_t)grid * kApCounts * 8))) return rc;
    A.part = g_label_ws.as<unsigned long long>();
  }
  hipLaunchKernelGGL(answer_pos_kernel, dim3(grid), dim3(kLbThreads), 0, st, A);
  if (d_info) launch_counts_sum(A.part, grid, kApCounts, reinterpret_cast<unsigned long long *>(d_info), st);
  SWT_HIP(hipGetLastError());
  return SWT_OK;
} SWT_API_CATCH

int swt_answer_positions(const uint32_t *spans, const uint32_t *word, const int8_t *seq, int32_t side, const uint32_t *sample, uint64_t rows,
                         uint32_t width, const uint32_t *ans, uint64_t n_samples, const uint32_t *len, int32_t ignore, uint32_t flags,
                         void *out_start, void *out_end, uint8_t *out_has, uint8_t *out_hit, uint64_t *info) try {
  int rc = answer_check({spans, word, seq, side, sample, rows, width, ans, n_samples, len, flags, out_start, out_end, out_has, out_hit, info});
  if (rc) return rc;
  if (info)
    for (uint32_t k = 0; k < kApCounts; k++) info[k] = 0;
  if (out_hit)
    for (uint64_t s = 0; s < n_samples; s++) out_hit[s] = 0;
  if (!rows) return SWT_OK;
  if ((rc = ensure_device())) return rc;
  const size_t cells = (size_t)rows * width, t = (flags & SWT_LABEL_IDS64) ? 8 : 4;
  BatchStage s;
  const uint32_t *d_spans = s.in(spans, cells * 8), *d_word = s.in(word, cells * 4), *d_sample = s.in(sample, (size_t)rows * 4);
  const int8_t *d_seq = s.in(seq, cells);
  const uint32_t *d_ans = s.in(ans, (size_t)n_samples * 8), *d_len = s.in(len, (size_t)rows * 4);
  void *d_start = s.out(static_cast<uint8_t *>(out_start), (size_t)rows * t), *d_end = s.out(static_cast<uint8_t *>(out_end), (size_t)rows * t);
  uint8_t *d_has = s.out(out_has, (size_t)rows), *d_hit = n_samples ? s.out(out_hit, (size_t)n_samples) : nullptr;
  uint64_t *d_info = s.out(info, kApCounts * 8);
  if (s.rc) return s.rc;
  if ((rc = swt_answer_positions_dev(d_spans, d_word, d_seq, side, d_sample, rows, width, d_ans, n_samples, d_len, ignore, flags, d_start, d_end,
                                     d_has, d_hit, d_info, nullptr)))
    return rc;
  return s.fetch();
} SWT_API_CATCH

int swt_answer_best_dev(const float *d_start_logit, const float *d_end_logit, const uint32_t *d_spans, const uint32_t *d_word, const int8_t *d_seq,
                        int32_t side, const uint32_t *d_sample, uint64_t rows, uint32_t width, uint64_t n_samples, uint32_t max_len,
                        const uint32_t *d_len, uint32_t flags, float *d_out_score, float *d_out_null_score, int32_t *d_out_row,
                        int32_t *d_out_start_col, int32_t *d_out_end_col, uint32_t *d_out_char_start, uint32_t *d_out_char_end,
                        float *d_out_row_score, int32_t *d_out_row_start, int32_t *d_out_row_end, uint64_t *d_info, void *stream) try {
  int rc = best_check({d_start_logit, d_end_logit, d_spans, d_word, d_seq, side, d_sample, rows, width, n_samples, max_len, d_len, flags,
                       d_out_score, d_out_null_score, d_out_row, d_out_start_col, d_out_end_col, d_out_char_start, d_out_char_end,
                       d_out_row_score, d_out_row_start, d_out_row_end, d_info});
  if (rc) return rc;
  if ((rc = ensure_device())) return rc;
  hipStream_t st = (hipStream_t)stream;
  TextArgs T{d_sample, rows, n_samples, width, d_spans, d_out_row_score, nullptr, d_out_row_start, d_out_row_end, d_out_score,
             d_out_null_score, d_out_row, d_out_start_col, d_out_end_col, d_out_char_start, d_out_char_end, nullptr};
  if (n_samples)
    hipLaunchKernelGGL(answer_defaults_kernel, dim3((unsigned)((n_samples + kLbThreads - 1) / kLbThreads)), dim3(kLbThreads), 0, st, T);
  if (!rows) {
    if (d_info) SWT_HIP(hipMemsetAsync(d_info, 0, 16, st));
    SWT_HIP(hipGetLastError());
    return SWT_OK;
  }
  BestArgs A{{d_word, d_seq, d_sample, (uint32_t)side, rows, n_samples, width, 0, 0, 1, 1}, d_start_logit, d_end_logit, d_len,
             max_len < width ? max_len : width, (flags & SWT_ANSWER_CLS) ? 1u : 0u, (flags & SWT_ANSWER_PAD_LEFT) ? 1u : 0u,
             d_out_row_score, nullptr, d_out_row_start, d_out_row_end, nullptr, 0};
  const unsigned grid = lb_shape(A.R), text_grid = (unsigned)((rows + kLbThreads - 1) / kLbThreads);
  A.vec_end = width % kBtQuad == 0 && bt_aligned(16, {d_end_logit});
  // the workspace: the two launches' counts, the rows' null scores, and the rows' results where the caller takes none
  const size_t part_bytes = lb_round(((size_t)grid + text_grid) * 8), row_bytes = lb_round((size_t)rows * 4);
  if ((rc = g_label_ws.reserve(part_bytes + 4 * row_bytes))) return rc;
  uint8_t *ws = g_label_ws.as<uint8_t>();
  if (d_info) {
    A.part = reinterpret_cast<unsigned long long *>(ws);
    T.part = A.part + grid;
  }
  A.row_null = reinterpret_cast<float *>(ws + part_bytes);
  if (!A.row_score) A.row_score = reinterpret_cast<float *>(ws + part_bytes + row_bytes);
  if (!A.row_start) A.row_start = reinterpret_cast<int32_t *>(ws + part_bytes + 2 * row_bytes);
  if (!A.row_end) A.row_end = reinterpret_cast<int32_t *>(ws + part_bytes + 3 * row_bytes);
  T.row_score = A.row_score; T.row_null = A.row_null; T.row_start = A.row_start; T.row_end = A.row_end;
  hipLaunchKernelGGL(answer_best_kernel, dim3(grid), dim3(kLbThreads), 0, st, A);
  if (n_samples) hipLaunchKernelGGL(answer_text_kernel, dim3(text_grid), dim3(kLbThreads), 0, st, T);
  if (d_info) {
    launch_counts_sum(A.part, grid, 1, reinterpret_cast<unsigned long long *>(d_info), st);
    if (n_samples) launch_counts_sum(T.part, text_grid, 1, reinterpret_cast<unsigned long long *>(d_info) + 1, st);
    else SWT_HIP(hipMemsetAsync(d_info + 1, 0, 8, st));
  }
  SWT_HIP(hipGetLastError());
  return SWT_OK;
} SWT_API_CATCH

int swt_answer_best(const float *start_logit, const float *end_logit, const uint32_t *spans, const uint32_t *word, const int8_t *seq, int32_t side,
                    const uint32_t *sample, uint64_t rows, uint32_t width, uint64_t n_samples, uint32_t max_len, const uint32_t *len,
                    uint32_t flags, float *out_score, float *out_null_score, int32_t *out_row, int32_t *out_start_col, int32_t *out_end_col,
                    uint32_t *out_char_start, uint32_t *out_char_end, float *out_row_score, int32_t *out_row_start, int32_t *out_row_end,
                    uint64_t *info) try {
  int rc = best_check({start_logit, end_logit, spans, word, seq, side, sample, rows, width, n_samples, max_len, len, flags, out_score,
                       out_null_score, out_row, out_start_col, out_end_col, out_char_start, out_char_end, out_row_score, out_row_start,
                       out_row_end, info});
  if (rc) return rc;
  if (sample)
    for (uint64_t r = 1; r < rows; r++)
      if (sample[r] < sample[r - 1]) return fail(SWT_ERR_INVALID, "sample: a text's rows are contiguous, the texts in order");
  if (info) info[0] = info[1] = 0;
  if (!rows) {  // every text's "nothing" record, without a device
    for (uint64_t s = 0; s < n_samples; s++) {
      out_score[s] = -INFINITY;
      out_null_score[s] = INFINITY;
      out_row[s] = out_start_col[s] = out_end_col[s] = -1;
      out_char_start[s] = out_char_end[s] = 0;
    }
    return SWT_OK;
  }
  if ((rc = ensure_device())) return rc;
  const size_t cells = (size_t)rows * width, ns = (size_t)n_samples * 4, nr = (size_t)rows * 4;
  BatchStage s;
  const float *d_sl = s.in(start_logit, cells * 4), *d_el = s.in(end_logit, cells * 4);
  const uint32_t *d_spans = s.in(spans, cells * 8), *d_word = s.in(word, cells * 4), *d_sample = s.in(sample, nr), *d_len = s.in(len, nr);
  const int8_t *d_seq = s.in(seq, cells);
  float *d_score = s.out(out_score, ns), *d_null = s.out(out_null_score, ns), *d_row_score = s.out(out_row_score, nr);
  int32_t *d_row = s.out(out_row, ns), *d_i = s.out(out_start_col, ns), *d_j = s.out(out_end_col, ns);
  uint32_t *d_cs = s.out(out_char_start, ns), *d_ce = s.out(out_char_end, ns);
  int32_t *d_row_start = s.out(out_row_start, nr), *d_row_end = s.out(out_row_end, nr);
  uint64_t *d_info = s.out(info, 16);
  if (s.rc) return s.rc;
  if ((rc = swt_answer_best_dev(d_sl, d_el, d_spans, d_word, d_seq, side, d_sample, rows, width, n_samples, max_len, d_len, flags, d_score, d_null,
                                d_row, d_i, d_j, d_cs, d_ce, d_row_score, d_row_start, d_row_end, d_info, nullptr)))
    return rc;
  return s.fetch();
} SWT_API_CATCH

}  // extern "C"
