// swt_tags.hip -- token-classification inference on the device, over the finished rows of the batch calls and a model's logits
// [rows, width, L]: how many words each text has (the plan), one label and softmax score per word from the run that speaks for
// it, and the BIO grouping of the words into entities.  Semantics: include/swt.h; tests/tag_cases.py holds them in NumPy; the
// design: DESIGN.md 4.15.
//
// A RUN is a maximal set of consecutive token columns of a row with the same word id: the first-column rule of
// label_words_kernel continued to the right.  The row kernels are of the family of swt_labels.hip (a group of g lanes per row,
// four columns a lane and step, rows beyond `rows` masked so that every lane meets every shuffle):
//   tag_row_words_kernel   per row 1 + the greatest word id of its token columns, folded over the group; tag_text_words_kernel
//                          then has the lane of a text's first row walk the text's rows (as answer_text_kernel does), and
//                          launch_scan_bases turns the texts' counts into word_off in place
//   tag_runs_kernel<false> finds the runs: first columns as label_words_kernel finds them, the token columns to the left from a
//                          scan of the quads' counts over the group and a carry over the steps, the row's total from that scan
//                          (a row of one step) or a pass of its own before; the lane of a first column walks to the run's end
//                          through L1.  Every run that takes part puts its KEY -- context, then the smaller row, then the smaller
//                          column, packed into 64 bits with field widths taken from the launch -- into the word's slot of a
//                          zeroed workspace with a vector atomicMax: no value comes back, the slots are spread over the words,
//                          and the order is total, so the launch shape cannot show in the result
//   tag_runs_kernel<true>  finds the runs again; the run whose key is the slot's owns the word and alone stores its record.  It
//                          walks the L logits of its columns twice through L1 -- once for the word's vector, the label and the
//                          maximum, once for the sum of expf -- so that no vector of L floats lives in registers or scratch
//   tag_missing_kernel     a lane per word: the "nothing" record where the slot is still zero
//   ent_head_kernel, launch_scan_bases, ent_scatter_kernel: head flags (a word's text by bisection of word_off), their exclusive
//                          sums, and the heads' lanes walking their entities; lanes at or beyond the count write "nothing"
// Counts are stored per workgroup and summed by launch_counts_sum; the only atomic is the key's.
#include <cmath>

#include "swt_labels.h"

namespace swt {

constexpr uint32_t kTgStrategies = 3;

struct PlanArgs {
  LbRows R;
  unsigned long long *row_words;  // per row: 1 + its greatest word id, 0 without a token column or a text
  unsigned long long *word_off;
  unsigned long long *part;  // one count each: rows of no text
};

__global__ __launch_bounds__(kLbThreads) void tag_row_words_kernel(PlanArgs A) {
  __shared__ unsigned long long counts[kLbWaves][1];
  const LbRows &R = A.R;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t g = R.group, sub = lane & (g - 1), per_wave = 64 / g;
  uint32_t n[1] = {0};
  const uint64_t b0 = ((uint64_t)blockIdx.x * kLbWaves + wave) * per_wave * R.sets + lane / g;
  for (uint32_t it = 0; it < R.sets; it++) {
    const uint64_t b = b0 + (uint64_t)it * per_wave;
    const bool live = b < R.rows;
    const uint64_t at = live ? b * R.width : 0;
    const bool known = live && (R.sample ? R.sample[b] : b) < R.n_samples;
    unsigned long long m = 0;
    for (uint64_t base = 0; base < R.width; base += (uint64_t)g * kBtQuad) {
      const uint64_t c0 = base + (uint64_t)sub * kBtQuad;
      uint32_t w[kBtQuad];
      const uint32_t tok = lb_load_cols<true>(R, at, c0, known, w);
#pragma unroll
      for (uint32_t j = 0; j < kBtQuad; j++)
        if (((tok >> j) & 1u) && (unsigned long long)w[j] + 1 > m) m = (unsigned long long)w[j] + 1;
    }
    for (uint32_t d = 1; d < g; d <<= 1) {  // stays inside the group: g is a power of two
      const unsigned long long o = __shfl_xor(m, d, 64);
      if (o > m) m = o;
    }
    if (live && !sub) {
      A.row_words[b] = m;
      n[0] += !known;
    }
  }
  const unsigned long long sum = bt_fold_counts(n, counts);
  if (threadIdx.x < 1) A.part[blockIdx.x] = sum;
}

// One lane per row; the lane of a text's first row takes the greatest count of the text's rows.  word_off is zeroed before.
__global__ __launch_bounds__(kLbThreads) void tag_text_words_kernel(PlanArgs A) {
  const LbRows &R = A.R;
  const uint64_t r = (uint64_t)blockIdx.x * kLbThreads + threadIdx.x;
  if (r >= R.rows) return;
  const uint64_t s = R.sample ? R.sample[r] : r;
  if (s >= R.n_samples || (r && R.sample && R.sample[r - 1] == s)) return;
  unsigned long long m = 0;
  for (uint64_t k = r; k < R.rows && (k == r || (R.sample && R.sample[k] == s)); k++)
    if (A.row_words[k] > m) m = A.row_words[k];
  A.word_off[s] = m;
}

// ---- one label and score per word

struct TagArgs {
  LbRows R;
  const float *logits;
  uint32_t L, strategy;
  const uint32_t *spans;
  const unsigned long long *word_off;
  uint64_t n_words;
  unsigned long long *key;     // per word: the greatest key of its runs, 0 without one
  uint32_t row_bits, col_bits;  // the key's fields: context | row | column
  int32_t *label;
  float *score;
  int32_t *row, *col, *ncols;
  uint32_t *char_start, *char_end;
  float *word_logits;
  unsigned long long *part0, *part1;  // one count each per workgroup; null: nobody asked for info
};

// Greater context first, then the smaller row, then the smaller column; never 0: 2^col_bits > width.
__device__ inline unsigned long long tag_key(const TagArgs &A, uint32_t context, uint64_t row, uint32_t col) {
  const unsigned long long rmask = (1ull << A.row_bits) - 1, cmask = (1ull << A.col_bits) - 1;
  return ((unsigned long long)context << (A.row_bits + A.col_bits)) | ((rmask - row) << A.col_bits) | (cmask - col);
}

__device__ inline uint64_t tag_key_row(const TagArgs &A, unsigned long long key) {
  const unsigned long long rmask = (1ull << A.row_bits) - 1;
  return rmask - ((key >> A.col_bits) & rmask);
}

// Entry l of the word's vector; x: the logits of the run's first column, the next column L floats on.
__device__ inline float tag_value(const float *x, uint32_t L, uint32_t strategy, uint32_t ncols, uint32_t l) {
  float v = x[l];
  if (strategy == SWT_TAG_FIRST || ncols == 1) return v;
  if (strategy == SWT_TAG_MEAN) {
    for (uint32_t i = 1; i < ncols; i++) v = __fadd_rn(v, x[(uint64_t)i * L + l]);  // in column order: part of the contract
    return __fdiv_rn(v, (float)ncols);
  }
  for (uint32_t i = 1; i < ncols; i++) {
    const float y = x[(uint64_t)i * L + l];
    if (y == y && (!(v == v) || y > v)) v = y;
  }
  return v;
}

// The record of word `at` from the run of ncols columns at column c of row b: the owner's lane alone.
__device__ inline void tag_store(const TagArgs &A, uint64_t at, uint64_t b, uint32_t c, uint32_t ncols) {
  const uint64_t cell = b * A.R.width + c;
  const float *x = A.logits + cell * A.L;
  int32_t best = -1;
  float m = NAN;
  for (uint32_t l = 0; l < A.L; l++) {
    const float v = tag_value(x, A.L, A.strategy, ncols, l);
    if (A.word_logits) A.word_logits[at * A.L + l] = v;
    if (v == v && (best < 0 || v > m)) {
      best = (int32_t)l;
      m = v;
    }
  }
  if (A.label) A.label[at] = best;
  if (A.score) {
    float sum = 0.f;
    for (uint32_t l = 0; l < A.L; l++) sum = __fadd_rn(sum, expf(__fsub_rn(tag_value(x, A.L, A.strategy, ncols, l), m)));
    A.score[at] = __fdiv_rn(1.0f, sum);
  }
  if (A.row) A.row[at] = (int32_t)b;
  if (A.col) A.col[at] = (int32_t)c;
  if (A.ncols) A.ncols[at] = (int32_t)ncols;
  if (A.char_start) A.char_start[at] = A.spans[cell * 2];
  if (A.char_end) A.char_end[at] = A.spans[(cell + ncols - 1) * 2 + 1];
}

// kStore false: every run that takes part puts its key into its word's slot; n: runs that take no part.
// kStore true: the run whose key is the slot's stores the word; n: words stored, runs that lost to another row's run.
template <bool kStore>
__global__ __launch_bounds__(kLbThreads) void tag_runs_kernel(TagArgs A) {
  __shared__ unsigned long long counts[kLbWaves][2];
  const LbRows &R = A.R;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t g = R.group, sub = lane & (g - 1), per_wave = 64 / g;
  const uint32_t group_last = lane | (g - 1);  // the last lane of this lane's group
  const bool one = R.width <= g * kBtQuad;     // a row of one step: the scan of the step has the row's total
  uint32_t n[2] = {0, 0};
  const uint64_t b0 = ((uint64_t)blockIdx.x * kLbWaves + wave) * per_wave * R.sets + lane / g;
  for (uint32_t it = 0; it < R.sets; it++) {
    const uint64_t b = b0 + (uint64_t)it * per_wave;
    const bool live = b < R.rows;
    const uint64_t at = live ? b * R.width : 0;
    uint64_t lo = 0, n_word = 0;  // the text's words: [lo, lo + n_word)
    bool known = false;
    if (live) {
      const uint64_t s = R.sample ? R.sample[b] : b;
      known = s < R.n_samples;
      if (known) {
        lo = A.word_off[s];
        const uint64_t hi = A.word_off[s + 1];
        n_word = hi > lo ? hi - lo : 0;
      }
    }
    uint32_t total = 0;  // the token columns of the row
    if (!one) {
      for (uint64_t base = 0; base < R.width; base += (uint64_t)g * kBtQuad) {
        uint32_t w[kBtQuad];
        total += __popc(lb_load_cols<false>(R, at, base + (uint64_t)sub * kBtQuad, live, w));
      }
      for (uint32_t d = 1; d < g; d <<= 1) total += __shfl_xor(total, d, 64);  // stays inside the group
    }
    uint32_t carry_word = kLbNone, carry_tok = 0, carry_count = 0;  // the last column of the step before, the token columns so far
    for (uint64_t base = 0; base < R.width; base += (uint64_t)g * kBtQuad) {
      const uint64_t c0 = base + (uint64_t)sub * kBtQuad;
      uint32_t w[kBtQuad];
      const uint32_t tok = lb_load_cols<true>(R, at, c0, live, w);
      const uint32_t before_word = __shfl_up(w[kBtQuad - 1], 1, 64), before_tok = __shfl_up(tok >> (kBtQuad - 1), 1, 64);
      uint32_t left_word = sub ? before_word : carry_word, left_tok = sub ? before_tok : carry_tok;
      carry_word = __shfl(w[kBtQuad - 1], group_last, 64);
      carry_tok = __shfl(tok >> (kBtQuad - 1), group_last, 64);
      const uint32_t mine = __popc(tok);
      uint32_t upto = mine;  // the token columns of the step up to and with this lane's
      for (uint32_t d = 1; d < g; d <<= 1) {
        const uint32_t o = __shfl_up(upto, d, 64);
        if (sub >= d) upto += o;
      }
      const uint32_t before = carry_count + upto - mine, step_total = __shfl(upto, group_last, 64);
      carry_count += step_total;
      if (one) total = step_total;
#pragma unroll
      for (uint32_t j = 0; j < kBtQuad; j++) {
        const uint32_t t = (tok >> j) & 1u, k = w[j];
        if (t && (!left_tok || left_word != k)) {  // the first column of a run: no shuffle in here
          const uint64_t c = c0 + j;
          uint64_t e = c + 1;
          while (e < R.width && lb_is_token(R, at + e) && R.word[at + e] == k) e++;
          const uint32_t ncols = (uint32_t)(e - c), left = before + __popc(tok & ((1u << j) - 1u)), right = total - left - ncols;
          if (!known || k >= n_word || lo + k >= A.n_words) {
            if (!kStore) n[0]++;
          } else {
            const unsigned long long key = tag_key(A, left < right ? left : right, b, (uint32_t)c);
            if (!kStore) {
              atomicMax(&A.key[lo + k], key);
            } else {
              const unsigned long long winner = A.key[lo + k];
              if (winner == key) {
                tag_store(A, lo + k, b, (uint32_t)c, ncols);
                n[0]++;
              } else if (tag_key_row(A, winner) != b) {
                n[1]++;
              }
            }
          }
        }
        left_tok = t;
        left_word = k;
      }
    }
  }
  if (!A.part0) return;  // uniform over the workgroup
  const unsigned long long sum = bt_fold_counts(n, counts);
  if (threadIdx.x == 0) A.part0[blockIdx.x] = sum;
  if (threadIdx.x == 1 && kStore) A.part1[blockIdx.x] = sum;
}

// the record of a word with no run
__global__ __launch_bounds__(kLbThreads) void tag_missing_kernel(TagArgs A) {
  __shared__ unsigned long long counts[kLbWaves][1];
  const uint64_t at = (uint64_t)blockIdx.x * kLbThreads + threadIdx.x;
  uint32_t n[1] = {0};
  if (at < A.n_words && !A.key[at]) {
    n[0] = 1;
    if (A.label) A.label[at] = -1;
    if (A.score) A.score[at] = 0.f;
    if (A.row) A.row[at] = -1;
    if (A.col) A.col[at] = -1;
    if (A.ncols) A.ncols[at] = -1;
    if (A.char_start) A.char_start[at] = 0;
    if (A.char_end) A.char_end[at] = 0;
    if (A.word_logits)
      for (uint32_t l = 0; l < A.L; l++) A.word_logits[at * A.L + l] = NAN;
  }
  if (!A.part0) return;  // uniform over the launch
  const unsigned long long sum = bt_fold_counts(n, counts);
  if (threadIdx.x < 1) A.part0[blockIdx.x] = sum;
}

// ---- BIO grouping over the word arrays

struct EntArgs {
  const int32_t *label;
  const float *score;
  const uint32_t *char_start, *char_end;
  const unsigned long long *word_off;
  uint64_t n_samples, n_words;
  const int32_t *etype;
  const uint8_t *begins;
  uint32_t L;
  unsigned long long *head;  // n_words + 1: the head flags, then their exclusive sums and the count
  int32_t *text, *type, *first, *last;
  uint32_t *out_start, *out_end;
  float *out_score;
  unsigned long long *part;  // one count each: words inside entities; null: nobody asked for info
};

__device__ inline int32_t ent_type(const EntArgs &A, uint64_t w) {
  const int32_t l = A.label[w];
  return l >= 0 && (uint32_t)l < A.L ? A.etype[l] : -1;
}

// The text of word w: the last s with word_off[s] <= w; n_samples for a word of no text.
__device__ inline uint64_t ent_text(const EntArgs &A, uint64_t w) {
  if (w >= A.word_off[A.n_samples] || w < A.word_off[0]) return A.n_samples;
  uint64_t lo = 0, hi = A.n_samples;  // word_off[lo] <= w < word_off[hi]
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (A.word_off[mid] <= w) lo = mid;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(kLbThreads) void ent_head_kernel(EntArgs A) {
  __shared__ unsigned long long counts[kLbWaves][1];
  const uint64_t w = (uint64_t)blockIdx.x * kLbThreads + threadIdx.x;
  uint32_t n[1] = {0};
  if (w < A.n_words) {
    const uint64_t s = ent_text(A, w);
    const int32_t t = s < A.n_samples ? ent_type(A, w) : -1;
    bool head = false;
    if (t >= 0) {
      n[0] = 1;
      head = w == A.word_off[s] || ent_type(A, w - 1) != t || A.begins[A.label[w]];
    }
    A.head[w] = head;
  }
  if (!A.part) return;  // uniform over the launch
  const unsigned long long sum = bt_fold_counts(n, counts);
  if (threadIdx.x < 1) A.part[blockIdx.x] = sum;
}

// A lane per word: the lane of a head walks its entity and stores record head[w]; the lanes at or beyond the count store the
// "nothing" record at their own index.  Every record is stored once.
__global__ __launch_bounds__(kLbThreads) void ent_scatter_kernel(EntArgs A) {
  const uint64_t w = (uint64_t)blockIdx.x * kLbThreads + threadIdx.x;
  if (w >= A.n_words) return;
  const unsigned long long at = A.head[w];
  if (w >= A.head[A.n_words]) {
    A.text[w] = A.type[w] = A.first[w] = A.last[w] = -1;
    A.out_start[w] = A.out_end[w] = 0;
    A.out_score[w] = 0.f;
  }
  if (A.head[w + 1] == at) return;  // no head
  const uint64_t s = ent_text(A, w), lo = A.word_off[s], hi = A.word_off[s + 1], end = hi < A.n_words ? hi : A.n_words;
  const int32_t t = ent_type(A, w);
  float sum = A.score[w];
  uint64_t e = w + 1;
  while (e < end && A.head[e + 1] == A.head[e] && ent_type(A, e) == t) sum = __fadd_rn(sum, A.score[e++]);
  A.text[at] = (int32_t)s;
  A.type[at] = t;
  A.first[at] = (int32_t)(w - lo);
  A.last[at] = (int32_t)(e - 1 - lo);
  A.out_start[at] = A.char_start[w];
  A.out_end[at] = A.char_end[e - 1];
  A.out_score[at] = __fdiv_rn(sum, (float)(e - w));
}

// the runs' keys, the rows' counts, the head flags and the workgroups' counts between the launches of a call: grow-only and
// shared by all calls of the process, as the workspace of the label calls and under the same rule
static DevBuf g_tag_ws;

static uint32_t tg_bits(uint64_t v) {  // the bits that hold v
  uint32_t n = 0;
  while (v >> n) n++;
  return n;
}

struct PlanCall {
  const uint32_t *word;
  const int8_t *seq;
  int32_t side;
  const uint32_t *sample;
  uint64_t rows;
  uint32_t width;
  uint64_t n_samples;
  uint64_t *word_off, *info;
};

static int plan_check(const PlanCall &c) {
  if (int rc = lb_check_null({{"word", c.word, 0, 4, true, false}, {"out_word_off", c.word_off, 0, 8, true, true}, {"info", c.info, 0, 8, true, true}}))
    return rc;
  if (int rc = lb_check_rows(c.rows, c.width, c.n_samples, c.seq, c.side)) return rc;
  const size_t cells = (size_t)c.rows * c.width;
  return lb_check_layout({{"word", c.word, cells * 4, 4, true, false}, {"seq", c.seq, cells, 1, false, false},
                          {"sample", c.sample, (size_t)c.rows * 4, 4, false, false},
                          {"out_word_off", c.word_off, ((size_t)c.n_samples + 1) * 8, 8, true, true}, {"info", c.info, 16, 8, true, true}});
}

struct PredictCall {
  const float *logits;
  const uint32_t *word;
  const int8_t *seq;
  int32_t side;
  const uint32_t *sample, *spans;
  uint64_t rows;
  uint32_t width, L;
  const uint64_t *word_off;
  uint64_t n_samples, n_words;
  uint32_t strategy;
  int32_t *label;
  float *score;
  int32_t *row, *col, *ncols;
  uint32_t *char_start, *char_end;
  float *word_logits;
  uint64_t *info;
};

static int predict_check(const PredictCall &c) {
  if (int rc = lb_check_null({{"logits", c.logits, 0, 4, true, false}, {"word", c.word, 0, 4, true, false}, {"spans", c.spans, 0, 4, true, false},
                              {"word_off", c.word_off, 0, 8, true, false}}))
    return rc;
  if (int rc = lb_check_rows(c.rows, c.width, c.n_samples, c.seq, c.side)) return rc;
  if (c.rows > 0x7FFFFFFFull) return fail(SWT_ERR_INVALID, "rows: 2^31 rows or more");
  if (!c.L) return fail(SWT_ERR_INVALID, "n_labels: logits of no label");
  if (c.strategy >= kTgStrategies) return fail(SWT_ERR_INVALID, "strategy: unknown strategy");
  const uint64_t most = ((1ull << 40) - 1) / c.L, all_cells = c.rows * c.width;  // below 2^63: what lb_check_rows let through
  if (all_cells > most) return fail(SWT_ERR_INVALID, "logits: 2^40 elements or more");
  if (c.n_words > most) return fail(SWT_ERR_INVALID, "n_words: 2^40 elements of out_logits or more");
  if (c.rows && 2 * tg_bits(c.width) + tg_bits(c.rows - 1) > 64)
    return fail(SWT_ERR_INVALID, "width: a run's context, row and column do not fit the 64 bits of its key");
  const size_t cells = (size_t)c.rows * c.width, nw = (size_t)c.n_words * 4;
  return lb_check_layout({{"logits", c.logits, cells * c.L * 4, 4, true, false}, {"word", c.word, cells * 4, 4, true, false},
                          {"seq", c.seq, cells, 1, false, false}, {"sample", c.sample, (size_t)c.rows * 4, 4, false, false},
                          {"spans", c.spans, cells * 8, 4, true, false}, {"word_off", c.word_off, ((size_t)c.n_samples + 1) * 8, 8, true, false},
                          {"out_label", c.label, nw, 4, false, true}, {"out_score", c.score, nw, 4, false, true},
                          {"out_row", c.row, nw, 4, false, true}, {"out_col", c.col, nw, 4, false, true},
                          {"out_ncols", c.ncols, nw, 4, false, true}, {"out_char_start", c.char_start, nw, 4, false, true},
                          {"out_char_end", c.char_end, nw, 4, false, true}, {"out_logits", c.word_logits, nw * c.L, 4, false, true},
                          {"info", c.info, 32, 8, false, true}});
}

struct EntityCall {
  const int32_t *label;
  const float *score;
  const uint32_t *char_start, *char_end;
  const uint64_t *word_off;
  uint64_t n_samples, n_words;
  const int32_t *etype;
  const uint8_t *begins;
  uint32_t L;
  int32_t *text, *type, *first, *last;
  uint32_t *out_start, *out_end;
  float *out_score;
  uint64_t *info;
};

static int entity_check(const EntityCall &c) {
  if (int rc = lb_check_null({{"word_off", c.word_off, 0, 8, true, false}, {"etype", c.etype, 0, 4, true, false}, {"begins", c.begins, 0, 1, true, false}}))
    return rc;
  if (c.n_words)
    if (int rc = lb_check_null({{"label", c.label, 0, 4, true, false}, {"score", c.score, 0, 4, true, false},
                                {"char_start", c.char_start, 0, 4, true, false}, {"char_end", c.char_end, 0, 4, true, false},
                                {"ent_text", c.text, 0, 4, true, true}, {"ent_type", c.type, 0, 4, true, true},
                                {"ent_first_word", c.first, 0, 4, true, true}, {"ent_last_word", c.last, 0, 4, true, true},
                                {"ent_char_start", c.out_start, 0, 4, true, true}, {"ent_char_end", c.out_end, 0, 4, true, true},
                                {"ent_score", c.out_score, 0, 4, true, true}}))
      return rc;
  if (c.n_samples > 0xFFFFFFFFull) return fail(SWT_ERR_INVALID, "n_samples: 2^32 texts or more");
  if (c.n_words >> 40) return fail(SWT_ERR_INVALID, "n_words: 2^40 words or more");
  if (!c.L) return fail(SWT_ERR_INVALID, "n_labels: a scheme of no label");
  const size_t nw = (size_t)c.n_words * 4;
  return lb_check_layout({{"label", c.label, nw, 4, false, false}, {"score", c.score, nw, 4, false, false},
                          {"char_start", c.char_start, nw, 4, false, false}, {"char_end", c.char_end, nw, 4, false, false},
                          {"word_off", c.word_off, ((size_t)c.n_samples + 1) * 8, 8, true, false}, {"etype", c.etype, (size_t)c.L * 4, 4, true, false},
                          {"begins", c.begins, c.L, 1, true, false}, {"ent_text", c.text, nw, 4, false, true}, {"ent_type", c.type, nw, 4, false, true},
                          {"ent_first_word", c.first, nw, 4, false, true}, {"ent_last_word", c.last, nw, 4, false, true},
                          {"ent_char_start", c.out_start, nw, 4, false, true}, {"ent_char_end", c.out_end, nw, 4, false, true},
                          {"ent_score", c.out_score, nw, 4, false, true}, {"info", c.info, 16, 8, false, true}});
}

// what the host forms ask of the offsets: they do not decrease and end at or below the words
static int tg_check_offsets(const uint64_t *word_off, uint64_t n_samples, uint64_t n_words) {
  for (uint64_t s = 0; s < n_samples; s++)
    if (word_off[s] > word_off[s + 1]) return fail(SWT_ERR_INVALID, "word_off: offsets must not decrease");
  if (word_off[n_samples] > n_words) return fail(SWT_ERR_INVALID, "word_off runs past the n_words words");
  return SWT_OK;
}

static int tg_check_sample(const uint32_t *sample, uint64_t rows) {
  if (sample)
    for (uint64_t r = 1; r < rows; r++)
      if (sample[r] < sample[r - 1]) return fail(SWT_ERR_INVALID, "sample: a text's rows are contiguous, the texts in order");
  return SWT_OK;
}

static unsigned tg_grid(uint64_t n) { return (unsigned)((n + kLbThreads - 1) / kLbThreads); }

}  // namespace swt

using namespace swt;

extern "C" {

int swt_tag_capacity(uint32_t *cols_per_step, uint32_t *text_rows, uint32_t *scan_words) try {
  if (cols_per_step) *cols_per_step = kBtCols;
  if (text_rows) *text_rows = kLbThreads;
  if (scan_words) *scan_words = kBtScanGroup;
  return SWT_OK;
} SWT_API_CATCH

int swt_word_plan_dev(const uint32_t *d_word, const int8_t *d_seq, int32_t side, const uint32_t *d_sample, uint64_t rows, uint32_t width,
                      uint64_t n_samples, uint64_t *d_out_word_off, uint64_t *d_info, void *stream) try {
  int rc = plan_check({d_word, d_seq, side, d_sample, rows, width, n_samples, d_out_word_off, d_info});
  if (rc) return rc;
  if ((rc = ensure_device())) return rc;
  hipStream_t st = (hipStream_t)stream;
  SWT_HIP(hipMemsetAsync(d_info, 0, 16, st));
  SWT_HIP(hipMemsetAsync(d_out_word_off, 0, ((size_t)n_samples + 1) * 8, st));
  if (!rows) return SWT_OK;
  PlanArgs A{{d_word, d_seq, d_sample, (uint32_t)side, rows, n_samples, width, 0, 0, 1, 1}, nullptr,
             reinterpret_cast<unsigned long long *>(d_out_word_off), nullptr};
  const unsigned grid = lb_shape(A.R);
  const size_t row_bytes = lb_round((size_t)rows * 8);
  if (n_samples && (rc = g_batch_ws.reserve(n_samples))) return rc;
  if ((rc = g_tag_ws.reserve(row_bytes + (size_t)grid * 8))) return rc;
  A.row_words = g_tag_ws.as<unsigned long long>();
  A.part = reinterpret_cast<unsigned long long *>(g_tag_ws.as<uint8_t>() + row_bytes);
  hipLaunchKernelGGL(tag_row_words_kernel, dim3(grid), dim3(kLbThreads), 0, st, A);
  if (n_samples) {
    hipLaunchKernelGGL(tag_text_words_kernel, dim3(tg_grid(rows)), dim3(kLbThreads), 0, st, A);
    launch_scan_bases(n_samples, A.word_off, d_info, st);
  }
  launch_counts_sum(A.part, grid, 1, reinterpret_cast<unsigned long long *>(d_info) + 1, st);
  SWT_HIP(hipGetLastError());
  return SWT_OK;
} SWT_API_CATCH

int swt_word_plan(const uint32_t *word, const int8_t *seq, int32_t side, const uint32_t *sample, uint64_t rows, uint32_t width,
                  uint64_t n_samples, uint64_t *out_word_off, uint64_t *info) try {
  int rc = plan_check({word, seq, side, sample, rows, width, n_samples, out_word_off, info});
  if (rc) return rc;
  if ((rc = tg_check_sample(sample, rows))) return rc;
  info[0] = info[1] = 0;
  for (uint64_t s = 0; s <= n_samples; s++) out_word_off[s] = 0;
  if (!rows) return SWT_OK;
  if ((rc = ensure_device())) return rc;
  const size_t cells = (size_t)rows * width;
  BatchStage s;
  const uint32_t *d_word = s.in(word, cells * 4), *d_sample = s.in(sample, (size_t)rows * 4);
  const int8_t *d_seq = s.in(seq, cells);
  uint64_t *d_off = s.out(out_word_off, ((size_t)n_samples + 1) * 8), *d_info = s.out(info, 16);
  if (s.rc) return s.rc;
  if ((rc = swt_word_plan_dev(d_word, d_seq, side, d_sample, rows, width, n_samples, d_off, d_info, nullptr))) return rc;
  return s.fetch();
} SWT_API_CATCH

int swt_word_predict_dev(const float *d_logits, const uint32_t *d_word, const int8_t *d_seq, int32_t side, const uint32_t *d_sample,
                         const uint32_t *d_spans, uint64_t rows, uint32_t width, uint32_t n_labels, const uint64_t *d_word_off,
                         uint64_t n_samples, uint64_t n_words, uint32_t strategy, int32_t *d_out_label, float *d_out_score, int32_t *d_out_row,
                         int32_t *d_out_col, int32_t *d_out_ncols, uint32_t *d_out_char_start, uint32_t *d_out_char_end, float *d_out_logits,
                         uint64_t *d_info, void *stream) try {
  int rc = predict_check({d_logits, d_word, d_seq, side, d_sample, d_spans, rows, width, n_labels, d_word_off, n_samples, n_words, strategy,
                          d_out_label, d_out_score, d_out_row, d_out_col, d_out_ncols, d_out_char_start, d_out_char_end, d_out_logits, d_info});
  if (rc) return rc;
  if ((rc = ensure_device())) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (d_info) SWT_HIP(hipMemsetAsync(d_info, 0, 32, st));
  if (!n_words && !rows) return SWT_OK;
  TagArgs A{{d_word, d_seq, d_sample, (uint32_t)side, rows, n_samples, width, 0, 0, 1, 1}, d_logits, n_labels, strategy, d_spans,
            reinterpret_cast<const unsigned long long *>(d_word_off), n_words, nullptr, rows ? tg_bits(rows - 1) : 0, tg_bits(width),
            d_out_label, d_out_score, d_out_row, d_out_col, d_out_ncols, d_out_char_start, d_out_char_end, d_out_logits, nullptr, nullptr};
  const unsigned grid = rows ? lb_shape(A.R) : 0, word_grid = tg_grid(n_words);
  const size_t key_bytes = lb_round((size_t)n_words * 8);
  if ((rc = g_tag_ws.reserve(key_bytes + (3 * (size_t)grid + word_grid) * 8 + 16))) return rc;
  A.key = g_tag_ws.as<unsigned long long>();
  unsigned long long *part = reinterpret_cast<unsigned long long *>(g_tag_ws.as<uint8_t>() + key_bytes), *info = reinterpret_cast<unsigned long long *>(d_info);
  if (n_words) SWT_HIP(hipMemsetAsync(A.key, 0, (size_t)n_words * 8, st));
  if (rows) {
    if (d_info) A.part0 = part + 2 * (size_t)grid;  // the runs that take no part
    hipLaunchKernelGGL(tag_runs_kernel<false>, dim3(grid), dim3(kLbThreads), 0, st, A);
    if (d_info) {
      launch_counts_sum(A.part0, grid, 1, info + 3, st);
      A.part0 = part;
      A.part1 = part + grid;
    }
    hipLaunchKernelGGL(tag_runs_kernel<true>, dim3(grid), dim3(kLbThreads), 0, st, A);
    if (d_info) {
      launch_counts_sum(A.part0, grid, 1, info, st);
      launch_counts_sum(A.part1, grid, 1, info + 2, st);
    }
  }
  if (n_words) {
    if (d_info) A.part0 = part + 3 * (size_t)grid;
    hipLaunchKernelGGL(tag_missing_kernel, dim3(word_grid), dim3(kLbThreads), 0, st, A);
    if (d_info) launch_counts_sum(A.part0, word_grid, 1, info + 1, st);
  }
  SWT_HIP(hipGetLastError());
  return SWT_OK;
} SWT_API_CATCH

int swt_word_predict(const float *logits, const uint32_t *word, const int8_t *seq, int32_t side, const uint32_t *sample, const uint32_t *spans,
                     uint64_t rows, uint32_t width, uint32_t n_labels, const uint64_t *word_off, uint64_t n_samples, uint64_t n_words,
                     uint32_t strategy, int32_t *out_label, float *out_score, int32_t *out_row, int32_t *out_col, int32_t *out_ncols,
                     uint32_t *out_char_start, uint32_t *out_char_end, float *out_logits, uint64_t *info) try {
  int rc = predict_check({logits, word, seq, side, sample, spans, rows, width, n_labels, word_off, n_samples, n_words, strategy, out_label,
                          out_score, out_row, out_col, out_ncols, out_char_start, out_char_end, out_logits, info});
  if (rc) return rc;
  if ((rc = tg_check_sample(sample, rows))) return rc;
  if ((rc = tg_check_offsets(word_off, n_samples, n_words))) return rc;
  if (info) info[0] = info[1] = info[2] = info[3] = 0;
  if (!rows) {  // every word's "nothing" record, without a device
    for (uint64_t w = 0; w < n_words; w++) {
      if (out_label) out_label[w] = -1;
      if (out_score) out_score[w] = 0.f;
      if (out_row) out_row[w] = -1;
      if (out_col) out_col[w] = -1;
      if (out_ncols) out_ncols[w] = -1;
      if (out_char_start) out_char_start[w] = 0;
      if (out_char_end) out_char_end[w] = 0;
      if (out_logits)
        for (uint32_t l = 0; l < n_labels; l++) out_logits[w * n_labels + l] = NAN;
    }
    if (info) info[1] = n_words;
    return SWT_OK;
  }
  if ((rc = ensure_device())) return rc;
  const size_t cells = (size_t)rows * width, nw = (size_t)n_words * 4;
  BatchStage s;
  const float *d_logits = s.in(logits, cells * n_labels * 4);
  const uint32_t *d_word = s.in(word, cells * 4), *d_sample = s.in(sample, (size_t)rows * 4), *d_spans = s.in(spans, cells * 8);
  const int8_t *d_seq = s.in(seq, cells);
  const uint64_t *d_off = s.in(word_off, ((size_t)n_samples + 1) * 8);
  int32_t *d_label = s.out(out_label, nw), *d_row = s.out(out_row, nw), *d_col = s.out(out_col, nw), *d_ncols = s.out(out_ncols, nw);
  float *d_score = s.out(out_score, nw), *d_wl = s.out(out_logits, nw * n_labels);
  uint32_t *d_cs = s.out(out_char_start, nw), *d_ce = s.out(out_char_end, nw);
  uint64_t *d_info = s.out(info, 32);
  if (s.rc) return s.rc;
  if ((rc = swt_word_predict_dev(d_logits, d_word, d_seq, side, d_sample, d_spans, rows, width, n_labels, d_off, n_samples, n_words, strategy,
                                 d_label, d_score, d_row, d_col, d_ncols, d_cs, d_ce, d_wl, d_info, nullptr)))
    return rc;
  return s.fetch();
} SWT_API_CATCH

int swt_entity_spans_dev(const int32_t *d_label, const float *d_score, const uint32_t *d_char_start, const uint32_t *d_char_end,
                         const uint64_t *d_word_off, uint64_t n_samples, uint64_t n_words, const int32_t *d_etype, const uint8_t *d_begins,
                         uint32_t n_labels, int32_t *d_ent_text, int32_t *d_ent_type, int32_t *d_ent_first_word, int32_t *d_ent_last_word,
                         uint32_t *d_ent_char_start, uint32_t *d_ent_char_end, float *d_ent_score, uint64_t *d_info, void *stream) try {
  int rc = entity_check({d_label, d_score, d_char_start, d_char_end, d_word_off, n_samples, n_words, d_etype, d_begins, n_labels, d_ent_text,
                         d_ent_type, d_ent_first_word, d_ent_last_word, d_ent_char_start, d_ent_char_end, d_ent_score, d_info});
  if (rc) return rc;
  if ((rc = ensure_device())) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (!n_words) {
    if (d_info) SWT_HIP(hipMemsetAsync(d_info, 0, 16, st));
    return SWT_OK;
  }
  EntArgs A{d_label, d_score, d_char_start, d_char_end, reinterpret_cast<const unsigned long long *>(d_word_off), n_samples, n_words, d_etype,
            d_begins, n_labels, nullptr, d_ent_text, d_ent_type, d_ent_first_word, d_ent_last_word, d_ent_char_start, d_ent_char_end,
            d_ent_score, nullptr};
  const unsigned grid = tg_grid(n_words);
  const size_t head_bytes = lb_round(((size_t)n_words + 1) * 8);
  if ((rc = g_batch_ws.reserve(n_words))) return rc;
  if ((rc = g_tag_ws.reserve(head_bytes + ((size_t)grid + 1) * 8))) return rc;
  A.head = g_tag_ws.as<unsigned long long>();
  unsigned long long *part = reinterpret_cast<unsigned long long *>(g_tag_ws.as<uint8_t>() + head_bytes);
  if (d_info) A.part = part;
  hipLaunchKernelGGL(ent_head_kernel, dim3(grid), dim3(kLbThreads), 0, st, A);
  launch_scan_bases(n_words, A.head, d_info ? d_info : reinterpret_cast<uint64_t *>(part + grid), st);
  hipLaunchKernelGGL(ent_scatter_kernel, dim3(grid), dim3(kLbThreads), 0, st, A);
  if (d_info) launch_counts_sum(part, grid, 1, reinterpret_cast<unsigned long long *>(d_info) + 1, st);
  SWT_HIP(hipGetLastError());
  return SWT_OK;
} SWT_API_CATCH

int swt_entity_spans(const int32_t *label, const float *score, const uint32_t *char_start, const uint32_t *char_end, const uint64_t *word_off,
                     uint64_t n_samples, uint64_t n_words, const int32_t *etype, const uint8_t *begins, uint32_t n_labels, int32_t *ent_text,
                     int32_t *ent_type, int32_t *ent_first_word, int32_t *ent_last_word, uint32_t *ent_char_start, uint32_t *ent_char_end,
                     float *ent_score, uint64_t *info) try {
  int rc = entity_check({label, score, char_start, char_end, word_off, n_samples, n_words, etype, begins, n_labels, ent_text, ent_type,
                         ent_first_word, ent_last_word, ent_char_start, ent_char_end, ent_score, info});
  if (rc) return rc;
  if ((rc = tg_check_offsets(word_off, n_samples, n_words))) return rc;
  if (info) info[0] = info[1] = 0;
  if (!n_words) return SWT_OK;
  if ((rc = ensure_device())) return rc;
  const size_t nw = (size_t)n_words * 4;
  BatchStage s;
  const int32_t *d_label = s.in(label, nw), *d_etype = s.in(etype, (size_t)n_labels * 4);
  const float *d_score = s.in(score, nw);
  const uint32_t *d_cs = s.in(char_start, nw), *d_ce = s.in(char_end, nw);
  const uint64_t *d_off = s.in(word_off, ((size_t)n_samples + 1) * 8);
  const uint8_t *d_begins = s.in(begins, n_labels);
  int32_t *d_text = s.out(ent_text, nw), *d_type = s.out(ent_type, nw), *d_first = s.out(ent_first_word, nw), *d_last = s.out(ent_last_word, nw);
  uint32_t *d_start = s.out(ent_char_start, nw), *d_end = s.out(ent_char_end, nw);
  float *d_es = s.out(ent_score, nw);
  uint64_t *d_info = s.out(info, 16);
  if (s.rc) return s.rc;
  if ((rc = swt_entity_spans_dev(d_label, d_score, d_cs, d_ce, d_off, n_samples, n_words, d_etype, d_begins, n_labels, d_text, d_type, d_first,
                                 d_last, d_start, d_end, d_es, d_info, nullptr)))
    return rc;
  return s.fetch();
} SWT_API_CATCH

}  // extern "C"
