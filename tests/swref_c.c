/* swref_c.c - runSmithWaterman and lastIndex (filters/sw.go:96-316) once more in plain C with the full matrices, written from the Go
 * source: the fast restatement the GPU tests take their expected values from.  It includes nothing of elprep_amd/csrc; tests/swref.py
 * is the readable twin, tests/test_swref_cpu.py holds the two against hand-derived cases and against each other.
 * Built by the host compiler on first use (tests/sw_cases.py: cc -O2 -shared -fPIC). */
#include <stdint.h>
#include <stdlib.h>

enum { SOFTCLIP = 0, INDEL = 1, LEADING_INDEL = 2, IGNORE = 3 };
enum { OP_M = 0, OP_I = 1, OP_D = 2, OP_S = 4 };
#define MATRIX_MIN_CUTOFF (-100000000)
#define LOW_INIT_VALUE (INT32_MIN / 2)

static uint8_t to_upper_and_n(uint8_t c) { /* fasta/fasta-files.go:126-151 */
  switch (c) {
    case 'A': case 'a': return 'A';
    case 'C': case 'c': return 'C';
    case 'G': case 'g': return 'G';
    case 'T': case 't': return 'T';
    case 'N': case 'n': case 'R': case 'r': case 'Y': case 'y': case 'M': case 'm': case 'K': case 'k': case 'W': case 'w':
    case 'S': case 's': case 'B': case 'b': case 'D': case 'd': case 'H': case 'h': case 'V': case 'v': return 'N';
    default: return c;
  }
}

int32_t swref_last_index(const uint8_t *ref, int32_t ref_len, const uint8_t *seq, int32_t seq_len) { /* sw.go:96-108 */
  for (int32_t r = ref_len - seq_len; r >= 0; r--) {
    int32_t q = 0;
    while (q < seq_len && to_upper_and_n(ref[r + q]) == seq[q]) q++;
    if (q == seq_len) return r;
  }
  return -1;
}

typedef struct { int32_t length; int32_t op; } cigar_op;

static int32_t max_i32(int32_t a, int32_t b) { return a > b ? a : b; }
static int32_t abs_i32(int32_t a) { return a < 0 ? -a : a; }

/* cigar_out: room for ref_len + alt_len + 3 words (len << 4 | op); returns the number of ops, or -1 without memory */
int swref_run(const uint8_t *reference, int32_t ref_length, const uint8_t *alternate, int32_t alt_length, int32_t match_value,
              int32_t mismatch_penalty, int32_t gap_open, int32_t gap_extend, int strategy, uint32_t *cigar_out, int32_t *offset_out) {
  if (strategy == SOFTCLIP || strategy == IGNORE) {
    const int32_t off = swref_last_index(reference, ref_length, alternate, alt_length);
    if (off >= 0) {
      cigar_out[0] = ((uint32_t)alt_length << 4) | OP_M;
      *offset_out = off;
      return 1;
    }
  }
  const int32_t nrow = ref_length + 1, ncol = alt_length + 1;
  int32_t *sw = (int32_t *)calloc((size_t)nrow * ncol, sizeof(int32_t));
  int32_t *backtrack = (int32_t *)calloc((size_t)nrow * ncol, sizeof(int32_t));
  int32_t *best_gap_v = (int32_t *)malloc(sizeof(int32_t) * (size_t)(ncol + 1)), *gap_size_v = (int32_t *)calloc((size_t)ncol + 1, sizeof(int32_t));
  int32_t *best_gap_h = (int32_t *)malloc(sizeof(int32_t) * (size_t)(nrow + 1)), *gap_size_h = (int32_t *)calloc((size_t)nrow + 1, sizeof(int32_t));
  cigar_op *lce = (cigar_op *)malloc(sizeof(cigar_op) * (size_t)(ref_length + alt_length + 4));
  if (!sw || !backtrack || !best_gap_v || !gap_size_v || !best_gap_h || !gap_size_h || !lce) {
    free(sw); free(backtrack); free(best_gap_v); free(gap_size_v); free(best_gap_h); free(gap_size_h); free(lce);
    return -1;
  }
  for (int32_t j = 0; j < ncol + 1; j++) best_gap_v[j] = LOW_INIT_VALUE;
  for (int32_t i = 0; i < nrow + 1; i++) best_gap_h[i] = LOW_INIT_VALUE;

  if (strategy == INDEL || strategy == LEADING_INDEL) { /* :141-156 */
    int32_t cur = gap_open;
    if (ncol > 1) sw[1] = gap_open;
    for (int32_t i = 2; i < ncol; i++) { cur += gap_extend; sw[i] = cur; }
    if (nrow > 1) sw[(size_t)1 * ncol] = gap_open;
    cur = gap_open;
    for (int32_t i = 2; i < nrow; i++) { cur += gap_extend; sw[(size_t)i * ncol] = cur; }
  }

  for (int32_t i = 1; i < nrow; i++) { /* :160-210 */
    const uint8_t a_base = reference[i - 1];
    const int32_t *last_row = sw + (size_t)(i - 1) * ncol;
    int32_t *cur_row = sw + (size_t)i * ncol, *bt_row = backtrack + (size_t)i * ncol;
    for (int32_t j = 1; j < ncol; j++) {
      const uint8_t b_base = alternate[j - 1];
      int32_t step_diag = last_row[j - 1];
      if (a_base == b_base) step_diag += match_value; else step_diag += mismatch_penalty;

      int32_t prev_gap = last_row[j] + gap_open;
      best_gap_v[j] += gap_extend;
      if (prev_gap > best_gap_v[j]) { best_gap_v[j] = prev_gap; gap_size_v[j] = 1; } else gap_size_v[j]++;
      const int32_t step_down = best_gap_v[j], kd = gap_size_v[j];

      prev_gap = cur_row[j - 1] + gap_open;
      best_gap_h[i] += gap_extend;
      if (prev_gap > best_gap_h[i]) { best_gap_h[i] = prev_gap; gap_size_h[i] = 1; } else gap_size_h[i]++;
      const int32_t step_right = best_gap_h[i], ki = gap_size_h[i];

      if (step_diag >= step_down && step_diag >= step_right) { cur_row[j] = max_i32(MATRIX_MIN_CUTOFF, step_diag); bt_row[j] = 0; }
      else if (step_right >= step_down) { cur_row[j] = max_i32(MATRIX_MIN_CUTOFF, step_right); bt_row[j] = -ki; }
      else { cur_row[j] = max_i32(MATRIX_MIN_CUTOFF, step_down); bt_row[j] = kd; }
    }
  }

  int64_t max_score = INT32_MIN; /* :212-238 (an int in Go) */
  int32_t segment_length = 0, p1 = 0, p2 = alt_length;
  if (strategy == INDEL) p1 = ref_length;
  else {
    for (int32_t i = 1; i < nrow; i++) {
      const int64_t cur_score = sw[(size_t)i * ncol + alt_length];
      if (cur_score >= max_score) { p1 = i; max_score = cur_score; }
    }
    if (strategy != LEADING_INDEL) {
      const int32_t *bottom = sw + (size_t)ref_length * ncol;
      for (int32_t j = 1; j < ncol; j++) {
        const int64_t cur_score = bottom[j];
        if (cur_score > max_score || (cur_score == max_score && abs_i32(ref_length - j) < abs_i32(p1 - p2))) {
          p1 = ref_length; p2 = j; max_score = cur_score; segment_length = alt_length - j;
        }
      }
    }
  }

  int n = 0; /* :240-275 */
  if (segment_length > 0 && strategy == SOFTCLIP) { lce[n].length = segment_length; lce[n++].op = OP_S; segment_length = 0; }
  int32_t state = OP_M;
  for (;;) {
    int32_t step_length = 1, new_state;
    const int32_t btr = backtrack[(size_t)p1 * ncol + p2];
    if (btr > 0) { new_state = OP_D; step_length = btr; p1 -= btr; }
    else if (btr < 0) { new_state = OP_I; step_length = -btr; p2 += btr; }
    else { new_state = OP_M; p1--; p2--; }
    if (new_state == state) segment_length += step_length;
    else { lce[n].length = segment_length; lce[n++].op = state; segment_length = step_length; state = new_state; }
    if (p1 <= 0 || p2 <= 0) break;
  }

  int32_t offset; /* :277-297 */
  if (strategy == SOFTCLIP) {
    lce[n].length = segment_length; lce[n++].op = state;
    if (p2 > 0) { lce[n].length = p2; lce[n++].op = OP_S; }
    offset = p1;
  } else if (strategy == IGNORE) {
    lce[n].length = segment_length + p2; lce[n++].op = state;
    offset = p1 - p2;
  } else {
    lce[n].length = segment_length; lce[n++].op = state;
    if (p1 > 0) { lce[n].length = p1; lce[n++].op = OP_D; }
    else if (p2 > 0) { lce[n].length = p2; lce[n++].op = OP_I; }
    offset = 0;
  }

  for (int i = 0, j = n - 1; i < j; i++, j--) { const cigar_op t = lce[i]; lce[i] = lce[j]; lce[j] = t; } /* :299-315 */
  for (int i = 1; i < n;) {
    if (lce[i - 1].length == 0) { for (int k = i - 1; k + 1 < n; k++) lce[k] = lce[k + 1]; n--; }
    else if (lce[i - 1].op == lce[i].op) { lce[i - 1].length += lce[i].length; for (int k = i; k + 1 < n; k++) lce[k] = lce[k + 1]; n--; }
    else i++;
  }
  if (lce[n - 1].length == 0) n--;
  for (int i = 0; i < n; i++) cigar_out[i] = ((uint32_t)lce[i].length << 4) | (uint32_t)lce[i].op;
  *offset_out = offset;
  free(sw); free(backtrack); free(best_gap_v); free(gap_size_v); free(best_gap_h); free(gap_size_h); free(lce);
  return n;
}

/* problems k0 .. k1 of a batch in the flat form of elp_sw_align; problem k writes its ops at cigar_out + slot_off[k] (room for
 * len_ref + len_alt + 3) and their number into n_ops_out[k].  Returns 0, or -1 without memory. */
int swref_batch(const uint8_t *a, const uint64_t *a_off, const uint8_t *b, const uint64_t *b_off, uint64_t k0, uint64_t k1, const uint32_t *ref_of,
                const uint32_t *alt_of, int32_t match_value, int32_t mismatch_penalty, int32_t gap_open, int32_t gap_extend, int strategy,
                uint32_t *cigar_out, const uint64_t *slot_off, uint32_t *n_ops_out, int32_t *offset_out) {
  for (uint64_t k = k0; k < k1; k++) {
    const uint32_t r = ref_of[k], q = alt_of[k];
    const int n = swref_run(a + a_off[r], (int32_t)(a_off[r + 1] - a_off[r]), b + b_off[q], (int32_t)(b_off[q + 1] - b_off[q]), match_value, mismatch_penalty,
                            gap_open, gap_extend, strategy, cigar_out + slot_off[k], offset_out + k);
    if (n < 0) return -1;
    n_ops_out[k] = (uint32_t)n;
  }
  return 0;
}
