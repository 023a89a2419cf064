// sw_core.hpp — the HaplotypeCaller's Smith-Waterman (runSmithWaterman, filters/sw.go:110-316; lastIndex, :96-108) as host-and-device
// code: what one lane does in one step of the sweep, where a backtrack cell lives, the end search as a reduction, the traceback's two
// moves, the three strategy tails and the clean-up loop.  sw.hip walks it with a wave per problem; tests/sw_host.cpp walks it the same
// way with lane loops on the CPU (the __HIPCC__ switch below is the attribute switch for that emulation, nothing else).
//
// The sweep.  A wave takes the alternate in tiles of SW_TILE = 64 x SW_COLS columns.  In a tile lane l owns the SW_COLS columns from
// j0 = tile * SW_TILE + l * SW_COLS on and keeps lastRow[j], bestGapV[j] and gapSizeV[j] of them (SwLane); at step t it computes row
// t - l + 1 of its strip (sw_strip_row) from what the lane to its left left behind one step earlier: curRow[j0], bestGapH[i] and
// gapSizeH[i] (SwLeft).  Lane 0 takes them from the matrix's first column, or from the right edge the tile before it wrote.  The score
// matrix is never stored: the end search (:212-238) needs its last column - the lane that owns column n sees it row by row, in order -
// and its bottom row, which the lanes reduce (sw_bottom_key).  The backtrack (0, -ki or kd, :199-208) is stored as int16: a sequence is
// at most SW_MAX_LEN = 4095 long, so a gap length fits.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define ELP_SW_HD __host__ __device__ __forceinline__
#else
#define ELP_SW_HD inline
#endif

namespace elp {

constexpr uint32_t SW_MAX_LEN = 4095;    // longest sequence: a gap length fits the backtrack's int16
constexpr int32_t SW_MAX_PARAM = 65535;  // largest |parameter|: MinInt32 / 2 - 4095 * 65535 = -1342107649 > MinInt32, and a score is a sum
                                         // of at most 8190 parameters, within +-536731650 < 2^30: no int32 of the reference wraps
constexpr uint32_t SW_COLS = 4;          // columns per lane: one 8-byte backtrack store per lane and step
constexpr uint32_t SW_TILE = 64 * SW_COLS;
constexpr int32_t SW_MIN_CUTOFF = -100000000;  // matrixMinCutoff, sw.go:132
constexpr int32_t SW_LOW_INIT = INT32_MIN / 2; // lowInitValue, sw.go:133

enum : int32_t { SW_SOFTCLIP = 0, SW_INDEL = 1, SW_LEADING_INDEL = 2, SW_IGNORE = 3 };  // sw.go:31-36
enum : uint32_t { SW_OP_M = 0, SW_OP_I = 1, SW_OP_D = 2, SW_OP_S = 4 };                 // BAM's codes

struct SwParams {
  int32_t match, mismatch, gap_open, gap_extend, strategy;
};

// fasta.ToUpperAndN (fasta/fasta-files.go:126-151): acgtn / ACGTN -> ACGTN, the other IUPAC letters in either case -> N, the rest stays
ELP_SW_HD uint8_t sw_to_upper_and_n(uint8_t c) {
  const uint8_t u = (c >= 'a' && c <= 'z') ? (uint8_t)(c - 32) : c;
  switch (u) {
    case 'A': case 'C': case 'G': case 'T': case 'N': return u;
    case 'R': case 'Y': case 'M': case 'K': case 'W': case 'S': case 'B': case 'D': case 'H': case 'V': return 'N';
    default: return c;
  }
}
// one candidate offset of lastIndex (:98-105): the normalised reference against the raw alternate
ELP_SW_HD bool sw_occurs_at(const uint8_t *ref, const uint8_t *alt, uint32_t alt_len, uint32_t r) {
  uint32_t q = 0;
  while (q < alt_len && sw_to_upper_and_n(ref[r + q]) == alt[q]) q++;
  return q == alt_len;
}

// ---- the backtrack's layout.  Tile q of a problem of m x n cells has L lanes (64, the last tile ceil(width / SW_COLS)) and m + L - 1
// steps; step t holds L x SW_COLS cells, lane l's four at (t * L + l) * SW_COLS: what the wave stores in one step is one contiguous run.
// Cell (i, j), 1-based, belongs to lane l = ((j - 1) % SW_TILE) / SW_COLS at step i - 1 + l.
ELP_SW_HD uint32_t sw_tiles(uint32_t n) { return (n + SW_TILE - 1) / SW_TILE; }
ELP_SW_HD uint32_t sw_tile_lanes(uint32_t n, uint32_t q) {
  return q + 1 < sw_tiles(n) ? 64u : (n - q * SW_TILE + SW_COLS - 1) / SW_COLS;
}
ELP_SW_HD uint64_t sw_full_tile_cells(uint32_t m) { return (uint64_t)(m + 63) * SW_TILE; }
ELP_SW_HD uint64_t sw_bt_cells(uint32_t m, uint32_t n) {  // a multiple of SW_COLS
  const uint32_t nt = sw_tiles(n), L = sw_tile_lanes(n, nt - 1);
  return (uint64_t)(nt - 1) * sw_full_tile_cells(m) + (uint64_t)(m + L - 1) * L * SW_COLS;
}
ELP_SW_HD uint64_t sw_bt_index(uint32_t m, uint32_t n, uint32_t i, uint32_t j) {
  const uint32_t q = (j - 1) / SW_TILE, jj = (j - 1) % SW_TILE, l = jj / SW_COLS, c = jj % SW_COLS, L = sw_tile_lanes(n, q);
  return (uint64_t)q * sw_full_tile_cells(m) + ((uint64_t)(i - 1 + l) * L + l) * SW_COLS + c;
}

// ---- the matrix's first row and first column (:141-156): 0, or under indel / leadingIndel gapOpen + (idx - 1) * gapExtend - not clamped
ELP_SW_HD int32_t sw_border(const SwParams &p, uint32_t idx) {
  if (idx == 0 || (p.strategy != SW_INDEL && p.strategy != SW_LEADING_INDEL)) return 0;
  return p.gap_open + (int32_t)(idx - 1) * p.gap_extend;
}

struct SwLeft {  // of the lane's row i: curRow[j0], bestGapH[i], gapSizeH[i] as the columns up to j0 leave them
  int32_t cur, gap, size;
};
struct SwLane {
  int32_t last[SW_COLS];  // lastRow over the strip
  int32_t gap[SW_COLS];   // bestGapV
  int32_t size[SW_COLS];  // gapSizeV
  int32_t diag;           // lastRow[j0]
  uint32_t bases;         // the strip's alternate bytes, column c in byte c (0 behind the alternate's end: those cells are computed and
                          // never read - nothing to their right exists)
};
ELP_SW_HD void sw_lane_init(const SwParams &p, SwLane &s, uint32_t j0, uint32_t bases) {
  for (uint32_t c = 0; c < SW_COLS; c++) {
    s.last[c] = sw_border(p, j0 + 1 + c);
    s.gap[c] = SW_LOW_INIT;
    s.size[c] = 0;
  }
  s.diag = sw_border(p, j0);
  s.bases = bases;
}
ELP_SW_HD SwLeft sw_first_column(const SwParams &p, uint32_t i) { return SwLeft{sw_border(p, i), SW_LOW_INIT, 0}; }

// one row of a strip (:166-209).  bt: the four backtrack values.  Returns what the lane to the right needs.
ELP_SW_HD SwLeft sw_strip_row(const SwParams &p, SwLane &s, uint8_t a_base, SwLeft in, int16_t *bt) {
  int32_t left = in.cur, gh = in.gap, ghs = in.size, diag = s.diag;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (uint32_t c = 0; c < SW_COLS; c++) {
    const uint8_t b_base = (uint8_t)(s.bases >> (8 * c));
    const int32_t up = s.last[c];
    const int32_t step_diag = diag + (a_base == b_base ? p.match : p.mismatch);
    int32_t gv = s.gap[c] + p.gap_extend, gvs = s.size[c] + 1;  // += gapExtend first, then the strict test (:175-182)
    if (up + p.gap_open > gv) { gv = up + p.gap_open; gvs = 1; }
    gh += p.gap_extend;
    ghs += 1;
    if (left + p.gap_open > gh) { gh = left + p.gap_open; ghs = 1; }
    int32_t cur, b;
    if (step_diag >= gv && step_diag >= gh) { cur = step_diag; b = 0; }  // diagonal if >= both; else right if >= down; else down
    else if (gh >= gv) { cur = gh; b = -ghs; }
    else { cur = gv; b = gvs; }
    cur = cur > SW_MIN_CUTOFF ? cur : SW_MIN_CUTOFF;
    s.gap[c] = gv;
    s.size[c] = gvs;
    s.last[c] = cur;
    bt[c] = (int16_t)b;
    diag = up;
    left = cur;
  }
  s.diag = in.cur;
  return SwLeft{left, gh, ghs};
}

// ---- the end search (:212-238).  The last column: rows in order, `>=` - the lane that owns column n calls this once per row.
struct SwColumnBest {
  int32_t score = INT32_MIN, p1 = 0;
};
ELP_SW_HD void sw_column_step(SwColumnBest &b, int32_t score, uint32_t i) {
  if (score >= b.score) { b.score = score; b.p1 = (int32_t)i; }
}
// The bottom row: the scan replaces its best by cell j when the score is larger, or equal and |m - j| smaller than the best's
// |p1 - p2| - which for a best (m, j') is |m - j'|.  "Strictly better in (score, -distance)" is a strict weak order, so the scan ends at
// the FIRST cell that no cell beats, whatever the order in which cells are compared: the largest key below (score, then the smaller
// distance, then the smaller j), and the last column's choice stays unless that cell beats it.
constexpr int64_t SW_NO_KEY = INT64_MIN;
ELP_SW_HD int64_t sw_bottom_key(int32_t score, uint32_t m, uint32_t j) {
  const uint32_t d = m > j ? m - j : j - m;
  return (int64_t)score * (1ll << 24) + (int64_t)((SW_MAX_LEN - d) << 12) + (int64_t)(SW_MAX_LEN - j);
}
struct SwTrace {
  int32_t p1, p2, seg, state, offset;
  uint32_t n_raw;
};
ELP_SW_HD void sw_push(uint32_t *raw, uint32_t cap, SwTrace &t, int32_t len, int32_t op) {
  if (t.n_raw < cap) raw[t.n_raw] = ((uint32_t)len << 4) | (uint32_t)op;
  t.n_raw++;
}
// where the traceback starts, and the optional leading S (:212-244)
ELP_SW_HD SwTrace sw_trace_begin(const SwParams &p, uint32_t m, uint32_t n, SwColumnBest col, int64_t bottom_key, uint32_t *raw, uint32_t cap) {
  SwTrace t{0, (int32_t)n, 0, (int32_t)SW_OP_M, 0, 0};
  if (p.strategy == SW_INDEL) {
    t.p1 = (int32_t)m;
  } else {
    t.p1 = col.p1;
    if (p.strategy != SW_LEADING_INDEL && bottom_key != SW_NO_KEY) {
      const int32_t low = (int32_t)(bottom_key & 0xFFFFFF);
      const int32_t score = (int32_t)((bottom_key - low) / (1ll << 24));
      const int32_t d = (int32_t)SW_MAX_LEN - (low >> 12), j = (int32_t)SW_MAX_LEN - (low & 0xFFF);
      const int32_t d0 = t.p1 > t.p2 ? t.p1 - t.p2 : t.p2 - t.p1;
      if (score > col.score || (score == col.score && d < d0)) {
        t.p1 = (int32_t)m;
        t.p2 = j;
        t.seg = (int32_t)n - j;
      }
    }
  }
  if (t.seg > 0 && p.strategy == SW_SOFTCLIP) {
    sw_push(raw, cap, t, t.seg, SW_OP_S);
    t.seg = 0;
  }
  return t;
}
// the loop body of :246-275 for `run` >= 1 consecutive cells whose backtrack is 0 ...
ELP_SW_HD void sw_trace_diagonal(SwTrace &t, int32_t run, uint32_t *raw, uint32_t cap) {
  if (t.state == (int32_t)SW_OP_M) t.seg += run;
  else { sw_push(raw, cap, t, t.seg, t.state); t.seg = run; t.state = (int32_t)SW_OP_M; }
  t.p1 -= run;
  t.p2 -= run;
}
// ... and for one cell whose backtrack is btr != 0
ELP_SW_HD void sw_trace_gap(SwTrace &t, int32_t btr, uint32_t *raw, uint32_t cap) {
  int32_t state, step;
  if (btr > 0) { state = (int32_t)SW_OP_D; step = btr; t.p1 -= btr; }
  else { state = (int32_t)SW_OP_I; step = -btr; t.p2 += btr; }
  if (state == t.state) t.seg += step;
  else { sw_push(raw, cap, t, t.seg, t.state); t.seg = step; t.state = state; }
}
ELP_SW_HD bool sw_trace_done(const SwTrace &t) { return t.p1 <= 0 || t.p2 <= 0; }
// the three tails (:277-297)
ELP_SW_HD void sw_trace_end(const SwParams &p, SwTrace &t, uint32_t *raw, uint32_t cap) {
  if (p.strategy == SW_SOFTCLIP) {
    sw_push(raw, cap, t, t.seg, t.state);
    if (t.p2 > 0) sw_push(raw, cap, t, t.p2, SW_OP_S);
    t.offset = t.p1;
  } else if (p.strategy == SW_IGNORE) {
    sw_push(raw, cap, t, t.seg + t.p2, t.state);
    t.offset = t.p1 - t.p2;
  } else {
    sw_push(raw, cap, t, t.seg, t.state);
    if (t.p1 > 0) sw_push(raw, cap, t, t.p1, SW_OP_D);
    else if (t.p2 > 0) sw_push(raw, cap, t, t.p2, SW_OP_I);
    t.offset = 0;
  }
}

// ---- the reversal and the clean-up (:299-315) in one pass over the raw list from its end.  The loop there keeps an index i and looks
// at the pair (i - 1, i): a zero-length i - 1 is removed, equal operations are merged into i - 1, otherwise i advances.  After a
// removal the element in FRONT of the removed one is never compared with the one that moved up ([3M 0D 2M] stays 3M 2M), which is
// why the finished prefix below is only ever appended to.  `prev` is element i - 1; the last element is dropped if its length is 0.
// emit(index, word) receives the finished operations in order; returns their number.  n_raw >= 1 (every tail pushes).
template <class Emit>
ELP_SW_HD uint32_t sw_clean(const uint32_t *raw, uint32_t n_raw, Emit emit) {
  uint32_t count = 0, prev = raw[n_raw - 1];
  for (uint32_t at = n_raw - 1; at-- > 0;) {
    const uint32_t cur = raw[at];
    if ((prev >> 4) == 0) prev = cur;
    else if ((prev & 15u) == (cur & 15u)) prev += cur & ~15u;
    else { emit(count++, prev); prev = cur; }
  }
  if ((prev >> 4) != 0) emit(count++, prev);
  return count;
}
struct SwCountOnly {
  ELP_SW_HD void operator()(uint32_t, uint32_t) const {}
};
struct SwStore {
  uint32_t *out;
  uint64_t at, cap;  // stores below cap only
  ELP_SW_HD void operator()(uint32_t idx, uint32_t word) const {
    if (at + idx < cap) out[at + idx] = word;
  }
};

}  // namespace elp
