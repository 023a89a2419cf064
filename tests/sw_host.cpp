// sw_host.cpp - elprep_amd/csrc/sw_core.hpp compiled by the host compiler and walked the way sw.hip's kernels walk it, with loops over
// the 64 lanes where the device has a wave: the shortcut's 64 candidate offsets per turn from the right, the sweep in tiles and strips
// with what a lane hands to its right neighbour one step later, the tile edge, the backtrack cells at their places in a buffer of
// exactly the planned size, the end search as a reduction, the traceback's fetch of 64 diagonal cells, the clean-up in its two passes.
// tests/test_sw_core_cpu.py compares it with tests/swref_c.c on the case lists of tests/sw_cases.py.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../elprep_amd/csrc/sw_core.hpp"
#include "../elprep_amd/csrc/sw_plan.hpp"

using namespace elp;

namespace {

constexpr uint32_t LANES = 64;

int32_t shortcut(const uint8_t *ref, uint32_t m, const uint8_t *alt, uint32_t len) {  // k_sw_shortcut
  for (int32_t top = (int32_t)m - (int32_t)len; top >= 0; top -= 64) {
    for (uint32_t lane = 0; lane < LANES; lane++) {  // (the ballot's lowest lane)
      const int32_t r = top - (int32_t)lane;
      if (r >= 0 && sw_occurs_at(ref, alt, len, (uint32_t)r)) return r;
    }
  }
  return -1;
}

// k_sw_dp; raw: the problem's region of sw_need(m, n).raw_words words.  Returns the cleaned-up count.
uint32_t dp(const uint8_t *ref, uint32_t m, const uint8_t *alt, uint32_t n, const SwParams &p, std::vector<int16_t> &bt, std::vector<int32_t> &edge, uint32_t *raw,
            int32_t *offset_out) {
  const uint32_t raw_cap = m + n + 3, nt = sw_tiles(n);
  SwColumnBest col[LANES];
  int64_t bottom[LANES];
  for (uint32_t l = 0; l < LANES; l++) bottom[l] = SW_NO_KEY;
  for (uint32_t q = 0; q < nt; q++) {
    const uint32_t width = n - q * SW_TILE < SW_TILE ? n - q * SW_TILE : SW_TILE, L = (width + SW_COLS - 1) / SW_COLS;
    SwLane s[LANES];
    SwLeft out[LANES], ahead{0, 0, 0};
    uint8_t a_ahead[LANES];
    for (uint32_t lane = 0; lane < LANES; lane++) {
      const uint32_t j0 = q * SW_TILE + lane * SW_COLS;
      uint32_t bases = 0;
      for (uint32_t c = 0; c < SW_COLS; c++)
        if (j0 + c < n) bases |= (uint32_t)alt[j0 + c] << (8 * c);
      sw_lane_init(p, s[lane], j0, bases);
      out[lane] = SwLeft{0, 0, 0};
      a_ahead[lane] = ref[0];
    }
    ahead = q == 0 ? sw_first_column(p, 1) : SwLeft{edge.at(0), edge.at(1), edge.at(2)};
    int16_t *bt_tile = bt.data() + (uint64_t)q * sw_full_tile_cells(m);
    const uint64_t tile_cells = q + 1 < nt ? sw_full_tile_cells(m) : (uint64_t)(m + L - 1) * L * SW_COLS;
    const uint32_t steps = m + L - 1;
    for (uint32_t t = 0; t < steps; t++) {
      SwLeft in[LANES];
      for (uint32_t lane = 0; lane < LANES; lane++) in[lane] = lane ? out[lane - 1] : out[0];  // the cross-lane move, all lanes at once
      for (uint32_t lane = 0; lane < LANES; lane++) {
        const int32_t i = (int32_t)t - (int32_t)lane + 1;
        if (lane == 0) {
          in[0] = ahead;
          if (t + 1 < m) ahead = q == 0 ? sw_first_column(p, t + 2) : SwLeft{edge.at(3 * (t + 1)), edge.at(3 * (t + 1) + 1), edge.at(3 * (t + 1) + 2)};
        }
        if (lane < L && i >= 1 && i <= (int32_t)m) {
          const uint32_t j0 = q * SW_TILE + lane * SW_COLS;
          const uint8_t a_base = a_ahead[lane];
          if ((uint32_t)i < m) a_ahead[lane] = ref[i];
          int16_t b4[SW_COLS];
          out[lane] = sw_strip_row(p, s[lane], a_base, in[lane], b4);
          const uint64_t at = ((uint64_t)t * L + lane) * SW_COLS;
          if (at + SW_COLS > tile_cells) return ~0u;  // (outside the tile's planned cells)
          for (uint32_t c = 0; c < SW_COLS; c++) bt_tile[at + c] = b4[c];
          if (q + 1 < nt && lane == 63) {
            edge.at(3 * (i - 1)) = out[lane].cur;
            edge.at(3 * (i - 1) + 1) = out[lane].gap;
            edge.at(3 * (i - 1) + 2) = out[lane].size;
          }
          if (q + 1 == nt && lane == (width - 1) / SW_COLS) sw_column_step(col[lane], s[lane].last[(width - 1) % SW_COLS], (uint32_t)i);
          if ((uint32_t)i == m)
            for (uint32_t c = 0; c < SW_COLS; c++)
              if (j0 + c < n) {
                const int64_t key = sw_bottom_key(s[lane].last[c], m, j0 + c + 1);
                bottom[lane] = key > bottom[lane] ? key : bottom[lane];
              }
        }
      }
    }
  }
  const uint32_t owner = ((n - 1) % SW_TILE) / SW_COLS;
  int64_t best = SW_NO_KEY;
  for (uint32_t l = 0; l < LANES; l++) best = bottom[l] > best ? bottom[l] : best;
  SwTrace t = sw_trace_begin(p, m, n, col[owner], best, raw, raw_cap);
  for (uint32_t turns = 0; turns < m + n + 2; turns++) {
    if (t.p1 < 1 || t.p2 < 1 || t.p1 > (int32_t)m || t.p2 > (int32_t)n) break;
    const int32_t lim = t.p1 < t.p2 ? t.p1 : t.p2;
    int32_t v[LANES], run = 64;
    for (uint32_t lane = 0; lane < LANES; lane++) {
      v[lane] = 1;
      if ((int32_t)lane < lim) v[lane] = bt.at(sw_bt_index(m, n, (uint32_t)t.p1 - lane, (uint32_t)t.p2 - lane));
    }
    for (uint32_t lane = 0; lane < LANES; lane++)
      if (v[lane] != 0) { run = (int32_t)lane; break; }
    if (run > 0) sw_trace_diagonal(t, run, raw, raw_cap);
    else sw_trace_gap(t, v[0], raw, raw_cap);
    if (sw_trace_done(t)) break;
  }
  sw_trace_end(p, t, raw, raw_cap);
  if (t.n_raw > raw_cap) return ~0u;
  raw[raw_cap] = t.n_raw;
  *offset_out = t.offset;
  return sw_clean(raw, t.n_raw, SwCountOnly{});
}

}  // namespace

extern "C" {

// one problem as the device runs it; cigar_out: room for len_ref + len_alt + 2 words.  Returns the number of operations, -1 if a
// walk left its planned region
int swh_run(const uint8_t *ref, uint32_t m, const uint8_t *alt, uint32_t n, int32_t match, int32_t mismatch, int32_t gap_open, int32_t gap_extend, int strategy,
            uint32_t *cigar_out, int32_t *offset_out) {
  const SwParams p{match, mismatch, gap_open, gap_extend, strategy};
  if (strategy == SW_SOFTCLIP || strategy == SW_IGNORE) {
    const int32_t r = shortcut(ref, m, alt, n);
    if (r >= 0) {
      cigar_out[0] = (n << 4) | SW_OP_M;
      *offset_out = r;
      return 1;
    }
  }
  const SwNeed need = sw_need(m, n);
  std::vector<int16_t> bt(need.bt_cells, (int16_t)0x7B7B);  // (garbage, not zeros: a cell read before it is written shows)
  std::vector<int32_t> edge(need.edge_words, 0x7B7B7B7B);
  std::vector<uint32_t> raw(need.raw_words, 0x7B7B7B7Bu);
  const uint32_t count = dp(ref, m, alt, n, p, bt, edge, raw.data(), offset_out);
  if (count == ~0u || count > m + n + 2) return -1;
  const uint32_t again = sw_clean(raw.data(), raw[m + n + 3], SwStore{cigar_out, 0, (uint64_t)m + n + 2});  // k_sw_write
  return again == count ? (int)count : -1;
}

int swh_batch(const uint8_t *a, const uint64_t *a_off, const uint8_t *b, const uint64_t *b_off, uint64_t k0, uint64_t k1, const uint32_t *ref_of, const uint32_t *alt_of,
              int32_t match, int32_t mismatch, int32_t gap_open, int32_t gap_extend, int strategy, uint32_t *cigar_out, const uint64_t *slot_off, uint32_t *n_ops_out,
              int32_t *offset_out) {
  for (uint64_t k = k0; k < k1; k++) {
    const uint32_t r = ref_of[k], q = alt_of[k];
    const int n = swh_run(a + a_off[r], (uint32_t)(a_off[r + 1] - a_off[r]), b + b_off[q], (uint32_t)(b_off[q + 1] - b_off[q]), match, mismatch, gap_open, gap_extend,
                          strategy, cigar_out + slot_off[k], offset_out + k);
    if (n < 0) return -1;
    n_ops_out[k] = (uint32_t)n;
  }
  return 0;
}

// sw_bt_index against the strips' own arithmetic, and as a bijection onto [0, sw_bt_cells): 1 if every cell of an m x n problem has a
// place of its own inside the planned cells and lane l's store of step t covers exactly its four
int swh_layout_ok(uint32_t m, uint32_t n) {
  const uint64_t cells = sw_bt_cells(m, n);
  std::vector<uint8_t> seen(cells, 0);
  for (uint32_t i = 1; i <= m; i++)
    for (uint32_t j = 1; j <= n; j++) {
      const uint64_t at = sw_bt_index(m, n, i, j);
      const uint32_t q = (j - 1) / SW_TILE, lane = ((j - 1) % SW_TILE) / SW_COLS, L = sw_tile_lanes(n, q);
      const uint64_t store = (uint64_t)q * sw_full_tile_cells(m) + ((uint64_t)(i - 1 + lane) * L + lane) * SW_COLS + (j - 1) % SW_COLS;
      if (at >= cells || at != store || seen[at]) return 0;
      seen[at] = 1;
    }
  return cells % SW_COLS == 0;
}

}  // extern "C"
