// sw_plan_host.cpp - elprep_amd/csrc/sw_plan.hpp (and the layout arithmetic of sw_core.hpp) behind a C interface for
// tests/test_sw_plan_cpu.py: built by the host compiler, no HIP.
#include <cstring>

#include "../elprep_amd/csrc/sw_plan.hpp"

using namespace elp;

static int refusal(const SwCheck &r, char *text, uint64_t text_cap) {
  if (text && text_cap) snprintf(text, text_cap, "%s", r.text.c_str());
  return (int)r.code;
}

extern "C" {

void sp_consts(uint64_t *out /* 6 */) {
  out[0] = SW_MAX_LEN; out[1] = (uint64_t)SW_MAX_PARAM; out[2] = SW_COLS; out[3] = SW_TILE; out[4] = SW_SCRATCH_DEFAULT; out[5] = sizeof(SwProb);
}
int sp_check_params(int32_t match, int32_t mismatch, int32_t gap_open, int32_t gap_extend, int strategy, char *text, uint64_t text_cap) {
  return refusal(sw_check_params(match, mismatch, gap_open, gap_extend, strategy), text, text_cap);
}
// -> the refusal (0: none); *ops_bound, len_ref, len_alt as sw_check_batch leaves them
int sp_check_batch(uint64_t n_a, const uint64_t *a_off, uint64_t n_b, const uint64_t *b_off, uint64_t n, const uint32_t *ref_of, const uint32_t *alt_of, uint32_t *len_ref,
                   uint32_t *len_alt, uint64_t *ops_bound, char *text, uint64_t text_cap) {
  const SwCheck r = sw_check_batch(n_a, a_off, n_b, b_off, n, ref_of, alt_of, len_ref, len_alt);
  *ops_bound = r.ops_bound;
  return refusal(r, text, text_cap);
}
uint64_t sp_tiles(uint32_t n) { return sw_tiles(n); }
uint64_t sp_tile_lanes(uint32_t n, uint32_t q) { return sw_tile_lanes(n, q); }
uint64_t sp_bt_cells(uint32_t m, uint32_t n) { return sw_bt_cells(m, n); }
void sp_need(uint32_t m, uint32_t n, uint64_t *out /* 4 */) {
  const SwNeed d = sw_need(m, n);
  out[0] = d.bt_cells; out[1] = d.raw_words; out[2] = d.edge_words; out[3] = d.bytes();
}
// the chunks of problems 0 .. n - 1 (all listed): cuts as rows of 5 (first, end, bt_cells, raw_words, edge_words), at most cap rows; the
// problems' three offsets as rows of 3; per chunk the three byte offsets and the size of SwChunk as rows of 4.  Returns the number of chunks.
uint64_t sp_chunks(uint64_t n, const uint32_t *len_ref, const uint32_t *len_alt, uint64_t budget, uint64_t *cuts, uint64_t cap, uint64_t *prob_at, uint64_t *chunk_at) {
  std::vector<SwProb> probs(n);
  for (uint64_t k = 0; k < n; k++) probs[k] = SwProb{(uint32_t)k, 7, 99, 99, 99};
  const std::vector<SwChunkCut> c = sw_chunks(probs, len_ref, len_alt, budget);
  for (uint64_t i = 0; i < c.size() && i < cap; i++) {
    const uint64_t row[5] = {c[i].first, c[i].end, c[i].bt_cells, c[i].raw_words, c[i].edge_words};
    memcpy(cuts + 5 * i, row, sizeof row);
    const SwChunk ch(c[i]);
    const uint64_t at[4] = {ch.bt_at, ch.raw_at, ch.edge_at, ch.bytes};
    memcpy(chunk_at + 4 * i, at, sizeof at);
  }
  for (uint64_t k = 0; k < n; k++) {
    prob_at[3 * k] = probs[k].bt_at; prob_at[3 * k + 1] = probs[k].raw_at; prob_at[3 * k + 2] = probs[k].edge_at;
    if (probs[k].pad != 0 || probs[k].k != k) return ~0ull;
  }
  return c.size();
}
void sp_per_problem(uint64_t n, uint64_t n_listed, uint64_t *out /* 7 */) {
  const SwPerProblem l(n, n_listed);
  const uint64_t v[7] = {l.miss, l.n_ops, l.scan, l.offset, l.cigar_off, l.probs, l.bytes};
  memcpy(out, v, sizeof v);
}
void sp_inputs(uint64_t pool_bytes, uint64_t n_seq, uint64_t n, uint64_t *out /* 6 */) {
  const SwInputs l(pool_bytes, n_seq, n);
  const uint64_t v[6] = {l.seq, l.off, l.idx0, l.idx1, l.idx2, l.bytes};
  memcpy(out, v, sizeof v);
}

}  // extern "C"
