// sort_plan_host.cpp — elprep_amd/csrc/sort_plan.hpp behind C functions, for tests/test_sort_plan_cpu.py.  The header is host
// arithmetic: this file is built by the host compiler alone.
#include "../elprep_amd/csrc/sort_plan.hpp"

using namespace elp;

extern "C" {

// ---- key format
int sp_index_bits(uint64_t n) { return index_bits(n); }
int sp_sort_words(int key_bits, int idx_bits, int sort_pairs) { return sort_words(key_bits, idx_bits, sort_pairs); }
void sp_key_width(uint32_t max_pos, int32_t n_ref, int *out /* pos_bits, ref_bits, key_bits */) {
  const KeyWidth k = key_width(max_pos, n_ref);
  out[0] = k.pos_bits; out[1] = k.ref_bits; out[2] = k.key_bits;
}

// ---- long runs
uint32_t sp_bounds_cap(uint64_t n) { return bounds_cap(n); }
uint32_t sp_bounds_head(uint32_t cap) { return bounds_head(cap); }
int sp_bounds_in_head(uint32_t nr) { return bounds_in_head(nr); }
int sp_run_counts_ok(uint32_t n_starts, uint32_t n_ends, uint32_t cap) { return run_counts_ok(n_starts, n_ends, cap); }
int sp_segbits(uint32_t nr) { return segbits(nr); }
// starts_out: n_starts words, first_out: n_starts + 1 words, counts: nr, nu.  Returns 0 where the plan refuses the bounds
int sp_long_runs(const uint32_t *starts, uint32_t n_starts, const uint32_t *ends, uint32_t n_ends, uint32_t *starts_out, uint32_t *first_out, uint32_t *counts) {
  LongRuns r;
  if (!long_runs(std::vector<uint32_t>(starts, starts + n_starts), std::vector<uint32_t>(ends, ends + n_ends), &r)) return 0;
  std::copy(r.starts.begin(), r.starts.end(), starts_out);
  std::copy(r.first.begin(), r.first.end(), first_out);
  counts[0] = r.nr; counts[1] = r.nu;
  return 1;
}

// ---- layout
void sp_sort_scratch(uint64_t n, uint64_t *out /* keys, vals, flags, cap, starts, ends */) {
  const SortScratch s(n);
  const uint64_t v[6] = {s.keys, s.vals, s.flags, s.cap, s.starts, s.ends};
  for (int k = 0; k < 6; k++) out[k] = v[k];
}
// out: m_bytes, rw, use_rows, u_pos, u_read, u_seg, uv0, uv1, d_start, d_first, u_words, words3, uk0, uk1, words4, d_vals, d_lut, words5
void sp_tie_scratch(uint32_t nu, uint32_t nr, uint32_t maxq, uint64_t *out) {
  const TieScratch t(nu, nr, maxq);
  const uint64_t v[18] = {t.m_bytes, t.rw, t.use_rows, t.u_pos, t.u_read, t.u_seg, t.uv0, t.uv1, t.d_start, t.d_first, t.u_words, t.words3,
                          t.uk0, t.uk1, t.words4, t.d_vals, t.d_lut, t.words5};
  for (int k = 0; k < 18; k++) out[k] = v[k];
}
void sp_qn_scratch(uint32_t maxq, uint64_t *out /* vwords, d_over, d_lut, lut_words, words3 */) {
  const QnScratch q(maxq);
  const uint64_t v[5] = {q.vwords, q.d_over, q.d_lut, q.lut_words, q.words3};
  for (int k = 0; k < 5; k++) out[k] = v[k];
}

// ---- rank tables
int sp_value_count(const uint32_t *set) { return value_count(set); }
int sp_rank_row(const uint32_t *set, uint8_t *row) { return rank_row(set, row); }
int sp_rank_bits(int nvalues) { return rank_bits(nvalues); }
int sp_live_positions(const uint32_t *live, uint32_t m_bytes, uint16_t *out) {
  const std::vector<uint16_t> lp = live_positions(live, m_bytes);
  std::copy(lp.begin(), lp.end(), out);
  return (int)lp.size();
}
int sp_rank_keys_apply(uint64_t nlive) { return rank_keys_apply((size_t)nlive); }
static int fields_out(const RankFields &f, uint16_t *pos, uint16_t *slot, int *bits, uint8_t *lut, int *lut_rows) {
  std::copy(f.pos.begin(), f.pos.end(), pos);
  std::copy(f.slot.begin(), f.slot.end(), slot);
  std::copy(f.bits.begin(), f.bits.end(), bits);
  std::copy(f.lut.begin(), f.lut.end(), lut);
  *lut_rows = (int)(f.lut.size() / 256);
  return f.n();
}
// pos, slot, bits: room for every field; lut: 256 bytes for every position
int sp_tie_fields(const uint16_t *lp, uint32_t nlp, const uint32_t *sets, uint16_t *pos, uint16_t *slot, int *bits, uint8_t *lut, int *lut_rows) {
  return fields_out(tie_fields(std::vector<uint16_t>(lp, lp + nlp), sets), pos, slot, bits, lut, lut_rows);
}
int sp_qn_fields(const uint32_t *sets, uint32_t maxq, int any_not_output, uint16_t *pos, uint16_t *slot, int *bits, uint8_t *lut, int *lut_rows) {
  return fields_out(qn_fields(sets, maxq, any_not_output != 0), pos, slot, bits, lut, lut_rows);
}

// ---- packing
void sp_pack_prefix(const int *bits, int n, int reserved, int *out /* lo, hi, total */) {
  const FieldCut c = pack_prefix(std::vector<int>(bits, bits + n), reserved);
  out[0] = c.lo; out[1] = c.hi; out[2] = c.total;
}
int sp_key_then_compare(int tie_rounds, int reserved, int first_bits) { return key_then_compare(tie_rounds, reserved, first_bits); }
static int cuts_out(const std::vector<FieldCut> &cuts, int *out) {
  for (size_t k = 0; k < cuts.size(); k++) { out[3 * k] = cuts[k].lo; out[3 * k + 1] = cuts[k].hi; out[3 * k + 2] = cuts[k].total; }
  return (int)cuts.size();
}
int sp_lsd_cuts(const int *bits, int n, int *out /* lo, hi, total per cut: room for n cuts */) { return cuts_out(lsd_cuts(std::vector<int>(bits, bits + n)), out); }
int sp_byte_cuts(uint64_t nlive, int *out) { return cuts_out(byte_cuts((size_t)nlive), out); }
void sp_field_shifts(const int *bits, int n, int lo, int hi, int total, uint8_t *shift /* hi - lo */) {
  field_shifts(std::vector<int>(bits, bits + n), FieldCut{lo, hi, total}, shift);
}
int sp_key_digits(int key_bits) { return key_digits(key_bits); }

// ---- the constants
void sp_constants(int *out /* TIE_SMALL, TIE_HEAD, TIE_MAX_PACKED, QN_STATE, QN_LEN */) {
  out[0] = TIE_SMALL; out[1] = (int)TIE_HEAD; out[2] = TIE_MAX_PACKED; out[3] = QN_STATE; out[4] = QN_LEN;
}

}  // extern "C"
