// bai_plan_host.cpp — elprep_amd/csrc/bai_plan.hpp behind a C interface for tests/test_bai_plan_cpu.py: the member walk, the virtual
// offset, the sizes and the scratch layouts, built by the host compiler alone (g++ -shared -fPIC).
#include "../elprep_amd/csrc/bai_plan.hpp"

using namespace elp;

extern "C" {

void bp_consts(uint64_t *out /* 7 */) {
  out[0] = BAI_PSEUDO_BIN; out[1] = BAI_WINDOW_SHIFT; out[2] = BAI_MAX_END; out[3] = BAI_MAX_COFFSET; out[4] = BAI_MEMBER_MIN; out[5] = BAI_SCAN_TILE;
  out[6] = sizeof(BaiRes);
}
// -> the error kind; out: at, value, n_members, inflated; coff: up to coff_cap entries of the table; text: the refusal as the calls report it
int bp_members(const uint8_t *bgzf, uint64_t n_bytes, uint64_t *out /* 4 */, uint64_t *coff, uint64_t coff_cap, char *text, uint64_t text_cap) {
  const BaiMembers m = bai_members(bgzf, n_bytes);
  out[0] = m.at; out[1] = m.value; out[2] = m.n_members(); out[3] = m.inflated;
  for (size_t k = 0; k < m.coff.size() && k < coff_cap; k++) coff[k] = m.coff[k];
  snprintf(text, text_cap, "%s", m.error ? m.text("elp_index_sorted_bgzf").c_str() : "");
  return (int)m.error;
}
int bp_is_the_stream(const uint8_t *bgzf, uint64_t n_bytes, uint64_t stream_bytes) { return bai_is_the_stream(bai_members(bgzf, n_bytes), stream_bytes) ? 1 : 0; }
uint64_t bp_voff(uint64_t base_coffset, const uint64_t *coff, uint64_t p) { return bai_voff(base_coffset, coff, p); }
int bp_coffsets_fit(uint64_t base_coffset, uint64_t n_bytes) { return bai_coffsets_fit(base_coffset, n_bytes) ? 1 : 0; }
uint64_t bp_contig_bytes(uint64_t n_records, uint64_t n_bins, uint64_t n_chunks, uint64_t n_intv) { return bai_contig_bytes(n_records, n_bins, n_chunks, n_intv); }
uint64_t bp_bin_at(uint64_t bins_before, uint64_t chunks_before) { return bai_bin_at(bins_before, chunks_before); }
uint64_t bp_chunk_at(uint64_t bins, uint64_t chunks_before) { return bai_chunk_at(bins, chunks_before); }
uint64_t bp_intv_at(uint64_t n_bins, uint64_t n_chunks) { return bai_intv_at(n_bins, n_chunks); }
uint64_t bp_total_bytes(uint64_t contig_bytes) { return bai_total_bytes(contig_bytes); }
uint64_t bp_size(uint64_t n_ref, uint64_t n_used, uint64_t n_bins, uint64_t n_chunks, uint64_t n_intv) { return bai_size(n_ref, n_used, n_bins, n_chunks, n_intv); }
void bp_scratch0(uint64_t n, uint64_t *out /* 13 */) {
  const BaiScratch0 s(n);
  const size_t v[13] = {s.start, s.key, s.gmax, s.size, s.val, s.head_bin, s.head_chunk, s.bins, s.chunks, s.unm, s.unms, s.bin_chunk0, s.words64};
  for (int k = 0; k < 13; k++) out[k] = v[k];
}
void bp_scratch1(uint64_t n, uint64_t *out /* 3 */) {
  const BaiScratch1 s(n);
  out[0] = s.key; out[1] = s.val; out[2] = s.words64;
}
void bp_scratch2(uint64_t n_ref, uint64_t n_members, uint64_t n_out, uint64_t *out /* 8 */) {
  const BaiScratch2 s(n_ref, n_members, n_out);
  const size_t v[8] = {s.res, s.coff, s.first, s.end, s.bytes, s.offset, s.partials, s.words64};
  for (int k = 0; k < 8; k++) out[k] = v[k];
}

}  // extern "C"
