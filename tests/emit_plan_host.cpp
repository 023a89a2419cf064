// emit_plan_host.cpp — elprep_amd/csrc/emit_plan.hpp behind C functions, for tests/test_emit_plan_cpu.py.  The header is host
// arithmetic: this file is built by the host compiler alone.
#include "../elprep_amd/csrc/emit_plan.hpp"

using namespace elp;

static OutFormat format_of(int fmt) { return fmt == 0 ? OutFormat::BAM : fmt == 1 ? OutFormat::BGZF : OutFormat::SAM; }

extern "C" {

// out: EMIT_PASS_BYTES, EMIT_PASS_RECORDS, BGZF_PAYLOAD, BGZF_OVERHEAD, BAM_PIECE_BYTES, TAG_TABLE_WORDS, EMIT_SLOT_PAD
void ep_consts(uint64_t *out) {
  const uint64_t v[7] = {EMIT_PASS_BYTES, EMIT_PASS_RECORDS, BGZF_PAYLOAD, BGZF_OVERHEAD, BAM_PIECE_BYTES, TAG_TABLE_WORDS, EMIT_SLOT_PAD};
  for (int k = 0; k < 7; k++) out[k] = v[k];
}

uint64_t ep_rec_bound(int fmt, uint64_t max_raw_rec, uint32_t max_name) { return emit_rec_bound(format_of(fmt), max_raw_rec, max_name); }
uint32_t ep_pass_records(uint64_t rec_bound, int tune_emit_pass) { return emit_pass_records(rec_bound, tune_emit_pass); }

// out: pass_bytes, frame_bytes, carry_bytes, out_bound, the requests of slots 5 and 7
void ep_pass(int fmt, uint64_t held, uint64_t chunk_bytes, int last, uint64_t *out) {
  const EmitPass p = emit_pass(format_of(fmt), held, chunk_bytes, last != 0);
  const uint64_t v[6] = {p.pass_bytes, p.frame_bytes, p.carry_bytes, p.out_bound, p.slot5_bytes(), p.slot7_bytes()};
  for (int k = 0; k < 6; k++) out[k] = v[k];
}
uint64_t ep_query_bytes(int fmt, uint64_t chunk_bytes) { return emit_query_bytes(format_of(fmt), chunk_bytes); }
int ep_fits(uint64_t total, uint64_t out_bound, uint64_t cap) { return emit_fits(total, out_bound, cap) ? 1 : 0; }
uint64_t ep_framed_size(uint64_t n_bytes) { return bgzf_framed_size(n_bytes); }

// out: sizes, offs, err, words
void ep_scratch4(uint32_t cnt, uint64_t *out) {
  const EmitScratch4 s(cnt);
  out[0] = s.sizes; out[1] = s.offs; out[2] = s.err; out[3] = s.words;
}

// words: TAG_TABLE_WORDS entries (left alone when there is no filter); returns 1 = a filter, 0 = none
int ep_tag_table(const uint8_t *remove_keys, int n_remove, const uint8_t *keep_keys, int n_keep, uint32_t *words) {
  const TagDropTable t = tag_drop_table(remove_keys, n_remove, keep_keys, n_keep);
  if (!t.filter) return t.words.empty() ? 0 : -1;
  if (t.words.size() != TAG_TABLE_WORDS) return -1;
  for (size_t w = 0; w < t.words.size(); w++) words[w] = t.words[w];
  return 1;
}

// out: error, at, block_size, records, end, next_rec, max_raw_rec; off: the first `cap` of the records + 1 offsets; text: the error's text
void ep_cut(const uint8_t *bytes, uint64_t n_bytes, const uint64_t *rec_off, uint64_t n_records, uint64_t at_byte, uint64_t at_rec, uint64_t piece_limit,
            uint64_t *out, uint64_t *off, uint64_t cap, char *text, uint64_t text_cap) {
  const BamCut r = bam_cut_piece(bytes, n_bytes, rec_off, n_records, at_byte, at_rec, piece_limit);
  out[0] = r.error; out[1] = r.at; out[2] = r.block_size; out[3] = r.error ? 0 : r.off.size() - 1; out[4] = r.end; out[5] = r.next_rec; out[6] = r.max_raw_rec;
  for (uint64_t k = 0; !r.error && k < r.off.size() && k < cap; k++) off[k] = r.off[k];
  snprintf(text, text_cap, "%s", r.text().c_str());
}

}  // extern "C"
