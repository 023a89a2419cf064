// bgzf_plan_host.cpp — elprep_amd/csrc/bgzf_plan.hpp behind C functions, for tests/test_bgzf_plan_cpu.py.  The header is host
// arithmetic: this file is built by the host compiler alone.
#include "../elprep_amd/csrc/bgzf_plan.hpp"

using namespace elp;

static std::vector<BgzfBlk> blocks_of(const uint32_t *out_len, uint64_t n) {
  std::vector<BgzfBlk> b(n);
  for (uint64_t k = 0; k < n; k++) b[k] = BgzfBlk{0, 0, out_len[k], 0, 0, 0};
  return b;
}

extern "C" {

// out: TOK_STRIDE, RES_THREADS, REC_BAD_CAP, BGZF_PAYLOAD, BGZF_OVERHEAD, BGZF_SLOT
void bz_consts(uint64_t *out) {
  const uint64_t v[6] = {TOK_STRIDE, (uint64_t)RES_THREADS, REC_BAD_CAP, BGZF_PAYLOAD, BGZF_OVERHEAD, BGZF_SLOT};
  for (int k = 0; k < 6; k++) out[k] = v[k];
}

// out: error, at, claimed, blocks, inflated; blk: in_off, in_len, out_len, out_off, crc of the first `cap` blocks; text: the error's text
void bz_parse(const uint8_t *bgzf, uint64_t n_bytes, uint64_t *out, uint64_t *blk, uint64_t cap, char *text, uint64_t text_cap) {
  const BgzfParse r = bgzf_parse(bgzf, n_bytes);
  out[0] = r.error; out[1] = r.at; out[2] = r.claimed; out[3] = r.blocks.size(); out[4] = r.inflated;
  for (uint64_t k = 0; k < r.blocks.size() && k < cap; k++) {
    const BgzfBlk &b = r.blocks[k];
    const uint64_t v[5] = {b.in_off, b.in_len, b.out_len, b.out_off, b.crc};
    for (int j = 0; j < 5; j++) blk[5 * k + j] = v[j];
  }
  snprintf(text, text_cap, "%s", r.text().c_str());
}

uint64_t bz_cut(const uint32_t *out_len, uint64_t n, uint64_t from, uint64_t limit, uint64_t max_bytes) {
  return bgzf_cut(blocks_of(out_len, n).data(), from, limit, max_bytes);
}

// a device on which the scratch of at most `room` blocks fits.  out: nt, pretended, how often the scratch was asked for
void bz_tok_fit(uint64_t nt, int fail_above, uint64_t room, uint64_t *out) {
  uint64_t asked = 0;
  const BgzfTokFit f = bgzf_tok_fit(nt, fail_above, [&](size_t k) { asked++; return k <= room; });
  out[0] = f.nt; out[1] = f.pretended; out[2] = asked;
}

// out: chunk, first, lane, turns, then q0, q1, side of each turn (at most cap)
void bz_chunks(uint32_t na, int copy_chunk, int first_chunk_div, int n_cu, uint64_t *out, uint64_t cap) {
  const BgzfChunks C(na, copy_chunk, first_chunk_div, n_cu);
  out[0] = C.chunk; out[1] = C.first; out[2] = C.lane; out[3] = C.turns.size();
  for (uint64_t k = 0; k < C.turns.size() && k < cap; k++) { out[4 + 3 * k] = C.turns[k].q0; out[5 + 3 * k] = C.turns[k].q1; out[6 + 3 * k] = C.turns[k].side; }
}

uint32_t bz_common_len(const uint32_t *out_len, uint64_t n) { return bgzf_common_len(blocks_of(out_len, n).data(), n); }

// out: slot 6: entry, exit, res, cnt, base, bad_list, words64; slot 7: ntok, pow_common, elems
void bz_scratch(uint32_t na, uint64_t *out) {
  const BgzfScratch6 A(na);
  const BgzfScratch7 B(na);
  const uint64_t v[10] = {A.entry, A.exit, A.res, A.cnt, A.base, A.bad_list, A.words64, B.ntok, B.pow_common, B.elems};
  for (int k = 0; k < 10; k++) out[k] = v[k];
}

// out: the 32-bit word of bad, max_rec, inflate; the words read back; the bytes cleared per inflate piece and per scan piece; the two bits
void bz_res(uint64_t *out) {
  const uint64_t v[8] = {offsetof(BgzfRes, bad) / 4, offsetof(BgzfRes, max_rec) / 4, offsetof(BgzfRes, inflate) / 4, sizeof(BgzfRes) / 4,
                         BgzfRes::CLEAR_PIECE, BgzfRes::CLEAR_SCAN, INFLATE_BAD_DATA, INFLATE_BAD_CRC};
  for (int k = 0; k < 8; k++) out[k] = v[k];
}

}  // extern "C"
