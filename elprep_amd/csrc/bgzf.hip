// bgzf.hip — BGZF on the device, the reader's entry point: elp_stage_bgzf stages the records of whole BGZF blocks.
//
// Reference: utils/bgzf/bgzf-files.go.  Every block is a gzip member with the 6-byte "BC" extra field that holds the block's size, a raw
// DEFLATE stream, the CRC-32 of the uncompressed bytes and their number.  The work is in four places:
//   bgzf_plan.hpp     host arithmetic: the member headers parsed, the pieces cut, the chunks scheduled, the scratch laid out
//   bgzf_inflate.hip  bgzf_inflate_piece: the blocks of a piece inflated into c->raw, their CRCs checked
//   bgzf_records.hip  bgzf_scan_piece: where the alignment records start in the inflated bytes
//   bam_in.hip        stage_bam_columns: the records into the columns, as elp_stage_bam does
// The writer is bgzf_out.hip.  This function decides nothing about sizes itself.
#include "bgzf.hpp"

using namespace elp;

// elp_stage_bgzf: see include/elprep_hip.h
extern "C" int elp_stage_bgzf(elp_ctx *c, const uint8_t *bgzf, uint64_t n_bytes, uint64_t first_record, uint16_t split_id) {
  if (!c || (!bgzf && n_bytes)) return ELP_ERR_ARG;
  std::lock_guard<std::mutex> g(c->stage_mu);
  ELP_HIP(c, hipSetDevice(c->device));
  if (!c->have_header) return set_error(c, ELP_ERR_ARG, "elp_stage_bgzf: call elp_set_header first");
  if (c->dict_replaced) return staging_refused_after_replace(c, "elp_stage_bgzf");
  if (c->n_rg && !c->have_rg_ids && !c->replace_rg) return set_error(c, ELP_ERR_ARG, "elp_stage_bgzf: call elp_set_read_group_ids first");
  if (c->n != c->raw_n) return set_error(c, ELP_ERR_ARG, "elp_stage_bgzf: the context already holds records staged with elp_stage");
  const BgzfParse file = bgzf_parse(bgzf, n_bytes);
  if (file.error) return set_error(c, ELP_ERR_DATA, "%s", file.text().c_str());
  const std::vector<BgzfBlk> &blocks = file.blocks;
  const uint64_t inflated = file.inflated;
  if (first_record > inflated) return set_error(c, ELP_ERR_ARG, "elp_stage_bgzf: first_record lies behind the inflated data");
  c->derived.records_changed();
  if (blocks.empty()) return 0;
  // the inflated stream goes to c->raw behind what is there; the records of the header prefix are never referenced
  const uint64_t raw0 = c->raw_bytes;
  ELP_TRY(ensure(c, c->raw, raw0 + inflated + 64, true, raw0));
  const uint64_t PIECE = (uint64_t)c->tune.bgzf_piece, IPIECE = (uint64_t)c->tune.bgzf_inflate_piece;
  uint64_t begin = raw0 + first_record;  // where the next record starts in c->raw
  CopyEvents copied;
  BgzfPiece piece;
  size_t a0 = 0, a1 = 0;  // the inflate piece: blocks [a0, a1)
  for (size_t b0 = 0, b1; b0 < blocks.size(); b0 = b1) {
    if (b0 == a1) {  // the next inflate piece: compressed bytes + block table to the device, every block inflated
      a0 = a1;
      ELP_TRY(bgzf_inflate_piece(c, bgzf, blocks.data() + a0, bgzf_cut(blocks.data(), a0, blocks.size(), IPIECE) - a0, raw0, copied, &piece));
      a1 = a0 + piece.na;
    }
    // the next scan piece, inside the inflate piece: its records found, their columns staged
    b1 = bgzf_cut(blocks.data(), b0, a1, PIECE);
    BgzfScan found;
    ELP_TRY(bgzf_scan_piece(c, piece, b0 - a0, (uint32_t)(b1 - b0), begin, &found));
    if (found.n_rec) ELP_TRY(stage_bam_columns(c, found.n_rec, found.rec_end - begin, found.rec_end, found.max_rec, split_id));
    begin = found.rec_end;
  }
  if (begin != raw0 + inflated) return set_error(c, ELP_ERR_DATA, "elp_stage_bgzf: the data ends inside an alignment record (%llu bytes left over)", (unsigned long long)(raw0 + inflated - begin));
  c->raw_bytes = raw0 + inflated;
  return 0;
}
