// emit_plan.hpp — the plan of the emitters and of elp_stage_bam as plain host arithmetic: the bound on an output record, the records of
// a device pass, what a pass frames into BGZF members and what it carries into the next, the size query's term, the capacity test, the
// layout of the loop's scratch slot, the tag filter's table, and the cut of a run of BAM records into pieces.  Nothing here touches the
// device or includes HIP: the header compiles with the host compiler alone (tests/emit_plan_host.cpp, tests/test_emit_plan_cpu.py, and
// tests/emit_plan_asan.cpp runs the cut and the pass functions under the sanitizers).  emit.hip and bam_in.hip take their sizes from
// here and compute none themselves.
#pragma once
#include <utility>

#include "bgzf_plan.hpp"

namespace elp {

// the format of an output stream: BAM records as they are; BGZF: the same as BGZF members (bgzf_out.hip), framed on the device pass by
// pass; SAM: lines (sam.hip)
enum class OutFormat { BAM, BGZF, SAM };

// ---- the scratch slots of the output side.  Who owns a slot of elp_ctx::scratch:
//   slot 4  sizes | offs | err            emit_stream, one pass: from the size launch to the emit launch's end (EmitScratch4)
//   slot 5  the pass: carried bytes | the records or lines of the pass      emit_stream: from the carry's upload to the copy to the host
//           (BAM, SAM) or to the end of the framing and the read-back of the next carry (BGZF)
//   slot 7  the framed members of the pass            emit_stream (BGZF): from bgzf_frame / bgzf_deflate to the copy to the host
//   slots 0, 1  bgzf_deflate (bgzf_out.hip), inside one call: the workgroups' tables | the members' sizes | their offsets (0) and the
//           compressed members BGZF_SLOT bytes apart (1), from k_bgzf_deflate until k_bgzf_compact has moved them into slot 7
//   slot 6  src | is_spread | before (emit_merged), src | g0 (emit_concat): from the merge kernels to the last pass of emit_stream,
//           which reads src in every pass
//   slots 2, 3, 6  split.hip: the emission list (2), its keys (3), the files' bounds and the group table (6): from split_list to the
//           last file's last pass - emit_stream reads slot 2 in every pass and touches none of the three
// emit_stream waits for the stream at the end of every pass, so a slot's next request (which may move it) meets no kernel in flight.
// The input side takes slots 4 to 7 at other times (stage_bam_columns: 4; elp_stage_bgzf: 5, 6, 7, bgzf_plan.hpp).
//
// Slot 4 of a pass of cnt records in 32-bit words: sizes, cnt + 8, at 0 | offs, cnt + 8 | err, 1 word; the request leaves 7 words behind err.
struct EmitScratch4 {
  size_t sizes, offs, err;  // 32-bit words from the slot's start
  size_t words;             // the request
  explicit EmitScratch4(uint32_t cnt) : sizes(0), offs((size_t)cnt + 8), err(2 * ((size_t)cnt + 8)), words(2 * ((size_t)cnt + 8) + 8) {}
};
constexpr size_t EMIT_SLOT_PAD = 64;  // bytes requested behind the pass (slot 5) and behind its framed members (slot 7)

// ---- the bound on an output record, in bytes.  BAM and BGZF: an output record is never longer than the staged one (integer fields only
// shrink when re-encoded) - except that elp_clean_sam may have added ONE CIGAR operation (4 bytes), and elp_set_replace_read_group may
// have made the record's RG field longer or added one (RG:Z:<id> = 4 + id_len bytes; the caller adds that to max_raw_rec), and a split
// file's tagged copy may get an sr field (4 bytes; the caller adds them) - so the largest staged record + 4 bounds it.  A tag filter
// only takes bytes away.
//   SAM text can be LONGER than the staged record, so its passes have a bound of their own:
// 5 x staged record + both reference names + 64.  Part by part, text against staged bytes (block_size field included):
//   fixed fields  FLAG 5, POS 11, MAPQ 3, PNEXT 11, TLEN 11, a "*" CIGAR 1, ten tabs and the newline 11 = 53 <= 64, beside 36 staged bytes
//   QNAME         l_name - 1 for l_name;  RNAME and RNEXT: the two names (or one byte each)
//   CIGAR         at most 9 digits + the operation = 10 for 4 (the one operation elp_clean_sam may add: 10, inside 5 x 36 - 64 = 116 spare)
//   SEQ + QUAL    2 l_seq for (l_seq + 1) / 2 + l_seq
//   a field       6 ("\tXX:T:") + value for 3 + value: A 7 for 4; c "-128" 10 for 4; s 12 for 5; i "-2147483648" 17 for 7; f 6 + 15 for 7;
//                 Z 6 + n for 4 + n; B 7 + elements for 8 + elements, an element with its comma: c "-128," 5 for 1 (the worst ratio
//                 of all), s 7 for 2, i 12 for 4, f 16 for 4
//   RG replaced   "\tRG:Z:<id>" = 6 + id_len: the caller's max_raw_rec holds 4 + id_len for it, five times that is more
inline uint64_t emit_rec_bound(OutFormat fmt, uint64_t max_raw_rec, uint32_t max_name) {
  return fmt == OutFormat::SAM ? 5 * max_raw_rec + 2 * (uint64_t)max_name + 64 : std::max<uint64_t>(max_raw_rec, 64) + 4;
}

// records per device pass: sizes and offsets of a pass are scanned in 32 bits, so a pass must stay below 4 GiB of output - below
// 0xFC000000 bytes: BGZF framing adds 31 bytes per 65280 (< 0.1 %) and a pass holds less than a member of carried bytes, the bound
// leaves 1/64 of headroom for both.  At most 2^21 records, at least one; tune_emit_pass > 0 (the tuning key "emit_pass": tests, several
// passes on small inputs) lowers it further.
constexpr uint64_t EMIT_PASS_BYTES = 0xFC000000ull;
constexpr uint32_t EMIT_PASS_RECORDS = 1u << 21;
inline uint32_t emit_pass_records(uint64_t rec_bound, int tune_emit_pass) {
  uint32_t n = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(EMIT_PASS_RECORDS, EMIT_PASS_BYTES / rec_bound));
  if (tune_emit_pass > 0) n = std::min<uint32_t>(n, (uint32_t)tune_emit_pass);
  return n;
}

// ---- one pass of a real call (out != NULL): `held` bytes carried in from the pass before, chunk_bytes of records written behind them.
// BGZF: every member but the stream's last holds BGZF_PAYLOAD bytes of it, wherever the passes fall - the bytes of a pass behind its
// last full member are carried into the next pass and framed there; the last pass frames all it holds.  So held < BGZF_PAYLOAD always
// (a carry is a remainder of that division; the first pass holds nothing).  A pass that frames nothing sends nothing.
// BAM and SAM: nothing is held or carried, the pass goes out as it is.
// out_bound: the bytes the pass may add to the output, what the capacity test asks room for - exact for BAM and SAM, the stored form of
// the pass's members for BGZF (compressed they are never larger).
struct EmitPass {
  uint64_t pass_bytes;   // held + chunk_bytes: what slot 5 holds
  uint64_t frame_bytes;  // its front part that goes out in this pass (BGZF: as members)
  uint64_t carry_bytes;  // the rest, carried into the next pass
  uint64_t out_bound;
  size_t slot5_bytes() const { return (size_t)pass_bytes + EMIT_SLOT_PAD; }
  size_t slot7_bytes() const { return (size_t)out_bound + EMIT_SLOT_PAD; }
};
inline EmitPass emit_pass(OutFormat fmt, uint64_t held, uint64_t chunk_bytes, bool last) {
  const uint64_t pass_bytes = held + chunk_bytes;
  if (fmt != OutFormat::BGZF) return EmitPass{pass_bytes, pass_bytes, 0, chunk_bytes};
  const uint64_t frame_bytes = last ? pass_bytes : pass_bytes / BGZF_PAYLOAD * BGZF_PAYLOAD;
  return EmitPass{pass_bytes, frame_bytes, pass_bytes - frame_bytes, frame_bytes ? bgzf_framed_size(frame_bytes) : 0};
}

// a size query's (out == NULL) term for a pass.  BGZF: the stored form of the pass framed ON ITS OWN, an upper bound: a query carries
// nothing, so every pass counts a short last member that a real call mostly does not write - the answer is looser than the framed
// result, never below it (ceil(a / P) + ceil(b / P) >= ceil((a + b) / P)).  BAM and SAM: exact.
inline uint64_t emit_query_bytes(OutFormat fmt, uint64_t chunk_bytes) { return fmt == OutFormat::BGZF ? bgzf_framed_size(chunk_bytes) : chunk_bytes; }

// the capacity test: the pass may run if its bound fits behind the `total` bytes written so far
inline bool emit_fits(uint64_t total, uint64_t out_bound, uint64_t cap) { return total + out_bound <= cap; }

// ---- elp_set_tag_filter's table.  RemoveOptionalFields / KeepOptionalFields (filters/simple-filters.go:235-288) in filters2's order -
// remove, then keep (cmd/filter.go:878-902) - folded into ONE table of 65536 bits: bit k set = a field whose two key bytes read as the
// number k (first byte low) does not go out.  SmallMap.DeleteIf drops every entry that matches (utils/small-map.go:89-99), so the key
// alone decides.  n_remove = -1: remove all; n_keep = -1: no keep list given (0: keep nothing); (0, -1): no filter, no table.
constexpr size_t TAG_TABLE_WORDS = 65536 / 32;
struct TagDropTable {
  bool filter;                  // false: (0, -1), `words` is empty
  std::vector<uint32_t> words;  // TAG_TABLE_WORDS
};
inline TagDropTable tag_drop_table(const uint8_t *remove_keys, int n_remove, const uint8_t *keep_keys, int n_keep) {
  if (n_remove == 0 && n_keep == -1) return TagDropTable{false, {}};
  std::vector<uint32_t> drop(TAG_TABLE_WORDS, n_remove == -1 ? 0xFFFFFFFFu : 0u);
  for (int k = 0; k < n_remove; k++) {
    const uint32_t key = (uint32_t)remove_keys[2 * k] | ((uint32_t)remove_keys[2 * k + 1] << 8);
    drop[key >> 5] |= 1u << (key & 31);
  }
  if (n_keep >= 0) {
    std::vector<uint32_t> keep(TAG_TABLE_WORDS, 0u);
    for (int k = 0; k < n_keep; k++) {
      const uint32_t key = (uint32_t)keep_keys[2 * k] | ((uint32_t)keep_keys[2 * k + 1] << 8);
      keep[key >> 5] |= 1u << (key & 31);
    }
    for (size_t w = 0; w < drop.size(); w++) drop[w] |= ~keep[w];
  }
  return TagDropTable{true, std::move(drop)};
}

// ---- elp_stage_bam's pieces: the device work unit is a run of whole records that START within BAM_PIECE_BYTES of the piece's first
// byte (u32 scans, bounded scratch).  The first record of a piece is always taken, whatever its length, and the last one may reach
// behind the limit: a piece is at most the limit + one record - 1 byte long, and a record of 256 MiB or more is tolerated in either
// form (kept as it always was: a BAM record that long has not been met).
// bam_cut_piece finds the record starts of the piece that begins at byte at_byte (= record at_rec), from bytes nobody vouches for:
//   rec_off given   the caller's offsets (n_records + 1; the caller has checked rec_off[0] == 0 and rec_off[n_records] == n_bytes):
//                   every record taken must be 36 bytes at least and end inside the bytes; `bytes` is not read
//   rec_off NULL    a walk along the block_size chain (a dependent load per record: the one serial part, ~100 ns per record when the
//                   bytes are cold): every block_size must be 32 at least and its record end inside the bytes
// It reads nothing outside [bytes, bytes + n_bytes) and rec_off[0 .. n_records].
constexpr uint64_t BAM_PIECE_BYTES = 256ull << 20;
enum BamCutError { BAM_CUT_OK = 0, BAM_CUT_BAD_OFFSETS, BAM_CUT_TRUNCATED, BAM_CUT_BAD_BLOCK_SIZE };
struct BamCut {
  BamCutError error = BAM_CUT_OK;
  uint64_t at = 0;          // BAD_OFFSETS: the record; TRUNCATED, BAD_BLOCK_SIZE: the byte of the block_size field
  uint32_t block_size = 0;  // BAD_BLOCK_SIZE: the value read
  std::vector<uint64_t> off;  // the records' starts from at_byte on, and the piece's length: records + 1 entries
  uint64_t end = 0;           // the first byte behind the piece
  uint64_t next_rec = 0;      // the first record behind it (rec_off form)
  uint64_t max_raw_rec = 0;   // the piece's longest record, block_size field included
  // the text elp_stage_bam reports (status ELP_ERR_DATA)
  std::string text() const {
    char buf[160] = "";
    if (error == BAM_CUT_BAD_OFFSETS) snprintf(buf, sizeof buf, "elp_stage_bam: bad record offsets at record %llu", (unsigned long long)at);
    if (error == BAM_CUT_TRUNCATED) snprintf(buf, sizeof buf, "elp_stage_bam: truncated record at byte %llu", (unsigned long long)at);
    if (error == BAM_CUT_BAD_BLOCK_SIZE) snprintf(buf, sizeof buf, "elp_stage_bam: bad block_size %u at byte %llu", block_size, (unsigned long long)at);
    return buf;
  }
};
inline BamCut bam_cut_piece(const uint8_t *bytes, uint64_t n_bytes, const uint64_t *rec_off, uint64_t n_records, uint64_t at_byte, uint64_t at_rec,
                            uint64_t piece_limit = BAM_PIECE_BYTES) {
  BamCut r;
  auto fail = [&r](BamCutError e, uint64_t at, uint32_t block_size = 0) -> BamCut & {
    r.error = e;
    r.at = at;
    r.block_size = block_size;
    return r;
  };
  uint64_t p = at_byte;
  if (rec_off) {
    while (at_rec < n_records && rec_off[at_rec] - at_byte < piece_limit) {
      const uint64_t o = rec_off[at_rec], e = rec_off[at_rec + 1];
      if (e < o + 36 || e > n_bytes) return fail(BAM_CUT_BAD_OFFSETS, at_rec);
      r.off.push_back(o - at_byte);
      at_rec++;
    }
    p = rec_off[at_rec];
  } else {
    while (p < n_bytes && p - at_byte < piece_limit) {
      if (p + 4 > n_bytes) return fail(BAM_CUT_TRUNCATED, p);
      uint32_t bs;
      memcpy(&bs, bytes + p, 4);
      if (bs < 32 || p + 4 + bs > n_bytes) return fail(BAM_CUT_BAD_BLOCK_SIZE, p, bs);
      r.off.push_back(p - at_byte);
      p += 4ull + bs;
    }
  }
  const size_t n_rec = r.off.size();
  r.off.push_back(p - at_byte);
  for (size_t k = 0; k < n_rec; k++) r.max_raw_rec = std::max<uint64_t>(r.max_raw_rec, r.off[k + 1] - r.off[k]);
  r.end = p;
  r.next_rec = at_rec;
  return r;
}

}  // namespace elp
