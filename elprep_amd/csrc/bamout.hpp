// bamout.hpp — what the emitters of both output formats share: the columns and staged bytes an output record is gathered from (BamOut),
// the tag filter's look-up and the choice of the source context in a stream made of two.  bam_out.hip writes BAM records from them
// (formatBamAlignment), sam.hip SAM lines (FormatAlignment); emit_stream (emit.hip) is the loop around either pair of launches, with the
// sizes of emit_plan.hpp.
#pragma once

#include "common.hpp"
#include "bamtag.hpp"
#include "emit_plan.hpp"

namespace elp {

struct BamOut {
  uint64_t n_out;
  const uint32_t *perm;
  const uint8_t *raw;
  const uint64_t *raw_off;   // per staged record: offset of its BAM record in raw (n + 1)
  const int32_t *refid, *pos, *next_refid, *pnext, *tlen;
  const uint16_t *flag;
  const uint8_t *mapq;
  const uint32_t *l_seq;
  const uint64_t *qname_off, *cigar_off, *qual_off;
  const uint8_t *qname, *qual;
  const uint32_t *cigar;
  const uint32_t *drop;      // elp_set_tag_filter: bit k = fields with the 16-bit key k stay behind (65536 bits); nullptr = no filter
  const uint8_t *rg_new;     // elp_set_replace_read_group: the id every record goes out with (rg_on), rg_len bytes
  uint32_t rg_len, rg_on;
  uint32_t sr_on;            // the split emitters (split.hip): src is their emission list - staging indices, bit 31 = the tagged copy
};
constexpr uint32_t KEY_RG = tag_key_of('R', 'G');
constexpr uint32_t KEY_SR = tag_key_of('s', 'r');
// filters2's RemoveOptionalFields / KeepOptionalFields (filters/simple-filters.go:235-288) as one look-up: every field of a key goes or stays
__device__ __forceinline__ bool tag_dropped(const uint32_t *__restrict__ drop, uint32_t key) { return drop && ((drop[key >> 5] >> (key & 31)) & 1u); }
// Output record k of a MERGED stream (elp_emit_merged_bam) comes from one of two contexts: src[k] = rank of the record in the first
// context's sorted output, or MERGE_SECOND | its rank in the second's.  src == nullptr: one context, output record k = perm[k].
__device__ __forceinline__ const BamOut &out_source(const BamOut &m, const BamOut &m2, const uint32_t *__restrict__ src, uint64_t k, uint32_t *i) {
  if (!src) { *i = m.perm[k]; return m; }
  const uint32_t s = src[k];
  const BamOut &mm = (s & MERGE_SECOND) ? m2 : m;
  *i = mm.perm[s & ~MERGE_SECOND];
  return mm;
}
// The split emitters' list (elp_emit_split_*, split.hip) names records by STAGING index, not by rank in a permutation; bit 31 of an entry
// marks the copy that stays in the group file of a record that also goes to the spread file: it gets aln.TAGS.Set(sr, int64(1))
// (sam/split-merge.go:290).  SR = false is out_source as it is.
constexpr uint32_t SPLIT_TAGGED = 0x80000000u;
template <bool SR>
__device__ __forceinline__ const BamOut &out_source(const BamOut &m, const BamOut &m2, const uint32_t *__restrict__ src, uint64_t k, uint32_t *i, bool *set_sr) {
  if constexpr (SR) {
    const uint32_t s = src[k];
    *i = s & ~SPLIT_TAGGED;
    *set_sr = (s & SPLIT_TAGGED) != 0;
    return m;
  } else {
    *set_sr = false;
    return out_source(m, m2, src, k, i);
  }
}

// Alignment.bin(), sam/bam-files.go:443-468
__device__ inline uint32_t reg2bin(int32_t beg, int32_t end) {
  if (beg >> 14 == end >> 14) return (uint32_t)(((1 << 15) - 1) / 7 + (beg >> 14));
  if (beg >> 17 == end >> 17) return (uint32_t)(((1 << 12) - 1) / 7 + (beg >> 17));
  if (beg >> 20 == end >> 20) return (uint32_t)(((1 << 9) - 1) / 7 + (beg >> 20));
  if (beg >> 23 == end >> 23) return (uint32_t)(((1 << 6) - 1) / 7 + (beg >> 23));
  if (beg >> 26 == end >> 26) return (uint32_t)(((1 << 3) - 1) / 7 + (beg >> 26));
  return 0;
}
// ... of a record with this FLAG whose POS - 1 is beg and whose reference-consuming CIGAR operations add up to ref_span (int32 arithmetic
// that wraps, as the reference's).  The BAM emitter (bam_out.hip) and SAM text in (samin.hip) write the bin field with it.
__device__ inline uint32_t record_bin(uint16_t flag, int32_t beg, uint32_t ref_span) {
  const int32_t end = (flag & F_UNMAPPED) ? beg : (int32_t)((uint32_t)beg + ref_span - 1u);
  return reg2bin(beg, end);
}

// SAM text (sam.hip): the @SQ SN strings of the stream's dictionary (elp_set_reference_names_flat), name of refid r = names[name_off[r] ..
// name_off[r + 1]).  A stream of two contexts has ONE table: both hold equal names (checked, as for the tag filter).
struct SamNames {
  const uint8_t *names;
  const uint32_t *name_off;
  int32_t n_ref;
  uint32_t max_name;  // bytes of the longest name (the host's bound of a pass, emit_stream)
};
// the two passes of a SAM chunk, queued on c->stream under the profile names emit_sam_sizes and emit_sam (sizes, err, offs, out as the
// BAM kernels take them)
int sam_sizes_launch(elp_ctx *c, const BamOut &m, const BamOut &m2, const SamNames &nm, const uint32_t *src, uint64_t k0, uint32_t cnt, uint32_t *sizes, uint32_t *err);
int sam_emit_launch(elp_ctx *c, const BamOut &m, const BamOut &m2, const SamNames &nm, const uint32_t *src, uint64_t k0, uint32_t cnt, const uint32_t *offs, uint8_t *out);
// the same two of a BAM chunk (bam_out.hip), under emit_bam_sizes and emit_bam - the split emitters' instantiations (m.sr_on) of either
// pair under emit_split_*
int bam_sizes_launch(elp_ctx *c, const BamOut &m, const BamOut &m2, const uint32_t *src, uint64_t k0, uint32_t cnt, uint32_t *sizes, uint32_t *err);
int bam_emit_launch(elp_ctx *c, const BamOut &m, const BamOut &m2, const uint32_t *src, uint64_t k0, uint32_t cnt, const uint32_t *offs, uint8_t *out);

// emit.hip, for the emitters of other files (split.hip): the chunked size / scan / gather loop over n_out output records in the format
// fmt (OutFormat, emit_plan.hpp), the context's columns as the kernels take them, its reference names and the check that they are set
int emit_stream(elp_ctx *c, const BamOut &m, const BamOut &m2, const uint32_t *src, uint64_t n_out, uint64_t max_raw_rec, uint8_t *out, uint64_t cap,
                uint64_t *n_bytes_out, OutFormat fmt, const SamNames &nm, const char *who);
BamOut bam_out_of(const elp_ctx *c);
SamNames sam_names_of(const elp_ctx *c);
int sam_names_checks(elp_ctx *c, elp_ctx *other, const char *who);
// emit.hip, for the index of a stream (bai.hip): what a replacing read group may add to a staged record, and the merged stream as
// elp_emit_merged_* walks it - its checks, both contexts' columns and the list `src` (scratch slot 6 of `groups`; nullptr for n_out = 0)
uint64_t emit_out_growth(const elp_ctx *c);
int emit_merged_list(elp_ctx *groups, elp_ctx *spread, const char *who, BamOut *mg, BamOut *ms, const uint32_t **src, uint64_t *n_out);

}  // namespace elp
