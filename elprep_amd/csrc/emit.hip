// emit.hip — the way out of the device, whatever the format: emit_stream, the pass loop every output stream runs through (sorted,
// merged, concat here, the split files from split.hip; as BAM records, BGZF members or SAM lines), the entry points of the sorted,
// merged and concat streams with the merge's kernels, and the two settings that only the emitters' walks over the optional fields read
// (elp_set_tag_filter, elp_set_replace_read_group).  The kernels that write a record are bam_out.hip's and sam.hip's, the framing is
// bgzf_out.hip's; every size the loop works with comes from emit_plan.hpp, where the scratch slots' owners are listed too.
#include "common.hpp"
#include "bamout.hpp"

namespace elp {

static_assert(TAG_TABLE_WORDS == elp_ctx::TAG_WORDS, "tag_drop_table fills the context's table");

// the chunked size / scan / gather loop of every emit call; src (device, n_out entries) or nullptr
// fmt: the format of the stream (emit_plan.hpp); SAM reads the names `nm`, which the other formats do not.  who: the entry point, for
// error messages.  max_raw_rec: the largest staged record + what the caller's settings may add to one (emit_rec_bound).
// (declared in bamout.hpp: split.hip runs it once per split file, on that file's slice of its list - m.sr_on)
int emit_stream(elp_ctx *c, const BamOut &m, const BamOut &m2, const uint32_t *src, uint64_t n_out, uint64_t max_raw_rec, uint8_t *out, uint64_t cap,
                uint64_t *n_bytes_out, OutFormat fmt, const SamNames &nm, const char *who) {
  const bool bgzf = fmt == OutFormat::BGZF, sam = fmt == OutFormat::SAM;
  const uint32_t CHUNK = emit_pass_records(emit_rec_bound(fmt, max_raw_rec, nm.max_name), c->tune.emit_pass);
  uint64_t total = 0;
  hipStream_t st = c->stream;
  std::vector<uint8_t> carry, next_carry;  // BGZF: the bytes behind a pass's last full member, framed by the next pass (emit_pass)
  for (uint64_t k0 = 0; k0 < n_out; k0 += CHUNK) {
    const uint32_t cnt = (uint32_t)std::min<uint64_t>(CHUNK, n_out - k0);
    const EmitScratch4 lay(cnt);
    uint32_t *wk;
    ELP_TRY(scratch(c, 4, lay.words, &wk));
    uint32_t *sizes = wk + lay.sizes, *offs = wk + lay.offs, *err = wk + lay.err;
    ELP_HIP(c, hipMemsetAsync(err, 0, 4, st));
    if (sam) ELP_TRY(sam_sizes_launch(c, m, m2, nm, src, k0, cnt, sizes, err));
    else ELP_TRY(bam_sizes_launch(c, m, m2, src, k0, cnt, sizes, err));
    uint32_t chunk_bytes = 0;
    ELP_TRY(exclusive_scan_u32(c, sizes, offs, cnt, &chunk_bytes));
    uint32_t he = 0;
    ELP_HIP(c, hipMemcpyAsync(&he, err, 4, hipMemcpyDeviceToHost, st));
    ELP_HIP(c, elp::stream_wait(st));
    if (he & 16u) return set_error(c, ELP_ERR_UNSUPPORTED, "%s: H-typed optional field", who);
    if (he & 32u) return set_error(c, ELP_ERR_DATA, "%s: a record's refid or next_refid is outside the dictionary", who);
    if (he) return set_error(c, ELP_ERR_DATA, "%s: malformed optional fields", who);
    if (!out) { total += emit_query_bytes(fmt, chunk_bytes); continue; }  // size query
    const EmitPass pass = emit_pass(fmt, carry.size(), chunk_bytes, k0 + cnt >= n_out);
    // (BGZF: out_bound is the size of the stored form - what the pass needs room for; the compressed members are never larger, their
    // actual size is known behind the device pass)
    if (!emit_fits(total, pass.out_bound, cap))
      return set_error(c, ELP_ERR_ARG, "%s: output buffer too small (%llu bytes needed so far)", who, (unsigned long long)(total + pass.out_bound));
    const uint64_t held = carry.size();
    uint8_t *d_out;
    ELP_TRY(scratch(c, 5, pass.slot5_bytes(), &d_out));
    if (held) ELP_HIP(c, hipMemcpyAsync(d_out, carry.data(), held, hipMemcpyHostToDevice, st));
    if (sam) ELP_TRY(sam_emit_launch(c, m, m2, nm, src, k0, cnt, offs, d_out + held));
    else ELP_TRY(bam_emit_launch(c, m, m2, src, k0, cnt, offs, d_out + held));
    const uint8_t *d_send = d_out;
    uint64_t out_bytes = pass.out_bound;
    if (bgzf) {
      uint8_t *d_framed = nullptr;
      if (pass.frame_bytes) {
        ELP_TRY(scratch(c, 7, pass.slot7_bytes(), &d_framed));
        if (c->tune.bgzf_stored) ELP_TRY(bgzf_frame(c, d_out, pass.frame_bytes, d_framed));  // stored DEFLATE blocks (tests, measurements)
        else ELP_TRY(bgzf_deflate(c, d_out, pass.frame_bytes, d_framed, &out_bytes));
      }
      next_carry.resize(pass.carry_bytes);  // (not `carry`: its bytes may still be on their way to the device)
      if (!next_carry.empty()) ELP_HIP(c, hipMemcpyAsync(next_carry.data(), d_out + pass.frame_bytes, next_carry.size(), hipMemcpyDeviceToHost, st));
      d_send = d_framed;
    }
    if (out_bytes) ELP_HIP(c, hipMemcpyAsync(out + total, d_send, out_bytes, hipMemcpyDeviceToHost, st));
    ELP_HIP(c, elp::stream_wait(st));
    carry.swap(next_carry);
    total += out_bytes;
  }
  *n_bytes_out = total;
  return 0;
}
BamOut bam_out_of(const elp_ctx *c) {
  return BamOut{c->n - c->n_sr, c->perm.p, c->raw.p, c->raw_off.p, c->refid.p, c->pos.p, c->next_refid.p, c->pnext.p, c->tlen.p, c->flag.p, c->mapq.p, c->l_seq.p,
                c->qname_off.p, c->cigar_off.p, c->qual_off.p, c->qname.p, c->qual.p, c->cigar.p, c->tag_filter ? c->tag_drop.p : nullptr,
                c->replace_rg_dev.p, c->replace_rg ? (uint32_t)c->replace_rg_id.size() : 0u, c->replace_rg ? 1u : 0u, 0u};
}
SamNames sam_names_of(const elp_ctx *c) { return SamNames{c->ref_names.p, c->ref_names_off.p, c->n_ref, c->max_ref_name}; }
// what the SAM emitters ask beyond their BAM counterparts: the names of the dictionary in force, in a stream of two contexts equal ones
int sam_names_checks(elp_ctx *c, elp_ctx *other, const char *who) {
  if (!c->have_ref_names || (other && !other->have_ref_names))
    return set_error(c, ELP_ERR_ARG, "%s: the reference names are not set (elp_set_reference_names_flat, for the dictionary the context holds now)", who);
  if (other && (c->h_ref_names != other->h_ref_names || c->h_ref_names_off != other->h_ref_names_off))
    return set_error(c, ELP_ERR_ARG, "%s: the two contexts' reference names differ (elp_set_reference_names_flat)", who);
  return 0;
}
}  // namespace elp

using namespace elp;

extern "C" {

// the largest output record is bounded by the largest staged one + this (emit_rec_bound adds the CIGAR operation of elp_clean_sam)
static uint64_t out_growth(const elp_ctx *c) { return c->replace_rg ? 4 + (uint64_t)c->replace_rg_id.size() : 0; }

// the records in the order of the context's permutation (elp_sort_coordinate, elp_sort_queryname or elp_order_keep), without the
// sr-tagged / filtered ones
static int emit_sorted(elp_ctx *c, uint8_t *out, uint64_t cap, uint64_t *n_bytes_out, OutFormat fmt, const char *who) {
  if (!c || !n_bytes_out) return ELP_ERR_ARG;
  ELP_HIP(c, hipSetDevice(c->device));
  if (!c->derived.sorted) return set_error(c, ELP_ERR_ARG, "%s: call elp_sort_coordinate, elp_sort_queryname or elp_order_keep first", who);
  ELP_TRY(radix_check(c));
  if (c->raw_n != c->n) return set_error(c, ELP_ERR_ARG, "%s: records were not staged with elp_stage_bam", who);
  if (fmt == OutFormat::SAM) ELP_TRY(sam_names_checks(c, nullptr, who));
  const BamOut m = bam_out_of(c);
  const SamNames nm = fmt == OutFormat::SAM ? sam_names_of(c) : SamNames{};
  return emit_stream(c, m, m, nullptr, c->n - c->n_sr, c->max_raw_rec + out_growth(c), out, cap, n_bytes_out, fmt, nm, who);
}

// MergeSortedFilesSplitPerChromosome (sam/split-merge.go:410-576) with payloads: the records of `groups` and of `spread` as ONE stream in
// the merge's order - every spread read behind all group reads of its (refid, POS) - gathered in HBM from both contexts' columns and
// inflated records (elp_merge_spread gives the order alone, for a host that merges bytes itself).
__global__ __launch_bounds__(256) void k_merge_mark(uint64_t ns, const uint64_t *__restrict__ slots, uint32_t *__restrict__ is_spread, uint32_t *__restrict__ src) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= ns) return;
  is_spread[slots[j]] = 1u;
  src[slots[j]] = MERGE_SECOND | (uint32_t)j;
}
__global__ __launch_bounds__(256) void k_merge_fill(uint64_t n_out, const uint32_t *__restrict__ is_spread, const uint32_t *__restrict__ before, uint32_t *__restrict__ src) {
  const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s < n_out && !is_spread[s]) src[s] = (uint32_t)s - before[s];  // group reads fill the remaining slots in order
}

// what a stream made of two contexts asks of them (elp_emit_merged_*, elp_emit_concat_*)
static int two_context_checks(elp_ctx *groups, elp_ctx *spread, const char *who) {
  if (groups->raw_n != groups->n || spread->raw_n != spread->n) return set_error(groups, ELP_ERR_ARG, "%s: records were not staged with elp_stage_bam", who);
  // one stream, one filter: the tag filter (and the replacing read group) of `groups`, which `spread` must share
  if (groups->tag_filter != spread->tag_filter || (groups->tag_filter && groups->h_tag_drop != spread->h_tag_drop))
    return set_error(groups, ELP_ERR_ARG, "%s: the two contexts' tag filters differ (elp_set_tag_filter)", who);
  if (!same_replace_rg(groups, spread)) return set_error(groups, ELP_ERR_ARG, "%s: the two contexts' replacing read groups differ (elp_set_replace_read_group)", who);
  if (groups->dict_replaced != spread->dict_replaced)
    return set_error(groups, ELP_ERR_ARG, "%s: one context has replaced its reference dictionary, the other has not (elp_replace_reference_dictionary)", who);
  return 0;
}
// the columns of both contexts as the kernels of a stream of two take them
static void two_columns(elp_ctx *groups, elp_ctx *spread, BamOut *mg, BamOut *ms) {
  *mg = bam_out_of(groups);
  *ms = bam_out_of(spread);
  ms->drop = mg->drop; ms->rg_new = mg->rg_new;  // (equal contents, checked by two_context_checks; both on this device)
}
static int emit_two(elp_ctx *groups, elp_ctx *spread, const uint32_t *src, uint64_t n_out, uint8_t *out, uint64_t cap, uint64_t *n_bytes_out, OutFormat fmt,
                    const char *who) {
  BamOut mg, ms;
  two_columns(groups, spread, &mg, &ms);
  const SamNames nm = fmt == OutFormat::SAM ? sam_names_of(groups) : SamNames{};  // (equal in both contexts: sam_names_checks)
  return emit_stream(groups, mg, ms, src, n_out, std::max(groups->max_raw_rec, spread->max_raw_rec) + out_growth(groups), out, cap, n_bytes_out, fmt, nm, who);
}

// the merged stream's checks and its list: *src_out (scratch slot 6 of `groups`, n_out entries, queued on its stream) names output record
// k as out_source reads it; an empty stream has no list.  The emitters below and the index of their stream (bai.hip) walk the same one.
static int merged_list(elp_ctx *groups, elp_ctx *spread, OutFormat fmt, const char *who, const uint32_t **src_out, uint64_t *n_out_p) {
  if (groups->derived.sorted_qname || spread->derived.sorted_qname) return merge_refuses_queryname(groups, who);
  ELP_TRY(two_context_checks(groups, spread, who));
  if (fmt == OutFormat::SAM) ELP_TRY(sam_names_checks(groups, spread, who));
  uint64_t *slots = nullptr;
  ELP_TRY(merge_spread_slots(groups, spread, &slots));  // checks: both coordinate-sorted or keep-ordered (then: monotonic), one device
  const uint64_t ng = groups->n - groups->n_sr, ns = spread->n - spread->n_sr, n_out = ng + ns;
  if (n_out >= MERGE_SECOND) return set_error(groups, ELP_ERR_UNSUPPORTED, "%s: more than 2^31 output records", who);
  *n_out_p = n_out;
  *src_out = nullptr;
  if (n_out == 0) return 0;
  uint32_t *w;
  ELP_TRY(scratch(groups, 6, 3 * (n_out + 8), &w));
  uint32_t *src = w, *is_spread = w + (n_out + 8), *before = w + 2 * (n_out + 8);
  hipStream_t st = groups->stream;
  ELP_HIP(groups, hipMemsetAsync(is_spread, 0, n_out * 4, st));
  if (ns) ELP_LAUNCH(groups, "merge_mark", k_merge_mark, dim3(blocks_for(ns, 256)), dim3(256), 0, ns, (const uint64_t *)slots, is_spread, src);
  ELP_TRY(exclusive_scan_u32(groups, is_spread, before, n_out, nullptr));
  ELP_LAUNCH(groups, "merge_fill", k_merge_fill, dim3(blocks_for(n_out, 256)), dim3(256), 0, n_out, (const uint32_t *)is_spread, (const uint32_t *)before, src);
  *src_out = src;
  return 0;
}
static int emit_merged(elp_ctx *groups, elp_ctx *spread, uint8_t *out, uint64_t cap, uint64_t *n_bytes_out, OutFormat fmt, const char *who) {
  if (!groups || !spread || groups == spread || !n_bytes_out) return ELP_ERR_ARG;
  const uint32_t *src = nullptr;
  uint64_t n_out = 0;
  ELP_TRY(merged_list(groups, spread, fmt, who, &src, &n_out));
  if (n_out == 0) { *n_bytes_out = 0; return 0; }
  return emit_two(groups, spread, src, n_out, out, cap, n_bytes_out, fmt, who);
}

// MergeUnsortedFilesSplitPerChromosome (sam/split-merge.go:581-619) with payloads: the unmapped file (split id 0 of `groups`), the spread
// file, then the group files in index order, each in its own (input) order
static int emit_concat(elp_ctx *groups, elp_ctx *spread, uint8_t *out, uint64_t cap, uint64_t *n_bytes_out, OutFormat fmt, const char *who) {
  if (!groups || !spread || groups == spread || !n_bytes_out) return ELP_ERR_ARG;
  if (!groups->derived.sorted_keep || !groups->derived.sorted_keep_by_split)
    return set_error(groups, ELP_ERR_ARG, "%s: the groups context must hold a keep permutation ordered by split id (elp_order_keep with by_split = 1)", who);
  if (!spread->derived.sorted_keep || spread->derived.sorted_keep_by_split)
    return set_error(groups, ELP_ERR_ARG, "%s: the spread context must hold a plain keep permutation (elp_order_keep with by_split = 0)", who);
  ELP_TRY(two_context_checks(groups, spread, who));
  if (fmt == OutFormat::SAM) ELP_TRY(sam_names_checks(groups, spread, who));
  if (groups->device != spread->device) return set_error(groups, ELP_ERR_ARG, "%s: contexts on different devices", who);
  ELP_HIP(groups, hipSetDevice(groups->device));
  const uint64_t ng = groups->n - groups->n_sr, ns = spread->n - spread->n_sr, n_out = ng + ns;
  if (n_out >= MERGE_SECOND) return set_error(groups, ELP_ERR_UNSUPPORTED, "%s: more than 2^31 output records", who);
  if (n_out == 0) { *n_bytes_out = 0; return 0; }
  uint32_t *w;
  ELP_TRY(scratch(groups, 6, n_out + 16, &w));
  ELP_HIP(groups, elp::stream_wait(spread->stream));  // (the spread's permutation is complete)
  ELP_TRY(keep_concat_src(groups, ng, ns, w + n_out + 8, w));
  return emit_two(groups, spread, w, n_out, out, cap, n_bytes_out, fmt, who);
}

int elp_emit_sorted_bam(elp_ctx *c, uint8_t *out, uint64_t cap, uint64_t *n_bytes_out) {
  return emit_sorted(c, out, cap, n_bytes_out, OutFormat::BAM, "elp_emit_sorted_bam");
}
// The same records as BGZF blocks (utils/bgzf/bgzf-files.go:324-383): members of at most 65280 input bytes, COMPRESSED on the device
// (bgzf_out.hip: parallel LZ77 + DEFLATE with each block's own dynamic Huffman codes, as compress/flate writes them; `elp_set_tuning`
// "bgzf_fixed" = 1 forces fixed codes, "bgzf_stored" = 1 stored blocks), CRC-32 and ISIZE per member, framed on the device: what follows a
// BAM file's header blocks; the host appends the 28-byte end-of-file block (:53-62).
// Inflating the members gives elp_emit_sorted_bam's bytes.
int elp_emit_sorted_bgzf(elp_ctx *c, uint8_t *out, uint64_t cap, uint64_t *n_bytes_out) {
  return emit_sorted(c, out, cap, n_bytes_out, OutFormat::BGZF, "elp_emit_sorted_bgzf");
}
int elp_emit_merged_bam(elp_ctx *groups, elp_ctx *spread, uint8_t *out, uint64_t cap, uint64_t *n_bytes_out) {
  return emit_merged(groups, spread, out, cap, n_bytes_out, OutFormat::BAM, "elp_emit_merged_bam");
}
// The merged stream as BGZF members, as elp_emit_sorted_bgzf frames the sorted one: `sfm`'s final output leaves the device compressed
int elp_emit_merged_bgzf(elp_ctx *groups, elp_ctx *spread, uint8_t *out, uint64_t cap, uint64_t *n_bytes_out) {
  return emit_merged(groups, spread, out, cap, n_bytes_out, OutFormat::BGZF, "elp_emit_merged_bgzf");
}
int elp_emit_concat_bam(elp_ctx *groups, elp_ctx *spread, uint8_t *out, uint64_t cap, uint64_t *n_bytes_out) {
  return emit_concat(groups, spread, out, cap, n_bytes_out, OutFormat::BAM, "elp_emit_concat_bam");
}
int elp_emit_concat_bgzf(elp_ctx *groups, elp_ctx *spread, uint8_t *out, uint64_t cap, uint64_t *n_bytes_out) {
  return emit_concat(groups, spread, out, cap, n_bytes_out, OutFormat::BGZF, "elp_emit_concat_bgzf");
}

// The same streams as SAM text (sam.hip): FormatAlignment (sam/sam-files.go:563-598) of the records the BAM calls above write, in their
// order, under their checks; no header lines, no framing - a size query (out = NULL) is exact.  The names of the dictionary in force must
// be set (elp_set_reference_names_flat).
int elp_emit_sorted_sam(elp_ctx *c, uint8_t *out, uint64_t cap, uint64_t *n_bytes_out) {
  return emit_sorted(c, out, cap, n_bytes_out, OutFormat::SAM, "elp_emit_sorted_sam");
}
int elp_emit_merged_sam(elp_ctx *groups, elp_ctx *spread, uint8_t *out, uint64_t cap, uint64_t *n_bytes_out) {
  return emit_merged(groups, spread, out, cap, n_bytes_out, OutFormat::SAM, "elp_emit_merged_sam");
}
int elp_emit_concat_sam(elp_ctx *groups, elp_ctx *spread, uint8_t *out, uint64_t cap, uint64_t *n_bytes_out) {
  return emit_concat(groups, spread, out, cap, n_bytes_out, OutFormat::SAM, "elp_emit_concat_sam");
}

// RemoveOptionalFields / KeepOptionalFields as ONE table of 65536 bits, folded on the host (tag_drop_table, emit_plan.hpp)
int elp_set_tag_filter(elp_ctx *c, const uint8_t *remove_keys, int n_remove, const uint8_t *keep_keys, int n_keep) {
  if (!c) return ELP_ERR_ARG;
  if (n_remove < -1 || n_keep < -1 || (n_remove > 0 && !remove_keys) || (n_keep > 0 && !keep_keys)) return set_error(c, ELP_ERR_ARG, "elp_set_tag_filter: bad arguments");
  if (n_remove > 4096 || n_keep > 4096) return set_error(c, ELP_ERR_UNSUPPORTED, "elp_set_tag_filter: more than 4096 keys in a list");
  TagDropTable table = tag_drop_table(remove_keys, n_remove, keep_keys, n_keep);
  if (!table.filter) { c->tag_filter = false; return 0; }
  ELP_HIP(c, hipSetDevice(c->device));
  ELP_TRY(ensure(c, c->tag_drop, elp_ctx::TAG_WORDS));
  ELP_HIP(c, hipMemcpyAsync(c->tag_drop.p, table.words.data(), table.words.size() * 4, hipMemcpyHostToDevice, c->stream));
  ELP_HIP(c, elp::stream_wait(c->stream));
  c->h_tag_drop.swap(table.words);
  c->tag_filter = true;
  return 0;
}

// AddOrReplaceReadGroup (filters/simple-filters.go:156-162): header.RG = []{readGroup}, aln.SetRG(id) on every alignment
int elp_set_replace_read_group(elp_ctx *c, const uint8_t *id, int id_len) {
  if (!c) return ELP_ERR_ARG;
  if (id_len < 0 || id_len > 255 || (id_len && !id) || (id_len && memchr(id, 0, (size_t)id_len)))
    return set_error(c, ELP_ERR_ARG, "elp_set_replace_read_group: the id must be 0 .. 255 bytes without a NUL");
  std::lock_guard<std::mutex> g(c->stage_mu);
  if (!c->have_header || c->n_rg != 1) return set_error(c, ELP_ERR_ARG, "elp_set_replace_read_group: call elp_set_header with a header of ONE read group (the new one) first");
  if (c->n) return set_error(c, ELP_ERR_ARG, "elp_set_replace_read_group: records are staged already (the read group decides their library and covariate)");
  ELP_HIP(c, hipSetDevice(c->device));
  ELP_TRY(ensure(c, c->replace_rg_dev, 256));
  if (id_len) ELP_HIP(c, hipMemcpyAsync(c->replace_rg_dev.p, id, (size_t)id_len, hipMemcpyHostToDevice, c->stream));
  ELP_HIP(c, elp::stream_wait(c->stream));
  c->replace_rg_id.assign(reinterpret_cast<const char *>(id), (size_t)id_len);
  c->replace_rg = true;
  return 0;
}

}  // extern "C"

// for the index of the sorted and the merged stream (bai.hip; declared in bamout.hpp): what their emitters above work from
namespace elp {
uint64_t emit_out_growth(const elp_ctx *c) { return out_growth(c); }
int emit_merged_list(elp_ctx *groups, elp_ctx *spread, const char *who, BamOut *mg, BamOut *ms, const uint32_t **src, uint64_t *n_out) {
  ELP_TRY(merged_list(groups, spread, OutFormat::BGZF, who, src, n_out));
  two_columns(groups, spread, mg, ms);
  return 0;
}
}  // namespace elp
