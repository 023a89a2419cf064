// split.hip — the files of `elprep split`, written on the device: SplitFilePerChromosome (sam/split-merge.go:225-311) and
// SplitSingleEndFilePerChromosome (:664-724) with payloads.  elp_split_classify (split_merge.hip) is the routing rule as three small arrays and
// elp_copy_records / elp_exchange_records (exchange.hip) deliver records to other contexts; here the records of ONE reader context leave as
// the bytes of the split files themselves - BAM records, BGZF members or SAM lines - so that a host writes `elprep split`'s output without
// re-encoding a payload.
//
// What the reference does with every alignment (:280-293): it writes it to the file of its contig group (contigToGroup["*"] is the unmapped
// file); if its mate lies in another group it writes it to the spread file first, sets sr:i:1 in its optional fields and writes THAT to the
// group file.  Single-end input has no spread file and tags nothing (:696-707).
//
// Two steps:
//   (1) the emission list: n + n_spread entries `staging index | tagged << 31`, ordered by file, inside a file by staging index.  One
//       kernel writes a (file id, entry) pair per slot - two slots per record, the second for the copy in the spread file; a slot that
//       holds nothing (no spread copy, a rejected record) gets the key n_files, behind every file - the stable radix pair sort (radix.hip,
//       as keep.hip's by_split order) sorts by the key's one or two bytes, and one thread per file finds its first entry in the sorted keys
//       by binary search (as keep.hip's k_keep_split0_end; up to 65535 files: too many counters for LDS).  The n_files + 1 bounds are the
//       one read-back.
//   (2) emit_stream (emit.hip) once per file on that file's slice of the list, with the emitters' SR instantiation (BamOut.sr_on): bit 31 of
//       an entry makes the walk over the optional fields write SmallMap.Set(sr, int64(1)).  BGZF members, carried bytes and device passes
//       are emit_stream's, per file: nothing crosses a file boundary.
// Scratch: slots 2 (entries), 3 (keys) and 6 (bounds, group table), beside emit_stream's and bgzf_deflate's - who holds which slot from
// when to when: emit_plan.hpp.  Nothing of the context's derived state is read or written (csrc/derived.hpp), not the split-id column and not the permutation.
#include <vector>

#include "common.hpp"
#include "bamout.hpp"
#include "filter_rules.hpp"  // split_route

namespace elp {

constexpr int32_t SPLIT_MAX_GROUPS = 65533;  // n_files = n_groups + 2 and the key behind every file fit 16 bits: two radix passes at most

// slot s = record s >> two | copy s & two (two = 1: paired, two slots per record; 0: single-end, one).  file ids: 0 the unmapped file,
// 1 .. n_groups the group files, n_groups + 1 the spread file (paired only); n_files = no file
__global__ __launch_bounds__(256) void k_split_list_keys(uint64_t n_slots, uint32_t two, const uint8_t *__restrict__ state, const int32_t *__restrict__ refid,
                                                         const int32_t *__restrict__ next_refid, const int32_t *__restrict__ group_of_ref, int32_t n_ref,
                                                         uint32_t n_files, uint64_t *__restrict__ keys, uint32_t *__restrict__ vals) {
  const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_slots) return;
  const uint64_t i = s >> two;
  const bool second = (s & two) != 0;
  uint32_t file = n_files, entry = (uint32_t)i;
  if (state[i] != 2) {  // (a rejected record appears nowhere; a record staged with an sr field, state 1, is routed as any other)
    int32_t g;
    const bool spread = split_route(refid[i], next_refid[i], group_of_ref, n_ref, &g) && two;
    if (!second) {
      file = (uint32_t)g;
      if (spread) entry |= SPLIT_TAGGED;  // the copy that stays in the group file
    } else if (spread) {
      file = n_files - 1;                 // the untagged original
    }
  }
  keys[s] = file;
  vals[s] = entry;
}

// start[f] = the first entry of the sorted keys that is >= f, f = 0 .. n_files: file f's entries are [start[f], start[f + 1])
__global__ __launch_bounds__(256) void k_split_list_bounds(uint64_t n_slots, const uint64_t *__restrict__ keys, uint32_t n_files, uint64_t *__restrict__ start) {
  const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f > n_files) return;
  uint64_t lo = 0, hi = n_slots;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (keys[mid] < f) lo = mid + 1; else hi = mid;
  }
  start[f] = lo;
}

// the list of c's records (device, in scratch slot 2) and its bounds (host, n_files + 1)
static int split_list(elp_ctx *c, const int32_t *group_of_ref, uint32_t n_files, bool paired, const uint32_t **list_out, std::vector<uint64_t> *bounds) {
  const uint64_t n = c->n, n_slots = paired ? 2 * n : n;
  uint64_t *kbuf, *start;
  uint32_t *vbuf;
  ELP_TRY(scratch(c, 3, 2 * n_slots + 8, &kbuf));
  ELP_TRY(scratch(c, 2, 2 * n_slots + 8, &vbuf));
  ELP_TRY(scratch(c, 6, (size_t)n_files + 1 + ((size_t)c->n_ref + 1) / 2 + 2, &start));
  int32_t *d_gof = reinterpret_cast<int32_t *>(start + n_files + 1);
  if (c->n_ref) ELP_HIP(c, hipMemcpyAsync(d_gof, group_of_ref, (size_t)c->n_ref * 4, hipMemcpyHostToDevice, c->stream));
  ELP_LAUNCH(c, "split_list_keys", k_split_list_keys, dim3(blocks_for(n_slots, 256)), dim3(256), 0, n_slots, paired ? 1u : 0u, (const uint8_t *)c->has_sr.p,
             (const int32_t *)c->refid.p, (const int32_t *)c->next_refid.p, (const int32_t *)d_gof, c->n_ref, n_files, kbuf, vbuf);
  uint64_t *ko;
  uint32_t *vo;
  ELP_TRY(radix_sort_pairs_low(c, kbuf, vbuf, kbuf + n_slots, vbuf + n_slots, n_slots, n_files < 256 ? 1 : 2, &ko, &vo));
  c->radix_check_pending = true;
  ELP_LAUNCH(c, "split_list_bounds", k_split_list_bounds, dim3(blocks_for((uint64_t)n_files + 1, 256)), dim3(256), 0, n_slots, (const uint64_t *)ko, n_files, start);
  bounds->resize((size_t)n_files + 1);
  ELP_HIP(c, hipMemcpyAsync(bounds->data(), start, ((size_t)n_files + 1) * 8, hipMemcpyDeviceToHost, c->stream));
  ELP_TRY(radix_check(c));  // (waits for the stream: the bounds are here, and no pass's look-back timed out)
  *list_out = vo;
  return 0;
}

static int emit_split(elp_ctx *c, const int32_t *group_of_ref, int32_t n_groups, int single_end, uint8_t *out, uint64_t cap, uint64_t *file_off_out,
                      uint64_t *n_bytes_out, OutFormat fmt, const char *who) {
  if (!c) return ELP_ERR_ARG;
  if (!group_of_ref || !file_off_out || !n_bytes_out) return set_error(c, ELP_ERR_ARG, "%s: group_of_ref, file_off_out and n_bytes_out must be given", who);
  *n_bytes_out = 0;
  if (n_groups < 1 || n_groups > SPLIT_MAX_GROUPS) return set_error(c, ELP_ERR_ARG, "%s: n_groups must be 1 .. %d", who, SPLIT_MAX_GROUPS);
  for (int32_t r = 0; r < c->n_ref; r++)
    if (group_of_ref[r] < 0 || group_of_ref[r] > n_groups)
      return set_error(c, ELP_ERR_ARG, "%s: group_of_ref[%d] = %d is not a group of 0 .. %d", who, r, group_of_ref[r], n_groups);
  ELP_HIP(c, hipSetDevice(c->device));
  if (c->raw_n != c->n) return set_error(c, ELP_ERR_ARG, "%s: records were not staged with elp_stage_bam (no bytes to write)", who);
  if (c->tag_filter || c->replace_rg)
    return set_error(c, ELP_ERR_ARG, "%s: a tag filter or a replacing read group is set (elp_set_tag_filter, elp_set_replace_read_group): `elprep split` has no such option", who);
  if (fmt == OutFormat::SAM) ELP_TRY(sam_names_checks(c, nullptr, who));
  if (c->n > 0x7FFFFFF0ull) return set_error(c, ELP_ERR_UNSUPPORTED, "%s: more than 2^31-16 staged records (bit 31 of a list entry marks the tagged copy)", who);
  const bool paired = single_end == 0;
  const uint32_t n_files = (uint32_t)n_groups + (paired ? 2u : 1u);
  std::vector<uint64_t> off((size_t)n_files + 1, 0);
  if (c->n) {
    const uint32_t *list = nullptr;
    std::vector<uint64_t> bounds;
    ELP_TRY(split_list(c, group_of_ref, n_files, paired, &list, &bounds));
    BamOut m = bam_out_of(c);
    m.sr_on = 1;
    const SamNames nm = fmt == OutFormat::SAM ? sam_names_of(c) : SamNames{};
    uint64_t total = 0;
    for (uint32_t f = 0; f < n_files; f++) {
      const uint64_t cnt = bounds[f + 1] - bounds[f];
      uint64_t bytes = 0;
      // (a tagged copy is at most 4 bytes longer than its staged record: the sr field it may get; emit_stream bounds its passes by this)
      if (cnt)
        ELP_TRY(emit_stream(c, m, m, list + bounds[f], cnt, c->max_raw_rec + 4, out ? out + total : nullptr, out ? cap - total : 0, &bytes, fmt, nm, who));
      total += bytes;
      off[f + 1] = total;
    }
  }
  for (size_t f = 0; f < off.size(); f++) file_off_out[f] = off[f];
  *n_bytes_out = off.back();
  return 0;
}

}  // namespace elp

using namespace elp;

extern "C" {

int elp_emit_split_bam(elp_ctx *c, const int32_t *group_of_ref, int32_t n_groups, int single_end, uint8_t *out, uint64_t cap, uint64_t *file_off_out,
                       uint64_t *n_bytes_out) {
  return emit_split(c, group_of_ref, n_groups, single_end, out, cap, file_off_out, n_bytes_out, OutFormat::BAM, "elp_emit_split_bam");
}
int elp_emit_split_bgzf(elp_ctx *c, const int32_t *group_of_ref, int32_t n_groups, int single_end, uint8_t *out, uint64_t cap, uint64_t *file_off_out,
                        uint64_t *n_bytes_out) {
  return emit_split(c, group_of_ref, n_groups, single_end, out, cap, file_off_out, n_bytes_out, OutFormat::BGZF, "elp_emit_split_bgzf");
}
int elp_emit_split_sam(elp_ctx *c, const int32_t *group_of_ref, int32_t n_groups, int single_end, uint8_t *out, uint64_t cap, uint64_t *file_off_out,
                       uint64_t *n_bytes_out) {
  return emit_split(c, group_of_ref, n_groups, single_end, out, cap, file_off_out, n_bytes_out, OutFormat::SAM, "elp_emit_split_sam");
}

}  // extern "C"
