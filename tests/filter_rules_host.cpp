// filter_rules_host.cpp — elprep_amd/csrc/filter_rules.hpp behind C functions, for tests/test_filter_rules_cpu.py: the host build of
// the per-record rules that the kernels of filter.hip, clean_sam.hip, split_merge.hip and split.hip run, and of the scratch layouts of
// their entry points.  Built by the host compiler alone.
#include "../elprep_amd/csrc/filter_rules.hpp"

#include <vector>

using namespace elp;

namespace {
struct Switches {  // the six switches of elp_predicates
  int remove_unmapped, remove_unmapped_strict, min_mapq, remove_non_exact, remove_duplicates, use_regions;
};
}  // namespace

extern "C" {

int fr_overlap(const int32_t *iv, int64_t n, int32_t start, int32_t end) { return overlap(iv, n, start, end); }

void fr_cigar_facts(const uint32_t *ops, uint64_t nop, int32_t *out /* ref_len, read_len, exact */) {
  const CigarFacts c = cigar_facts(ops, nop);
  out[0] = c.ref_len; out[1] = c.read_len; out[2] = c.exact;
}

// sw: remove_unmapped, remove_unmapped_strict, min_mapq, remove_non_exact, remove_duplicates, use_regions; the regions as
// elp_filter_records_flat takes them: region_off[r] .. region_off[r + 1] = the rows of refid r in `regions`.  fetched[0] / [1] count the
// calls of the MAPQ and CIGAR fetchers
int fr_record_rejected(const int *sw, uint16_t flag, int32_t refid, int32_t pos, uint8_t mapq, const uint32_t *ops, uint64_t nop, int32_t n_ref,
                       int32_t *regions, const int64_t *region_off, int *fetched) {
  const Switches p{sw[0], sw[1], sw[2], sw[3], sw[4], sw[5]};
  std::vector<int32_t *> ptr((size_t)n_ref + 1, nullptr);
  std::vector<int64_t> cnt((size_t)n_ref + 1, 0);
  for (int32_t r = 0; r < n_ref && regions; r++) {
    ptr[r] = regions + 2 * region_off[r];
    cnt[r] = region_off[r + 1] - region_off[r];
  }
  return record_rejected(
      p, flag, refid, pos, [&] { fetched[0]++; return mapq; }, [&] { fetched[1]++; return cigar_facts(ops, nop); }, n_ref, ptr.data(), cnt.data());
}

int32_t fr_clean_length(const int32_t *ref_len, int32_t n_ref, int32_t r) { return clean_length(ref_len, n_ref, r); }
int fr_clean_cigar(const uint32_t *ops, int nop, uint16_t flag, int32_t pos, int32_t length, uint32_t *out, int *changed) {
  bool ch = false;
  const int n = clean_cigar(ops, nop, flag, pos, length, out, &ch);
  *changed = ch;
  return n;
}

// a record with its block_size field in front, as k_filter_exact_strict reads it; -> STRICT_KEEP / _REJECT / _PANICS
int fr_strict(const uint8_t *p) {
  const uint8_t *rec = p + 4, *end = rec + ld_u32(p);
  return strict_decide(strict_walk(bam_fields_at(rec), end));
}

int fr_split_route(int32_t r, int32_t nr, const int32_t *group_of_ref, int32_t n_ref, int32_t *g) { return split_route(r, nr, group_of_ref, n_ref, g); }
uint64_t fr_merge_key(int32_t refid, int32_t pos) { return merge_key(refid, pos); }
uint64_t fr_merge_upper_bound(const uint64_t *kg, uint64_t ng, uint64_t key) { return merge_upper_bound(kg, ng, key); }

void fr_region_layout(uint64_t total, int32_t n_ref, uint64_t *out /* pool, ptr, cnt, bytes */) {
  const RegionLayout L((size_t)total, n_ref);
  out[0] = L.pool; out[1] = L.ptr; out[2] = L.cnt; out[3] = L.bytes;
}
void fr_classify_layout(uint64_t n, int32_t n_ref, int32_t n_groups, uint64_t *out /* gof, counts, split, spread, bytes, n_counts */) {
  const ClassifyLayout L(n, n_ref, n_groups);
  out[0] = L.gof; out[1] = L.counts; out[2] = L.split; out[3] = L.spread; out[4] = L.bytes; out[5] = L.n_counts;
}
void fr_dictionary_layout(int32_t n_old, uint64_t *out /* counters, map, bytes */) {
  const DictionaryLayout L(n_old);
  out[0] = L.counters; out[1] = L.map; out[2] = L.bytes;
}
void fr_grids(uint64_t n, int n_cu, unsigned *out /* clear flag, dictionary, classify */) {
  out[0] = clear_flag_grid(n, n_cu);
  out[1] = DictionaryLayout::grid(n, n_cu);
  out[2] = n ? ClassifyLayout::grid(n) : 0;
}

}  // extern "C"
