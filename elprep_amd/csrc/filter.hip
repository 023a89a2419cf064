// filter.hip — the record-state filters: the per-record predicates next to the hot path, evaluated on the column store.
//
// Fused predicates.  Reference: filters/simple-filters.go — RemoveUnmappedReads :73-75, RemoveUnmappedReadsStrict :79-83,
// RemoveNonExactMappingReads :90-99, RemoveDuplicateReads :136-138, RemoveNonOverlappingReads :310-328 (+ intervals.Overlap,
// intervals/intervals.go:146-160), RemoveMappingQualityLessThan :332-347.  In `elprep filter` they stand in FRONT of AddREFID
// and MarkDuplicates in filters1 (cmd/filter.go:696-803): a read they reject never reaches duplicate marking, the sort, the
// metrics or BQSR.  Here one kernel evaluates the selected predicates for every staged record and marks the rejected ones in the
// record-state column (2 = filtered; 1 = sr-tagged copy, which still takes part in duplicate marking): every later stage skips
// them, the sort puts them behind the output (elp_num_sorted).
// RemoveNonExactMappingReadsStrict :115-134 reads optional fields (X0, X1, XM, XO, XG): a kernel of its own over the staged BAM
// records (elp_filter_exact_strict), same record states.  ClearDuplicateFlag :350-355 (elp_clear_duplicate_flag) rewrites the FLAG
// column in one streaming pass.
// The rules themselves (record_rejected, the strict walk and decision) are filter_rules.hpp's; the other operators that were here
// live in clean_sam.hip, dictionary.hip and split_merge.hip.
#include "common.hpp"
#include "bamtag.hpp"
#include "filter_rules.hpp"

namespace elp {

static_assert(RULE_UNMAPPED == F_UNMAPPED && RULE_DUPLICATE == F_DUPLICATE && RULE_OP_M == OP_M && RULE_OP_I == OP_I && RULE_OP_D == OP_D &&
              RULE_OP_N == OP_N && RULE_OP_S == OP_S && RULE_OP_EQ == OP_EQ && RULE_OP_X == OP_X, "filter_rules.hpp restates common.hpp's numbers");

// the lanes of a wave for which `hit` holds, added to *cnt with one atomic per wave (none if there is no such lane)
__device__ __forceinline__ void count_per_wave(bool hit, unsigned long long *cnt) {
  const unsigned long long b = __ballot(hit);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(cnt, (unsigned long long)__popcll(b));
}

struct FilterCols {
  uint64_t n;
  const int32_t *refid, *pos;
  const uint16_t *flag;
  const uint8_t *mapq;
  const uint64_t *cigar_off;
  const uint32_t *cigar;
  uint8_t *state;  // has_sr column: 0 live, 1 sr-tagged, 2 filtered
  int32_t n_ref;
  int32_t *const *regions;   // per refid: [n][2] Start, End of intervals.FromBed, sorted by Start and flattened
  const int64_t *n_regions;
};

__global__ __launch_bounds__(256) void k_filter_records(FilterCols m, elp_predicates p, unsigned long long *n_dropped /* [0] rejected, [1] rejected tagged copies */) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool drop = false, tagged = false;
  if (i < m.n && m.state[i] != 2) {
    // (the fetchers capture by value: with `m` captured by reference the compiler no longer sees that the intervals lie in global
    // memory and reads them with flat loads)
    drop = record_rejected(
        p, m.flag[i], m.refid[i], m.pos[i], [=] { return m.mapq[i]; },
        [=] {
          const uint64_t c0 = m.cigar_off[i];
          return cigar_facts(m.cigar + c0, m.cigar_off[i + 1] - c0);
        },
        m.n_ref, m.regions, m.n_regions);
    if (drop) {
      tagged = m.state[i] == 1;  // a tagged copy that is rejected was already counted among the records that leave the output
      drop = !tagged;
      m.state[i] = 2;
    }
  }
  count_per_wave(drop, n_dropped);
  count_per_wave(tagged, n_dropped + 1);
}

// ---- RemoveNonExactMappingReadsStrict (filter_rules.hpp: strict_walk, strict_decide).
// One record per lane: a record's optional fields are a chain of dependent loads (every field's size is known only from its type byte
// or its NUL), and 64 chains in flight per wave hide what one chain per wave would wait for; the lanes of a wave read neighbouring
// records, whose tag areas lie a record's length apart.  The kernel writes verdicts only: the record states change in a second pass once
// the call is known not to fail.
struct StrictIn {
  uint64_t n;
  const uint8_t *raw;
  const uint64_t *raw_off;  // per staged record: offset of its block_size field in raw
  const uint8_t *state;
  uint8_t *verdict;         // 0 keep, 1 reject
};
__global__ __launch_bounds__(256) void k_filter_exact_strict(StrictIn m, unsigned long long *cnt /* [0] rejected, [1] rejected tagged copies, [2] panics */) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool drop = false, tagged = false, panics = false;
  if (i < m.n) {
    uint8_t verdict = 0;
    const uint8_t st = m.state[i];
    if (st != 2) {
      const uint8_t *p = m.raw + m.raw_off[i];
      const uint8_t *rec = p + 4, *end = rec + ld_u32(p);
      const int rule = strict_decide(strict_walk(bam_fields_at(rec), end));
      verdict = rule == STRICT_REJECT;
      panics = rule == STRICT_PANICS;
      if (verdict) { tagged = st == 1; drop = !tagged; }
    }
    m.verdict[i] = verdict;
  }
  count_per_wave(drop, cnt);
  count_per_wave(tagged, cnt + 1);
  count_per_wave(panics, cnt + 2);
}
__global__ __launch_bounds__(256) void k_reject_marked(uint64_t n, const uint8_t *__restrict__ verdict, uint8_t *__restrict__ state) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && verdict[i]) state[i] = 2;
}

// ---- ClearDuplicateFlag (filters/simple-filters.go:350-355): FLAG &^= 0x400 on every record; eight flags per 16-byte access
__global__ __launch_bounds__(256) void k_clear_duplicate_flag(uint64_t n, uint16_t *__restrict__ flag) {
  const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (uint64_t)gridDim.x * blockDim.x, nv = n >> 3;
  uint4 *v = reinterpret_cast<uint4 *>(flag);  // (a column starts at an allocation's start: 16-byte aligned)
  constexpr uint32_t KEEP = ~(((uint32_t)F_DUPLICATE << 16) | (uint32_t)F_DUPLICATE);
  for (uint64_t j = gid; j < nv; j += stride) {
    uint4 x = v[j];
    x.x &= KEEP; x.y &= KEEP; x.z &= KEEP; x.w &= KEEP;
    v[j] = x;
  }
  if (gid < (n & 7)) flag[nv * 8 + gid] &= (uint16_t)~F_DUPLICATE;
}

}  // namespace elp

using namespace elp;

extern "C" {

int elp_filter_records(elp_ctx *c, const elp_predicates *p, uint64_t *n_dropped_out) {
  if (!c || !p) return ELP_ERR_ARG;
  ELP_HIP(c, hipSetDevice(c->device));
  if (p->use_regions && (!p->regions || !p->n_regions)) return set_error(c, ELP_ERR_ARG, "elp_filter_records: use_regions without regions");
  const uint64_t n = c->n;
  unsigned long long dropped = 0, dropped_tagged = 0;
  if (n) {
    // target regions -> device (per refid pointer table)
    std::vector<int32_t *> h_ptr((size_t)c->n_ref, nullptr);
    std::vector<int64_t> h_cnt((size_t)c->n_ref, 0);
    int32_t **d_ptr = nullptr;
    int64_t *d_cnt = nullptr;
    if (p->use_regions) {
      size_t total = 0;
      for (int r = 0; r < c->n_ref; r++) total += (size_t)p->n_regions[r];
      const RegionLayout L(total, c->n_ref);
      uint8_t *blk;
      ELP_TRY(scratch(c, 5, L.bytes, &blk));
      int32_t *pool = reinterpret_cast<int32_t *>(blk + L.pool);
      d_ptr = reinterpret_cast<int32_t **>(blk + L.ptr);
      d_cnt = reinterpret_cast<int64_t *>(blk + L.cnt);
      size_t at = 0;
      for (int r = 0; r < c->n_ref; r++) {
        const size_t k = (size_t)p->n_regions[r];
        if (k) ELP_HIP(c, hipMemcpyAsync(pool + 2 * at, p->regions[r], k * 8, hipMemcpyHostToDevice, c->stream));
        h_ptr[r] = pool + 2 * at;
        h_cnt[r] = (int64_t)k;
        at += k;
      }
      if (c->n_ref) {
        ELP_HIP(c, hipMemcpyAsync(d_ptr, h_ptr.data(), (size_t)c->n_ref * sizeof(int32_t *), hipMemcpyHostToDevice, c->stream));
        ELP_HIP(c, hipMemcpyAsync(d_cnt, h_cnt.data(), (size_t)c->n_ref * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
      }
    }
    unsigned long long *cnt;
    ELP_TRY(scratch(c, 6, 4, &cnt));
    ELP_HIP(c, hipMemsetAsync(cnt, 0, 16, c->stream));
    FilterCols m{n, c->refid.p, c->pos.p, c->flag.p, c->mapq.p, c->cigar_off.p, c->cigar.p, c->has_sr.p, c->n_ref, d_ptr, d_cnt};
    ELP_LAUNCH(c, "filter_records", k_filter_records, dim3(blocks_for(n, 256)), dim3(256), 0, m, *p, cnt);
    unsigned long long both[2] = {0, 0};
    ELP_HIP(c, hipMemcpyAsync(both, cnt, 16, hipMemcpyDeviceToHost, c->stream));
    ELP_HIP(c, elp::stream_wait(c->stream));
    dropped = both[0];
    dropped_tagged = both[1];
  }
  commit_rejects(c, dropped, dropped_tagged);
  c->derived.fixed_fields_changed();  // (the has_sr column)
  if (n_dropped_out) *n_dropped_out = dropped;
  return 0;
}

// cgo-friendly form (no pointers to pointers): the regions of all contigs behind each other, region_off[r] .. region_off[r + 1] = the
// [k][2] rows of refid r (n_ref + 1 offsets, in intervals); regions NULL = no target-region test
int elp_filter_records_flat(elp_ctx *c, int remove_unmapped, int remove_unmapped_strict, int min_mapq, int remove_non_exact, int remove_duplicates,
                            const int32_t *regions, const int64_t *region_off, uint64_t *n_rejected_out) {
  if (!c) return ELP_ERR_ARG;
  if (regions && !region_off) return set_error(c, ELP_ERR_ARG, "elp_filter_records_flat: regions without region_off");
  std::vector<const int32_t *> ptr((size_t)c->n_ref + 1, nullptr);
  std::vector<int64_t> cnt((size_t)c->n_ref + 1, 0);
  if (regions)
    for (int r = 0; r < c->n_ref; r++) {
      if (region_off[r + 1] < region_off[r]) return set_error(c, ELP_ERR_ARG, "elp_filter_records_flat: region_off must not decrease");
      ptr[r] = regions + 2 * region_off[r];
      cnt[r] = region_off[r + 1] - region_off[r];
    }
  elp_predicates p;
  p.remove_unmapped = remove_unmapped; p.remove_unmapped_strict = remove_unmapped_strict; p.min_mapq = min_mapq; p.remove_non_exact = remove_non_exact;
  p.remove_duplicates = remove_duplicates; p.use_regions = regions ? 1 : 0; p.regions = ptr.data(); p.n_regions = cnt.data();
  return elp_filter_records(c, &p, n_rejected_out);
}

int elp_filter_exact_strict(elp_ctx *c, uint64_t *n_rejected_out) {
  if (!c) return ELP_ERR_ARG;
  ELP_HIP(c, hipSetDevice(c->device));
  if (c->raw_n != c->n) return set_error(c, ELP_ERR_ARG, "elp_filter_exact_strict: records were not staged with elp_stage_bam / elp_stage_bgzf (column-staged records have no optional fields)");
  if (n_rejected_out) *n_rejected_out = 0;
  const uint64_t n = c->n;
  if (!n) return 0;
  uint8_t *verdict;
  unsigned long long *cnt;
  ELP_TRY(scratch(c, 5, n + 64, &verdict));
  ELP_TRY(scratch(c, 6, 4, &cnt));
  ELP_HIP(c, hipMemsetAsync(cnt, 0, 24, c->stream));
  StrictIn m{n, c->raw.p, c->raw_off.p, c->has_sr.p, verdict};
  ELP_LAUNCH(c, "filter_exact_strict", k_filter_exact_strict, dim3(blocks_for(n, 256)), dim3(256), 0, m, cnt);
  unsigned long long h[3] = {0, 0, 0};
  ELP_HIP(c, hipMemcpyAsync(h, cnt, 24, hipMemcpyDeviceToHost, c->stream));
  ELP_HIP(c, elp::stream_wait(c->stream));
  // (a failed call leaves the record states as they were)
  if (h[2]) return set_error(c, ELP_ERR_DATA, "elp_filter_exact_strict: %llu record(s) hold an X0 / X1 / XM / XO / XG field that is no integer "
                             "(reference: panic on x.(int64), filters/simple-filters.go:117-131)", h[2]);
  if (h[0] + h[1]) {
    ELP_LAUNCH(c, "filter_exact_strict_mark", k_reject_marked, dim3(blocks_for(n, 256)), dim3(256), 0, n, (const uint8_t *)verdict, c->has_sr.p);
    ELP_HIP(c, elp::stream_wait(c->stream));
  }
  commit_rejects(c, h[0], h[1]);
  c->derived.fixed_fields_changed();  // (the has_sr column)
  if (n_rejected_out) *n_rejected_out = h[0];
  return 0;
}

int elp_clear_duplicate_flag(elp_ctx *c) {
  if (!c) return ELP_ERR_ARG;
  ELP_HIP(c, hipSetDevice(c->device));
  if (c->n) {
    ELP_LAUNCH(c, "clear_duplicate_flag", k_clear_duplicate_flag, dim3(clear_flag_grid(c->n, c->n_cu)), dim3(256), 0, c->n, c->flag.p);
    ELP_HIP(c, elp::stream_wait(c->stream));
  }
  c->derived.duplicate_bit_cleared();
  return 0;
}

}  // extern "C"
