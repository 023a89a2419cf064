// clean_sam.hip — CleanSam (filters/simple-filters.go:292-306): MAPQ 0 for unmapped reads; an alignment that ends behind its reference
// sequence is soft-clipped there by softClipEndOfRead (filters/utils.go:102-119), whose arithmetic filter_rules.hpp's clean_cigar
// restates as it stands.  The rewritten CIGAR has at most one operation more than the old one, so the CIGAR column is rebuilt (new
// lengths, a scan, a copy pass) - only if a record is affected at all.
#include "common.hpp"
#include "filter_rules.hpp"

namespace elp {

static_assert(RULE_UNMAPPED == F_UNMAPPED && RULE_OP_M == OP_M && RULE_OP_I == OP_I && RULE_OP_D == OP_D && RULE_OP_N == OP_N && RULE_OP_S == OP_S &&
              RULE_OP_EQ == OP_EQ && RULE_OP_X == OP_X, "filter_rules.hpp restates common.hpp's numbers");

struct CleanCols {
  uint64_t n;
  const int32_t *refid, *pos, *ref_len;
  const uint16_t *flag;
  uint8_t *mapq;
  const uint8_t *state;
  const uint64_t *cigar_off;
  const uint32_t *cigar;
  int32_t n_ref;
};
// clean_cigar on record i of the columns (out may be null: count only)
__device__ inline int clean_record(const CleanCols &m, uint64_t i, uint32_t *out, bool *changed) {
  const uint64_t c0 = m.cigar_off[i];
  return clean_cigar(m.cigar + c0, (int)(m.cigar_off[i + 1] - c0), m.flag[i], m.pos[i], clean_length(m.ref_len, m.n_ref, m.refid[i]), out, changed);
}
__global__ __launch_bounds__(256) void k_clean_count(CleanCols m, uint32_t *__restrict__ newcnt, uint32_t *res /* [0] rewritten records, [1] error bits */) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m.n) return;
  uint32_t cnt = (uint32_t)(m.cigar_off[i + 1] - m.cigar_off[i]);
  if (m.state[i] != 2) {  // (records an earlier filter removed never reach CleanSam)
    bool changed;
    const int nn = clean_record(m, i, nullptr, &changed);
    if (nn < 0) atomicOr(&res[1], nn == -1 ? 1u : 2u);
    else cnt = (uint32_t)nn;
    if (changed) atomicAdd(&res[0], 1u);
  }
  newcnt[i] = cnt;
}
__global__ __launch_bounds__(256) void k_clean_write(CleanCols m, const uint32_t *__restrict__ newoff, uint32_t total, uint32_t *__restrict__ cigar_new,
                                                     uint64_t *__restrict__ off_new) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i > m.n) return;
  if (i == m.n) { off_new[i] = total; return; }
  off_new[i] = newoff[i];
  bool changed;
  if (m.state[i] != 2) (void)clean_record(m, i, cigar_new + newoff[i], &changed);
  else {
    const uint64_t c0 = m.cigar_off[i], c1 = m.cigar_off[i + 1];
    for (uint64_t k = c0; k < c1; k++) cigar_new[newoff[i] + (k - c0)] = m.cigar[k];
  }
}
// aln.MAPQ = 0 for unmapped reads - queued once the count pass has shown that no record makes the call fail (a failed call leaves the
// columns as they were: ADVICE r4)
__global__ __launch_bounds__(256) void k_clean_mapq(uint64_t n, const uint16_t *__restrict__ flag, const uint8_t *__restrict__ state, uint8_t *__restrict__ mapq) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && state[i] != 2 && (flag[i] & F_UNMAPPED)) mapq[i] = 0;
}
__global__ __launch_bounds__(256) void k_copy_u64(uint64_t n, const uint64_t *__restrict__ src, uint64_t *__restrict__ dst) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = src[i];
}

}  // namespace elp

using namespace elp;

extern "C" {

int elp_clean_sam(elp_ctx *c, uint64_t *n_clipped_out) {
  if (!c) return ELP_ERR_ARG;
  std::lock_guard<std::mutex> g(c->stage_mu);
  ELP_HIP(c, hipSetDevice(c->device));
  if (!c->have_header) return set_error(c, ELP_ERR_ARG, "elp_clean_sam: call elp_set_header first");
  if (n_clipped_out) *n_clipped_out = 0;
  const uint64_t n = c->n;
  if (!n) return 0;
  if (c->cigar_ops + n >= 0xFFFFFFFFull) return set_error(c, ELP_ERR_UNSUPPORTED, "elp_clean_sam: more than 2^32 CIGAR operations in one context");
  hipStream_t st = c->stream;
  uint32_t *wk;
  ELP_TRY(scratch(c, 4, 2 * (n + 8) + 16, &wk));
  uint32_t *newcnt = wk, *newoff = wk + n + 8, *res = newoff + n + 8;
  ELP_HIP(c, hipMemsetAsync(res, 0, 8, st));
  CleanCols m{n, c->refid.p, c->pos.p, c->ref_len.p, c->flag.p, c->mapq.p, c->has_sr.p, c->cigar_off.p, c->cigar.p, c->n_ref};
  ELP_LAUNCH(c, "clean_count", k_clean_count, dim3(blocks_for(n, 256)), dim3(256), 0, m, newcnt, res);
  uint32_t hr[2] = {0, 0};
  ELP_HIP(c, hipMemcpyAsync(hr, res, 8, hipMemcpyDeviceToHost, st));
  ELP_HIP(c, elp::stream_wait(st));
  // MAPQ changed, CIGARs may: whatever was derived from them is stale
  c->derived.fixed_fields_changed();
  if (hr[1] & 1u) return set_error(c, ELP_ERR_DATA, "Unexpected non-0 relative clipping position in CleanSam. (reference: log.Panic, filters/utils.go:93)");
  if (hr[1] & 2u) return set_error(c, ELP_ERR_UNSUPPORTED, "elp_clean_sam: a clipped CIGAR needs an operation length outside the 28 bits of a BAM CIGAR field");
  ELP_LAUNCH(c, "clean_mapq", k_clean_mapq, dim3(blocks_for(n, 256)), dim3(256), 0, n, (const uint16_t *)c->flag.p, (const uint8_t *)c->has_sr.p, c->mapq.p);
  if (n_clipped_out) *n_clipped_out = hr[0];
  if (!hr[0]) { ELP_HIP(c, elp::stream_wait(st)); return 0; }
  uint32_t total = 0;
  ELP_TRY(exclusive_scan_u32(c, newcnt, newoff, n, &total));
  uint32_t *cig_new;
  uint64_t *off_new;
  ELP_TRY(scratch(c, 5, (size_t)total + 64, &cig_new));
  ELP_TRY(scratch(c, 6, n + 8, &off_new));
  ELP_LAUNCH(c, "clean_write", k_clean_write, dim3(blocks_for(n + 1, 256)), dim3(256), 0, m, (const uint32_t *)newoff, total, cig_new, off_new);
  // the rebuilt column replaces the staged one (the offsets first: the kernel above read the old ones)
  ELP_TRY(ensure(c, c->cigar, (size_t)total + 64));
  ELP_HIP(c, hipMemcpyAsync(c->cigar.p, cig_new, (size_t)total * 4, hipMemcpyDeviceToDevice, st));
  ELP_LAUNCH(c, "clean_offsets", k_copy_u64, dim3(blocks_for(n + 1, 256)), dim3(256), 0, n + 1, (const uint64_t *)off_new, c->cigar_off.p);
  ELP_HIP(c, elp::stream_wait(st));
  c->cigar_ops = total;
  return 0;
}

}  // extern "C"
