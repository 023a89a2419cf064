// bqsr_plan.hpp — the BQSR stage's launch plans as plain host arithmetic: which count kernel takes a read set, in how many passes and
// with how much LDS, and how the gather's scratch block is laid out.  Nothing here touches the device or includes HIP: the header
// compiles with the host compiler alone (tests/plan_host.cpp, tests/test_bqsr_plan_cpu.py).  The kernels' static LDS comes in as an
// argument; each value is a constexpr defined beside its kernel's __shared__ declarations (bqsr_common.hpp lists them).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace elp {

constexpr size_t LDS_CU = 160 * 1024;  // LDS of one CU (gfx950)

// ---- sizes the plans share with the kernels
// the general count kernel's private table (bqsr_count.hip describes the row): context words, extra rows per covariate, words behind the last row
constexpr int CT_CYC = 32, CT_XROWS = 3, CT_PAD = 64;
// the one-length count kernel's (count3.hip)
constexpr int C3_XROWS = 3, C3_PAD = 64;
constexpr int C3_NSEG = 64;       // class-1 record segments without the covariate split; the least with it
constexpr int C3_MAXSEG = 256;
constexpr int C3_CSTRIDE = 64;  // words between two counters: every counter in a 256-byte line of its own (one line = one L2 channel would serialise them all)
// k_bqsr_prologue_fast's workgroups take PF_TILES * 256 consecutive staged records, thread t of a workgroup the records t, t + 256, ...;
// k_c3_seg_hist walks the RGID column in the same workgroups to size the covariate-split segments exactly
constexpr int PF_TILES = 16;
constexpr int CO_MAXCOV = 256;  // covariates the other region's sort handles (a covariate id is a byte: any number of read groups the context accepts)

// ---- the one-length count kernel (count3.hip): one workgroup of 1024 threads per CU around one table; the context cells are replicated
// as often as the CU's LDS allows.  Returns 1 if the tables of this pass do not fit (the caller uses k_bqsr_count).
inline int count3_plan(int n_cov, int n_q, int lmax, size_t static_lds, int *rsw_out, int *rlog_out, size_t *dyn_out, int force_rlog = -1) {
  const int ncw = ((17 * 2 * lmax) >> 4) + 2;
  const size_t rows = (size_t)n_cov * (size_t)(n_q + C3_XROWS);
  for (int rlog = 5; rlog >= 1; rlog--) {
    if (force_rlog >= 0 && force_rlog != rlog) continue;  // elp_set_tuning "count3_rlog": measurements only
    const int rsw = ((16 << rlog) + 16 + ncw + 31) & ~31;
    const size_t dyn = (rows * (size_t)rsw + C3_PAD) * 4;
    if (dyn + static_lds <= LDS_CU && rows * (size_t)rsw * 4 < (1u << 22)) {
      *rsw_out = rsw; *rlog_out = rlog; *dyn_out = dyn;
      return 0;
    }
  }
  return 1;
}

// ---- the gather: what decides the plan besides the number of quality slots
struct GatherShape {
  int n_cov, lmax, max_cycle;      // read-group covariates, longest staged read (>= 1), --max-cycle
  uint32_t uniform_len;            // the one length of the staged reads, 0 = ragged
  int count_kernel, count3_rlog;   // elp_set_tuning
  size_t lds_count3, lds_count, lds_count1024;  // static LDS of k_bqsr_count3, k_bqsr_count<512 threads>, k_bqsr_count<1024 threads>
};

// How the one-length count kernel takes this read set with nq quality slots: 0 not at all (k_bqsr_count), 1 one private table with the rows of
// every covariate, or - if those do not fit, or only with little replication of the context cells - 2: split by covariate (records
// in per-covariate segments, a workgroup counts ONE covariate at a time: the table needs n_q + 3 rows whatever the number of read groups).
// It takes the count if the staged reads have one length, no read can exceed --max-cycle, and the quality slots fit one table pass
// (elp_set_tuning "count_kernel" = 1 forces the general kernel, 2 never splits, 3 always: A/B measurements).
inline int c3_mode(const GatherShape &g, int nq) {
  if (g.count_kernel == 1 || g.uniform_len == 0 || g.lmax > g.max_cycle || g.lmax > 1022) return 0;
  int rsw = 0, rlog = 0;
  size_t dyn = 0;
  const bool all_fits = count3_plan(g.n_cov, nq, g.lmax, g.lds_count3, &rsw, &rlog, &dyn, g.count3_rlog) == 0;
  if (all_fits && (rlog >= 3 || g.n_cov == 1) && g.count_kernel != 3) return 1;
  if (g.n_cov > 1 && g.count_kernel != 2 && count3_plan(1, nq, g.lmax, g.lds_count3, &rsw, &rlog, &dyn, g.count3_rlog) == 0) return 2;
  return all_fits ? 1 : 0;
}

// The general count kernel's plan for nq quality slots.  As many workgroups per CU (512 threads each) as still hold the rows of every
// covariate and quality slot in one pass; else ONE workgroup of 1024 threads per CU around one table (as many waves per SIMD as two of 512)
// and, if that does not hold them either, several passes: over quality subsets and - many read groups - over covariate subsets
// [cov0, cov0 + ncp) (a pass skips the reads of the other covariates).  The reference's tables are maps that just grow
// (filters/bqsr.go:467-551): any number of read groups runs.
struct CountPlan {
  bool fits;      // false: not even one covariate's four rows fit (nothing else is meaningful then)
  int wg_per_cu;  // 3, 2 (512 threads) or 1 (1024 threads: big)
  bool big, mg;   // mg: observation-only cycle cells (half the bytes; mismatches by global atomics)
  int rs;         // words per row of the private table
  int ncp, qcap;  // covariates and quality slots per pass
  long passes;    // ceil(n_cov / ncp) * ceil(nq / qcap)
  size_t dyn(int ncov_pass, int nqs) const { return ((size_t)ncov_pass * (size_t)(nqs + CT_XROWS) * (size_t)rs + CT_PAD) * 4; }
};
inline int count_row_words(int lmax, bool mg) {
  const int cyc = (17 * 2 * lmax) >> 4;
  return (CT_CYC + (mg ? cyc >> 1 : cyc) + 1 + 1) & ~1;
}
inline CountPlan count_general_plan(const GatherShape &g, int nq) {
  CountPlan p{true, 1, false, false, count_row_words(g.lmax, false), g.n_cov, 0, 1};
  const size_t per_slot = (size_t)g.n_cov * (size_t)p.rs * 4;
  for (int w = 3; w >= 2; w--) {
    const size_t budget = LDS_CU / (size_t)w;
    if (budget <= g.lds_count + 256) continue;
    const int cap = (int)((budget - g.lds_count - 256) / per_slot) - CT_XROWS;  // minus the extra rows per covariate
    if (cap >= nq) { p.wg_per_cu = w; p.qcap = cap; return p; }
  }
  p.big = true;
  // rows of `rsx` words that fit -> the (covariates, quality slots) per pass with the fewest passes; 0 = not even one covariate's four rows fit
  auto split = [&](int rsx, int *ncp_out, int *qcap_out) -> long {
    const long rows_fit = (long)((LDS_CU - g.lds_count1024 - 256) / ((size_t)rsx * 4));
    long best = 0;
    for (int k = g.n_cov; k >= 1; k--) {
      const long qc = std::min<long>((long)nq, rows_fit / k - CT_XROWS);
      if (qc < 1) continue;
      const long passes = (long)((g.n_cov + k - 1) / k) * (((long)nq + qc - 1) / qc);
      if (!best || passes < best) { best = passes; *ncp_out = k; *qcap_out = (int)qc; }
    }
    return best;
  };
  p.passes = split(p.rs, &p.ncp, &p.qcap);
  // still several passes: observation-only cycle cells
  if (p.passes != 1) {
    const int rs_mg = count_row_words(g.lmax, true);
    int ncp_mg = 0, qcap_mg = 0;
    const long passes_mg = split(rs_mg, &ncp_mg, &qcap_mg);
    if (passes_mg && (!p.passes || passes_mg < p.passes)) { p.mg = true; p.rs = rs_mg; p.ncp = ncp_mg; p.qcap = qcap_mg; p.passes = passes_mg; }
  }
  p.fits = p.qcap >= 1;
  return p;
}

// ---- the gather's scratch.  One block of 32-bit words (scratch slot 5) holds, in this order:
//   [0] records left to the general prologue, [1] reads of the second prologue pass (the two counts; words 2, 3 unused)
//   queue     [4 .. 4 + n)            the records left to the general prologue kernel
//   plist     [n + 20 .. 2 n + 20)    the reads of the second (plain) pass
//   rec_cnt   64-word aligned, (C3_MAXSEG + 1) counters C3_CSTRIDE words apart: records per class-1 segment, then of the other region (RecOut)
//   cw        [CO_MAXCOV] counts | [CO_MAXCOV + 1] offsets | [CO_MAXCOV] cursors: the other region's sort by covariate
//   seg_cap   [C3_MAXSEG] the covariate-split segments' sizes
//   seg_base  [C3_MAXSEG + 1] the segments' first slots
// and the record area (scratch slot 4, 32-byte records): class-1 segments | the other region | (mode 2) the other region sorted by covariate.
struct GatherScratch {
  uint64_t n;                                           // staged records
  size_t queue, plist, rec_cnt, cw, seg_cap, seg_base;  // word offsets in the block
  size_t words;                                         // the block's size
  unsigned pf_grid;                                     // workgroups of the first prologue pass
  uint64_t cap_s1;  // a class-1 segment's capacity without the covariate split: a wave of the first pass appends its class-1 records (at most PF_TILES * 64) to segment wave % C3_NSEG
  explicit GatherScratch(uint64_t n_records) : n(n_records) {
    queue = 4;
    plist = (size_t)n + 20;
    rec_cnt = (size_t)((2 * n + 48 + 63) & ~(uint64_t)63);
    cw = rec_cnt + (size_t)(C3_MAXSEG + 1) * C3_CSTRIDE;
    seg_cap = cw + 3 * CO_MAXCOV + 1;
    seg_base = seg_cap + C3_MAXSEG;
    words = 2 * (size_t)n + 128 + (size_t)(C3_MAXSEG + 1) * C3_CSTRIDE + 4 * CO_MAXCOV + 2 * C3_MAXSEG + 32;
    pf_grid = (unsigned)((n + 256 * PF_TILES - 1) / (256 * PF_TILES));
    cap_s1 = ((uint64_t)pf_grid * 4 + C3_NSEG - 1) / C3_NSEG * (uint64_t)(PF_TILES * 64);
  }
  // the record area by the one-length kernel's mode (1 or 2): first slot of the other region = the class-1 area's capacity; records in all
  uint64_t other_at(int mode) const { return mode == 2 ? n : (uint64_t)C3_NSEG * cap_s1; }
  size_t rec_slots(int mode) const { return (size_t)other_at(mode) + (mode == 2 ? 2 : 1) * (size_t)n + 64; }
  bool too_many() const { return (uint64_t)C3_NSEG * cap_s1 + 2 * n >= 0xFFFFFFF0ull; }  // record slots are 32-bit
};

}  // namespace elp

// ApplyBQSR's plans are a header of their own; whoever includes this one has them too (apply3_bytes lived here before)
#include "apply_plan.hpp"
