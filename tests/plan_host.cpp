// plan_host.cpp — elprep_amd/csrc/bqsr_plan.hpp behind C functions, for tests/test_bqsr_plan_cpu.py.  The header is host arithmetic: this
// file is built by the host compiler alone.  The kernels' static LDS comes from the caller (lds: count3, count 512, count 1024).
#include "../elprep_amd/csrc/bqsr_plan.hpp"

using namespace elp;

static GatherShape shape(int n_cov, int lmax, int max_cycle, uint32_t uniform_len, int count_kernel, int count3_rlog, const uint64_t *lds) {
  return GatherShape{n_cov, lmax, max_cycle, uniform_len, count_kernel, count3_rlog, (size_t)lds[0], (size_t)lds[1], (size_t)lds[2]};
}

extern "C" {

int plan_c3_mode(int n_cov, int nq, int lmax, int max_cycle, uint32_t uniform_len, int count_kernel, int count3_rlog, const uint64_t *lds) {
  return c3_mode(shape(n_cov, lmax, max_cycle, uniform_len, count_kernel, count3_rlog, lds), nq);
}

// out: rsw, rlog, dyn; returns 1 if the tables do not fit
int plan_count3(int n_cov, int nq, int lmax, uint64_t static_lds, int force_rlog, uint64_t *out) {
  int rsw = 0, rlog = 0;
  size_t dyn = 0;
  const int rc = count3_plan(n_cov, nq, lmax, (size_t)static_lds, &rsw, &rlog, &dyn, force_rlog);
  out[0] = (uint64_t)rsw; out[1] = (uint64_t)rlog; out[2] = (uint64_t)dyn;
  return rc;
}

// out: fits, wg_per_cu, big, mg, rs, ncp, qcap, passes, dyn of a full pass (ncp covariates x min(qcap, nq) slots)
void plan_general(int n_cov, int nq, int lmax, const uint64_t *lds, int64_t *out) {
  const CountPlan p = count_general_plan(shape(n_cov, lmax, 0, 0, 0, -1, lds), nq);
  out[0] = p.fits; out[1] = p.wg_per_cu; out[2] = p.big; out[3] = p.mg; out[4] = p.rs; out[5] = p.ncp; out[6] = p.qcap; out[7] = p.passes;
  out[8] = p.fits ? (int64_t)p.dyn(p.ncp, p.qcap < nq ? p.qcap : nq) : 0;
}

// out: queue, plist, rec_cnt, cw, seg_cap, seg_base, words, pf_grid, cap_s1, other_at(1), rec_slots(1), other_at(2), rec_slots(2)
void plan_scratch(uint64_t n, uint64_t *out) {
  const GatherScratch S(n);
  out[0] = S.queue; out[1] = S.plist; out[2] = S.rec_cnt; out[3] = S.cw; out[4] = S.seg_cap; out[5] = S.seg_base; out[6] = S.words;
  out[7] = S.pf_grid; out[8] = S.cap_s1;
  out[9] = S.other_at(1); out[10] = S.rec_slots(1); out[11] = S.other_at(2); out[12] = S.rec_slots(2);
}

// every plan of n_cov 1..255 x nq 1..88 x lmaxs in one call: out[n_cov - 1][nq - 1][l][12] = plan_general's nine values, then the one-length
// kernel's mode (reads of the one length lmax, --max-cycle 2000, no tuning) and, if it is not 0, its plan's rlog and dyn
void plan_sweep(const int *lmaxs, int n_lmax, const uint64_t *lds, int64_t *out) {
  for (int n_cov = 1; n_cov <= 255; n_cov++)
    for (int nq = 1; nq <= 88; nq++)
      for (int l = 0; l < n_lmax; l++) {
        int64_t *o = out + (((size_t)(n_cov - 1) * 88 + (size_t)(nq - 1)) * (size_t)n_lmax + (size_t)l) * 12;
        plan_general(n_cov, nq, lmaxs[l], lds, o);
        const int mode = plan_c3_mode(n_cov, nq, lmaxs[l], 2000, (uint32_t)lmaxs[l], 0, -1, lds);
        uint64_t p3[3] = {0, 0, 0};
        if (mode) (void)plan_count3(mode == 2 ? 1 : n_cov, nq, lmaxs[l], lds[0], -1, p3);
        o[9] = mode; o[10] = (int64_t)p3[1]; o[11] = (int64_t)p3[2];
      }
}

}  // extern "C"
