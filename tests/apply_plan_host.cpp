// apply_plan_host.cpp — elprep_amd/csrc/apply_plan.hpp behind C functions, for tests/test_apply_plan_cpu.py.  The header is host arithmetic:
// this file is built by the host compiler alone.  A shape travels as 13 integers in ApplyShape's order: n, n_cov, max_l_seq, uniform_len,
// max_cycle, qlo, qhi, apply_kernel, apply_wgs, n_cu, then the static LDS of k_bqsr_apply_flat, k_bqsr_apply3 and its covariate split.
#include "../elprep_amd/csrc/apply_plan.hpp"

using namespace elp;

static ApplyShape shape(const int64_t *s) {
  return ApplyShape{(uint64_t)s[0], (int)s[1], (uint32_t)s[2], (uint32_t)s[3], (int)s[4], (int)s[5], (int)s[6], (int)s[7], (int)s[8], (int)s[9],
                    (size_t)s[10], (size_t)s[11], (size_t)s[12]};
}

extern "C" {

// out: dyn; returns 1 if it does not fit
int plan_apply3(int n_cov, int n_qi, int lmax, uint64_t static_lds, uint64_t *out) {
  size_t dyn = 0;
  const int rc = apply3_bytes(n_cov, n_qi, lmax, (size_t)static_lds, &dyn);
  out[0] = (uint64_t)dyn;
  return rc;
}

// out: chk, want3, qlo, n_qi, lmax, n_rows, n1, a3, dyn3, flat_lds_lut
void ap_plan(const int64_t *s, int64_t *out) {
  const ApplyPlan p = apply_plan(shape(s));
  out[0] = p.chk; out[1] = p.want3; out[2] = p.qlo; out[3] = p.n_qi; out[4] = p.lmax; out[5] = (int64_t)p.n_rows; out[6] = (int64_t)p.n1;
  out[7] = p.a3; out[8] = (int64_t)p.dyn3; out[9] = p.flat_lds_lut;
}

// the form after form a3 overflowed; out: its dyn
int ap_overflow(const int64_t *s, int a3, int64_t *out) {
  const ApplyShape S = shape(s);
  size_t dyn3 = 0;
  const int next = apply3_after_overflow(S, apply_plan(S), a3, &dyn3);
  out[0] = (int64_t)dyn3;
  return next;
}

// out: mode, dyn, per_cu, grid
void ap_flat(const int64_t *s, uint32_t n_dict, uint64_t nsteps, int64_t *out) {
  const ApplyShape S = shape(s);
  const FlatLaunch f = flat_launch_plan(S, apply_plan(S), n_dict, nsteps);
  out[0] = f.mode; out[1] = (int64_t)f.dyn; out[2] = f.per_cu; out[3] = f.grid;
}

// out: n_slots, n_rows, n1, counter, slots, slot_id, row_slot, t1, t2, t2_bytes, words
void ap_dict_layout(int n_cov, int n_qi, int lmax, int64_t *out) {
  const LutDictLayout L(n_cov, n_qi, lmax);
  const size_t v[11] = {L.n_slots, L.n_rows, L.n1, L.counter, L.slots, L.slot_id, L.row_slot, L.t1, L.t2, L.t2_bytes, L.words};
  for (int k = 0; k < 11; k++) out[k] = (int64_t)v[k];
}

// out: group, rpi, per_cu, grid, recs, dump, ridx, cw, blk, size8
void ap_apply3_launch(uint64_t n, uint32_t len, int n_cu, uint64_t dyn, int split, int apply_wgs, uint64_t lds3, uint64_t lds3_split, int64_t *out) {
  const Apply3Launch P(n, len, n_cu, (size_t)dyn, split != 0, apply_wgs, (size_t)lds3, (size_t)lds3_split);
  const size_t v[10] = {P.group, P.rpi, P.per_cu, (size_t)P.grid, P.recs, P.dump, P.ridx, P.cw, P.blk, P.size8};
  for (int k = 0; k < 10; k++) out[k] = (int64_t)v[k];
}

// built: form, qlo, n_qi, lmax, max_cycle, n_cov of a dictionary built ahead, or null: the one the plan of `s_built` builds
int ap_serves(const int64_t *built, const int64_t *s_built, const int64_t *s_now, int lut_in_call) {
  const LutDictBuilt b = built ? LutDictBuilt{(int)built[0], (int)built[1], (int)built[2], (int)built[3], (int)built[4], (int)built[5]}
                               : LutDictBuilt::of(apply_plan(shape(s_built)));
  return b.serves(apply_plan(shape(s_now)), lut_in_call != 0) ? 1 : 0;
}

// every plan of n_cov 1..255 x n_qi 1..88 x lmaxs in one call (reads of the one length lmax, qualities 6 .. 6 + n_qi - 1, --max-cycle 2000,
// no tuning): out[n_cov - 1][n_qi - 1][l][18] = a3, dyn3, flat_lds_lut, then mode and dyn of the general kernel with 255 and with
// LUT_T2_CAP - 1 distinct rows, then ap_dict_layout's eleven values
void ap_sweep(const int *lmaxs, int n_lmax, const int64_t *lds, int64_t *out) {
  for (int n_cov = 1; n_cov <= 255; n_cov++)
    for (int n_qi = 1; n_qi <= 88; n_qi++)
      for (int l = 0; l < n_lmax; l++) {
        int64_t *o = out + (((size_t)(n_cov - 1) * 88 + (size_t)(n_qi - 1)) * (size_t)n_lmax + (size_t)l) * 18;
        const ApplyShape S{1000000, n_cov, (uint32_t)lmaxs[l], (uint32_t)lmaxs[l], 2000, 6, 6 + n_qi - 1, 0, 0, 256, (size_t)lds[0], (size_t)lds[1], (size_t)lds[2]};
        const ApplyPlan p = apply_plan(S);
        o[0] = p.a3; o[1] = (int64_t)p.dyn3; o[2] = p.flat_lds_lut;
        const FlatLaunch f1 = flat_launch_plan(S, p, 255, 1u << 20), f2 = flat_launch_plan(S, p, LUT_T2_CAP - 1, 1u << 20);
        o[3] = f1.mode; o[4] = (int64_t)f1.dyn; o[5] = f2.mode; o[6] = (int64_t)f2.dyn;
        ap_dict_layout(n_cov, n_qi, lmaxs[l], o + 7);
      }
}

}  // extern "C"
