// bqsr_apply.hip — elp_bqsr_apply: ApplyBQSR on the HBM column store as a chain of forms.  The plan (apply_plan.hpp) says where the chain
// starts; the one-length kernel (apply3.hip) says on the device when a form's row dictionary (bqsr_lut.hip) does not hold the LUT's distinct
// rows, and the next form takes over: one dictionary -> one per covariate -> the general kernel (apply_flat.hip) with a two-level LUT in LDS
// -> the general kernel on the dense LUT.
//
// Reference: BaseRecalibratorTables.ApplyBQSR (filters/bqsr.go:936-1005).
#include "bqsr_common.hpp"

using namespace elp;

extern "C" {

static int bqsr_apply_impl(elp_ctx *c, int max_cycle, const uint8_t *lut, const uint8_t *cov_present);
int elp_bqsr_apply(elp_ctx *c, int max_cycle, const uint8_t *lut, const uint8_t *cov_present) {
  const int rc = bqsr_apply_impl(c, max_cycle, lut, cov_present);
  if (c && !lut && rc == 0) {  // the kernels just queued read the uploaded LUT: the next upload waits for them
    if (!c->apply_ev && hipEventCreateWithFlags(&c->apply_ev, hipEventDisableTiming) != hipSuccess) return set_error(c, ELP_ERR_HIP, "hipEventCreate failed");
    ELP_HIP(c, hipEventRecord(c->apply_ev, c->stream));
  }
  return rc;
}
static int bqsr_apply_impl(elp_ctx *c, int max_cycle, const uint8_t *lut, const uint8_t *cov_present) {
  if (!c || max_cycle < 1 || (lut != nullptr) != (cov_present != nullptr)) return set_error(c, ELP_ERR_ARG, "elp_bqsr_apply: bad arguments");
  if (!lut && c->lut_uploaded_cycle != max_cycle) return set_error(c, ELP_ERR_ARG, "elp_bqsr_apply: no LUT given and none uploaded for this --max-cycle (elp_bqsr_lut_upload)");
  ELP_HIP(c, hipSetDevice(c->device));
  if (c->n_cov > 255) return set_error(c, ELP_ERR_UNSUPPORTED, "more than 255 read-group covariates");
  const size_t lut_bytes = (size_t)c->n_cov * ELP_NQUAL * (2 * (size_t)max_cycle + 1) * 17;
  ELP_TRY(ensure_adapted(c, false));  // low-quality-tail bounds per read (adapt_score)
  uint8_t *dl;
  if (lut) {
    ELP_TRY(scratch(c, 0, lut_bytes + (size_t)c->n_cov + 64, &dl));
    ELP_HIP(c, hipMemcpyAsync(dl, lut, lut_bytes, hipMemcpyHostToDevice, c->stream));
    ELP_HIP(c, hipMemcpyAsync(dl + lut_bytes, cov_present, (size_t)c->n_cov, hipMemcpyHostToDevice, c->stream));
  } else {
    dl = c->lut_dev.p;  // uploaded ahead of the call: this stream waits for the copy, not the host
    ELP_HIP(c, hipStreamWaitEvent(c->stream, c->lut_ev, 0));
  }
  if (c->n && c->qual_bytes) {
    // ---- the plan
    ELP_TRY(ensure_flat_index(c));
    ELP_TRY(ensure_qual_present(c));  // the resident quality range comes from a sample of the column (a hint: qualities outside it take the fix-up path)
    ELP_TRY(ensure_uniform_len(c));
    const ApplyShape S = apply_shape(c, max_cycle);
    const ApplyPlan P = apply_plan(S);
    // ---- the dictionary: the distinct rows of the resident part of the LUT, built behind the LUT's upload if that was possible
    // (elp_bqsr_lut_upload), else here; `form` 1: one for all covariates, 2: one per covariate
    LutDict D{};
    int dict_form = 0;
    if (P.a3 || P.flat_lds_lut) {
      const LutDictLayout L(c->n_cov, P.n_qi, P.lmax);
      uint32_t *wk = c->lut_wk.p;
      if (c->dict_built.serves(P, lut != nullptr)) dict_form = c->dict_built.form;
      else ELP_TRY(scratch(c, 4, L.words, &wk));
      D = lut_dict_at(wk, L);
    }
    auto dict = [&](int form) -> int {
      if (dict_form == form) return 0;
      c->dict_built.form = 0;  // (a prebuilt dictionary of the other form is overwritten)
      dict_form = form;
      return lut_dict_build(c, c->stream, D, dl, P.qlo, P.n_qi, P.lmax, max_cycle, form == 2);
    };
    // ---- the one-length kernel.  The number(s) of distinct rows stay on the device: if there are more than the one-byte ids hold the
    // kernel says so (bit 512) and leaves without touching a byte - the next form takes over
    size_t dyn3 = P.dyn3;
    for (int a3 = P.a3; a3; a3 = apply3_after_overflow(S, P, a3, &dyn3)) {
      ELP_TRY(dict(a3));
      ELP_TRY(apply3_launch(c, max_cycle, dl, dl + lut_bytes, D.t1, D.t2, D.counter, P.n_qi, P.lmax, dyn3, a3 == 2));
      uint32_t e3[4];
      ELP_TRY(fetch_err(c, e3));
      if ((e3[0] & ~512u) != 0) return bqsr_error(c, e3[0] & ~512u);
      if (!(e3[0] & 512u)) {
        c->derived.qual_changed();
        return 0;
      }
      ELP_HIP(c, hipMemsetAsync(c->err_flag.p, 0, 4, c->stream));
    }
    // ---- the general kernel: its LDS form shows when the number of distinct rows is known
    uint32_t n_dict = NO_DICT;
    if (P.flat_lds_lut) {
      ELP_TRY(dict(1));
      ELP_HIP(c, hipMemcpyAsync(&n_dict, D.counter, 4, hipMemcpyDeviceToHost, c->stream));
      ELP_HIP(c, elp::stream_wait(c->stream));
    }
    ELP_TRY(apply_flat_launch(c, S, P, dl, dl + lut_bytes, D.t1, D.t2, n_dict));
  }
  uint32_t e[4];
  ELP_TRY(fetch_err(c, e));
  if (e[0]) return bqsr_error(c, e[0]);
  c->derived.qual_changed();  // (the scores and the quality hint; the keys do not read QUAL)
  return 0;
}

}  // extern "C"
