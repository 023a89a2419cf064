// metrics_plan_host.cpp — elprep_amd/csrc/metrics_plan.hpp behind C functions, for tests/test_metrics_plan_cpu.py.  The header is host
// arithmetic: this file is built by the host compiler alone.
#include "../elprep_amd/csrc/metrics_plan.hpp"

using namespace elp;

extern "C" {

// out: ncell, norg, nhist, npr, origins, hist, pair_reads, cells, block, lds_refused, counters_lds, counters_grid, chunk, lcap, ndig,
//      lds_bins, eval_lds, origin_grid, origin_lds
void mx_sizes(uint64_t n, int n_lib, int n_split, int hist_len, uint64_t *out) {
  const MxSizes S(n, n_lib, n_split, hist_len);
  const uint64_t v[19] = {S.ncell, S.norg, S.nhist, S.npr, S.origins, S.hist, S.pair_reads, S.cells, S.block, S.lds_refused, S.counters_lds,
                          S.counters_grid, S.chunk, S.lcap, (uint64_t)S.ndig, (uint64_t)S.lds_bins, S.eval_lds, S.origin_grid, S.origin_lds};
  for (int k = 0; k < 19; k++) out[k] = v[k];
}

// out: words, pk, pv, keys' second half, values' second half, head, gidx, gstart, grid(L)
void mx_list_scratch(uint64_t lcap, int keys_in_first, int vals_in_first, uint32_t L, uint64_t *out) {
  const MxListScratch ls(lcap);
  const MxListScratch::Groups g = ls.groups(keys_in_first != 0, vals_in_first != 0);
  const uint64_t v[9] = {ls.words, ls.pk, ls.pv, ls.keys_half(false), ls.vals_half(false), g.head, g.gidx, g.gstart, MxListScratch::grid(L)};
  for (int k = 0; k < 9; k++) out[k] = v[k];
}

// out: tp, words3, parent, mset, linfo, lcount, setcnt, lvals, lvals_tmp, lkeys, lkeys_tmp, zero, zero_words, members, mread, ginfo,
//      member_grid, eval_grid, cand_grid(cl)
void mx_set_scratch(uint32_t total, uint32_t cl, uint64_t *out) {
  const MxSetScratch s(total);
  const uint64_t v[19] = {s.tp, s.words3, s.parent, s.mset, s.linfo, s.lcount, s.setcnt, s.lvals, s.lvals_tmp, s.lkeys, s.lkeys_tmp, s.zero, s.zero_words,
                          s.members, s.mread, s.ginfo, s.member_grid, s.eval_grid, MxSetScratch::cand_grid(cl)};
  for (int k = 0; k < 19; k++) out[k] = v[k];
}

// h: the counter block as read back (MxSizes::cells elements); hist may be null
void mx_finish_block(uint64_t n, int n_lib, int n_split, int hist_len, const unsigned long long *h, int64_t *counters, int64_t *hist) {
  mx_finish(MxSizes(n, n_lib, n_split, hist_len), h, counters, hist);
}

// the constants the plan shares with the kernels
void mx_constants(uint64_t *out) {
  const uint64_t v[11] = {OPT_SMALL, OPT_LIST_CAP, (uint64_t)DC_CAP, (uint64_t)DC_STEP, MX_GRID_CAP, (uint64_t)MX_EVAL_THREADS, (uint64_t)MX_HIST_LDS_BINS,
                          MX_COUNTERS_LDS, MX_EVAL_LDS, (uint64_t)MX_NAME_ERR_WORD, (uint64_t)MX_MAILBOX_WORD};
  for (int k = 0; k < 11; k++) out[k] = v[k];
}

}  // extern "C"
