// markdup_plan_host.cpp — elprep_amd/csrc/markdup_plan.hpp behind C functions, for tests/test_markdup_plan_cpu.py.  The header is host
// arithmetic: this file is built by the host compiler alone.
#include "../elprep_amd/csrc/markdup_plan.hpp"

using namespace elp;

extern "C" {

// out: T, bbits, ndig, sbits, nb, bw, tab_cap, npmax, nfx,
//      grid, frag_list_blocks, front_grid, mate_grid, coarse_grid, list_grid, bounds_grid, frag_list_grid(n_cu)
void md_sizes(uint64_t n, int n_cu, uint64_t *out) {
  const MdSizes S(n);
  const uint64_t v[17] = {S.T, (uint64_t)S.bbits, (uint64_t)S.ndig, (uint64_t)S.sbits, S.nb, S.bw, S.tab_cap, S.npmax, S.nfx,
                          S.grid, S.frag_list_blocks, S.front_grid, S.mate_grid, S.coarse_grid, S.list_grid, S.bounds_grid, S.frag_list_grid(n_cu)};
  for (int k = 0; k < 17; k++) out[k] = v[k];
}

// out: table, best, winner, fkey, big, flist, words1, bounds_words, coarse, hash32, code, tab_list, hash_lo, words6,
//      then slot 7 for Tf slots: pv, ftable, fbits, words64
void md_scratch(uint64_t n, uint64_t Tf, uint64_t *out) {
  const MdScratch L{MdSizes(n)};
  const MdScratch::Pairs P = L.pairs(Tf);
  const uint64_t v[18] = {L.table, L.best, L.winner, L.fkey, L.big, L.flist, L.words1, L.bounds_words,
                          L.coarse, L.hash32, L.code, L.tab_list, L.hash_lo, L.words6, P.pv, P.ftable, P.fbits, P.words64};
  for (int k = 0; k < 18; k++) out[k] = v[k];
}

uint64_t md_table_size_for(uint64_t n) { return table_size_for(n); }
uint64_t md_frag_table_size(uint32_t nf, uint64_t T) { return frag_table_size(nf, T); }

// out: fixed, fast, listed, nfixed, Tm, list_n
void md_mate_plan(uint64_t n, uint32_t n_tab, int mate_path, uint64_t T, uint64_t *out) {
  const MatePlan P = mate_plan(n, n_tab, mate_path, T);
  out[0] = P.fixed; out[1] = P.fast; out[2] = P.listed; out[3] = P.nfixed; out[4] = P.Tm; out[5] = P.list_n;
}

}  // extern "C"
