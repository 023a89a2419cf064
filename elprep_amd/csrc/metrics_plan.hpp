// metrics_plan.hpp — the duplication-metrics pass's launch plan as plain host arithmetic: every size, scratch offset, grid and LDS byte
// count of a call of elp_dup_metrics / elp_dup_metrics_hist, and the host arithmetic behind its last copy (mx_finish).  Nothing here
// touches the device or includes HIP: the header compiles with the host compiler alone (tests/metrics_plan_host.cpp,
// tests/test_metrics_plan_cpu.py).  metrics.hip's phases take their sizes and offsets from here and compute none themselves.
//
// Who owns a slot of elp_ctx::scratch (the side lane's own pool) in which phase of a call
// (counters -> groups -> small sets -> large sets -> origins -> read back):
//   slot 0  ctr | origins | hist | pair_reads   u64   all phases: the counter block, zeroed first, read back with one copy (MxSizes)
//   slot 1  pk x 2 | pv x 2                      u64, u32   counters .. groups: the loser list (pair group, owner) and its sort buffers
//           head | gidx | gstart                 u32   groups .. small sets: in the halves the sort left free (MxListScratch::groups)
//   slot 2  members                              32 B  small sets .. large sets: tile / x / y / RG and strand of every member slot
//   slot 3  parent | mset | linfo | lcount | setcnt | lvals x 2 | lkeys x 2     u32 but setcnt and lkeys u64 (MxSetScratch)
//           small sets: parent (union-find of sets of 4..OPT_SMALL), mset, linfo, lcount; large sets: all of it (parent anew)
//   slot 4  mread                                u32   small sets: the read listed at every member slot
//   slot 5  ginfo                                2 x u32   small sets .. large sets: {set size, owner of the origin} at an origin's slot
// Slots are grow-only and every size is taken before the slot's first kernel of the call.  Offsets are 32-bit words from the slot's start.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "../../include/elprep_hip.h"  // ELP_NCTR

namespace elp {

// ---- sizes the plan shares with the kernels (metrics.hip describes each beside its kernel)
constexpr uint32_t OPT_SMALL = 32;         // sets up to this size: one thread, all pairs
constexpr uint32_t OPT_LIST_CAP = 300000;  // filters/mark-optical-duplicates.go:289-299
constexpr int DC_CAP = 2048, DC_STEP = 1024;  // k_dup_counters: losers a workgroup holds in LDS; records per round of a workgroup
constexpr unsigned MX_GRID_CAP = 2048;     // k_dup_counters, k_opt_eval, k_origin_count: at most this many workgroups (each ends with
                                           // atomics on the same few global counters)
constexpr int MX_EVAL_THREADS = 128;       // k_opt_eval
constexpr int MX_HIST_LDS_BINS = 32;       // k_opt_eval: the first bins of every histogram are collected in LDS
// k_dup_counters' dynamic LDS (a 32-bit cell per counter and per (split, library)): static and dynamic LDS of a workgroup stay under
// 64 KB = 65 536 B, and the kernel has 16 392 B of static LDS (lq: DC_CAP x 8 B, two words); 46 000 + 16 392 = 62 392.
constexpr size_t MX_COUNTERS_LDS = 46000;
// k_opt_eval's dynamic LDS (the optical counts and, if they fit, the histograms' first bins): half of the 64 KB; no static LDS.
// Over it the bins are dropped (every histogram count is a global atomic), never the call.
constexpr size_t MX_EVAL_LDS = 32768;

// words of the context's error block (elp_ctx::err_flag, four words) the pass uses: k_opt_eval raises word 2 for a name the reference
// would have panicked on; word 3 is the pass's mailbox - zero between its uses, it carries the length of the loser list, then the
// members of large sets, then their candidates to the host
constexpr int MX_NAME_ERR_WORD = 2, MX_MAILBOX_WORD = 3;

inline unsigned mx_blocks(uint64_t n, unsigned per_block = 256) { return (unsigned)((n + per_block - 1) / per_block); }

// ---- everything the arguments of a call fix.  n_lib: libraries of the header (the "Unknown Library" row comes on top); n_split:
// 1 + largest staged split id; hist_len: bins per histogram, 0 = no histograms (elp_dup_metrics)
struct MxSizes {
  uint64_t n;
  int n_lib, n_split, hist_len;
  // the counter block, in 64-bit elements: ctr [0, ncell) = [n_lib + 1][ELP_NCTR] | origins, norg | hist, nhist = [n_lib + 1][3][hist_len]
  // | pair_reads, npr = [n_split][n_lib + 1].  `cells` are zeroed and read back; `block` = cells + 8 are asked for (as it was)
  size_t ncell, norg, nhist, npr, origins, hist, pair_reads, cells, block;
  bool lds_refused;      // more (split, library) cells than k_dup_counters has LDS for: the call is refused
  size_t counters_lds;   // k_dup_counters: dynamic LDS bytes, workgroups, records per workgroup (a multiple of DC_STEP)
  unsigned counters_grid;
  uint64_t chunk;
  size_t lcap;           // the loser list's capacity: a losing pair per two records at most, + 8
  int ndig;              // radix digits of the list's sort: its keys are record indices < n < 2^32
  int lds_bins;          // k_opt_eval: histogram bins kept in LDS (0: none, or no histograms), and its dynamic LDS bytes
  size_t eval_lds;
  unsigned origin_grid;  // k_origin_count
  size_t origin_lds;
  MxSizes(uint64_t records, int libs, int splits, int hlen) : n(records), n_lib(libs), n_split(splits), hist_len(hlen) {
    const size_t rows = (size_t)n_lib + 1;
    ncell = rows * ELP_NCTR;
    norg = hist_len ? rows : 0;
    nhist = rows * 3 * (size_t)hist_len;
    npr = (size_t)n_split * rows;
    origins = ncell;
    hist = origins + norg;
    pair_reads = hist + nhist;
    cells = pair_reads + npr;
    block = cells + 8;
    counters_lds = (ncell + npr) * sizeof(unsigned int);
    lds_refused = counters_lds > MX_COUNTERS_LDS;
    counters_grid = (unsigned)std::min<uint64_t>(MX_GRID_CAP, (n + DC_STEP - 1) / DC_STEP);
    chunk = counters_grid ? (((n + counters_grid - 1) / counters_grid) + DC_STEP - 1) / DC_STEP * DC_STEP : 0;
    lcap = (size_t)(n / 2 + 8);
    ndig = 1;
    while (ndig < 4 && (n >> (8 * ndig)) != 0) ndig++;
    lds_bins = std::min(hist_len, MX_HIST_LDS_BINS);
    if (rows * (1 + 3 * (size_t)lds_bins) * sizeof(unsigned int) > MX_EVAL_LDS) lds_bins = 0;
    eval_lds = rows * (1 + 3 * (size_t)lds_bins) * sizeof(unsigned int);
    origin_grid = std::min(mx_blocks(n), MX_GRID_CAP);
    origin_lds = rows * sizeof(unsigned int);
  }
};

// ---- slot 1: the loser list.  pk = 2 lcap 64-bit keys (the list, then the sort's second buffer) at word 0, pv = 2 lcap values at word
// 4 lcap; 6 lcap + 16 words in all (the + 16 as it was).  The sort leaves keys and values each in one half of their buffers
struct MxListScratch {
  size_t lcap, words, pk, pv;
  explicit MxListScratch(size_t cap) : lcap(cap), words(6 * cap + 16), pk(0), pv(4 * cap) {}
  size_t keys_half(bool first) const { return first ? pk : pk + 2 * lcap; }
  size_t vals_half(bool first) const { return first ? pv : pv + lcap; }
  // The halves the sort left free hold the head flags and the group numbers (L words each, in the free key half: lcap 64-bit keys =
  // 2 lcap words) and the group starts (in the free value half).  gstart[G] is written as well: G + 1 <= L + 1 words, and
  // L <= n / 2 = lcap - 8, so the lcap words of the half hold them.
  struct Groups { size_t head, gidx, gstart; };
  Groups groups(bool keys_in_first, bool vals_in_first) const {
    const size_t head = keys_half(!keys_in_first);
    return Groups{head, head + lcap, vals_half(!vals_in_first)};
  }
  static unsigned grid(uint32_t L) { return mx_blocks(L); }  // k_opt_heads, k_opt_starts, k_opt_slots: a thread per loser
};

// ---- the member slots (total = losers + groups: every group's origin in front of its losers), slots 2 .. 5
struct MxSetScratch {
  size_t total, tp;  // tp: total rounded up to a multiple of 8, so that every array of slot 3 starts 32-byte aligned
  // slot 3, 12 tp + 16 words (the + 16 as it was): seven arrays one behind the other, setcnt (tp) and lkeys (2 tp) of 64-bit elements
  size_t words3, parent, mset, linfo, lcount, setcnt, lvals, lvals_tmp, lkeys, lkeys_tmp;  // _tmp: the sort's second buffer
  // one memset over three arrays of two element widths: linfo (bit 0: a large set), lcount and setcnt must read 0 where k_opt_eval and
  // k_large_roots wrote nothing; they are adjacent, 4 tp words
  size_t zero, zero_words;
  size_t members, mread, ginfo;  // elements of slots 2, 4, 5 (the + 4 as it was)
  unsigned member_grid, eval_grid;  // a thread per member slot: k_opt_fill, k_large_list, k_large_final; k_opt_eval (strided)
  explicit MxSetScratch(uint32_t members_total) : total(members_total), tp(((size_t)members_total + 7) & ~(size_t)7) {
    words3 = 12 * tp + 16;
    parent = 0;
    mset = tp;
    linfo = 2 * tp;
    lcount = 3 * tp;
    setcnt = 4 * tp;
    lvals = 6 * tp;
    lvals_tmp = 7 * tp;
    lkeys = 8 * tp;
    lkeys_tmp = 10 * tp;
    zero = linfo;
    zero_words = 4 * tp;
    members = mread = ginfo = total + 4;
    member_grid = mx_blocks(total);
    eval_grid = std::min(mx_blocks(total, MX_EVAL_THREADS), MX_GRID_CAP);
  }
  static unsigned cand_grid(uint32_t cl) { return mx_blocks(cl); }  // k_iota32, k_large_union, k_large_roots: a thread per candidate
};

// ---- the host arithmetic behind the last copy.  h: the counter block as read back (S.cells elements); counters: [n_lib + 1][ELP_NCTR];
// hist: [n_lib + 1][3][hist_len], null without histograms
inline void mx_finish(const MxSizes &S, const unsigned long long *h, int64_t *counters, int64_t *hist) {
  for (int l = 0; l <= S.n_lib; l++)
    for (int k = 0; k < ELP_NCTR; k++) counters[l * ELP_NCTR + k] = (int64_t)h[l * ELP_NCTR + k];
  // ReadPairsExamined counts reads, then halves (:504-506) - per filter run, i.e. per split file
  for (int l = 0; l <= S.n_lib; l++) {
    int64_t pairs = 0;
    for (int sp = 0; sp < S.n_split; sp++) pairs += (int64_t)(h[S.pair_reads + (size_t)sp * (S.n_lib + 1) + l] / 2);
    counters[l * ELP_NCTR + 1] = pairs;
  }
  if (!hist) return;
  // the device counted the sets that have duplicates; an origin without duplicates is a set of one read, none of them optical
  const int hist_len = S.hist_len;
  const unsigned long long *ho = h + S.origins, *hh = h + S.hist;
  for (int l = 0; l <= S.n_lib; l++) {
    int64_t *out = hist + (size_t)l * 3 * hist_len;
    unsigned long long with_dups = 0;
    for (size_t k = 0; k < (size_t)3 * hist_len; k++) out[k] = (int64_t)hh[(size_t)l * 3 * hist_len + k];
    for (int b = 0; b < hist_len; b++) with_dups += hh[(size_t)l * 3 * hist_len + b];
    const int64_t alone = (int64_t)(ho[l] - with_dups);
    const int one = 1 < hist_len ? 1 : hist_len - 1;
    out[one] += alone;             // duplicatesCountHistogram[1]
    out[hist_len + one] += alone;  // nonOpticalDuplicatesCountHistogram[1]
  }
}

}  // namespace elp
