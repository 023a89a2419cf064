// sw_plan.hpp — host arithmetic of elp_sw_align / elp_sw_align_reads (sw.hip): the limits and refusals, what a problem needs of the
// chunk scratch and where it lies there, the cut of the listed problems into chunks under a scratch budget, and the layout of the
// context's scratch slots.  No HIP: tests/sw_plan_host.cpp and tests/sw_plan_asan.cpp compile it with the host compiler.
//
// Who owns which scratch slot of the context during a call (nothing is kept between calls; the side lanes have pools of their own):
//   slot 0  SwInputs: the reference pool, its offsets, ref_of, alt_of (elp_sw_align_reads: the staging indices too)
//   slot 4  the alternate pool and its offsets (uploaded, or decoded from the staged SEQ column)
//   slot 1  SwPerProblem: miss flags, op counts and their scan, alignment offsets, CIGAR offsets, the listed problems' descriptors
//   slot 2  SwChunk: backtrack cells, raw operations and tile edges of the chunk that runs
//   slot 3  the CIGAR words on their way out
//   slot 5  per problem that missed the shortcut: its entry of the list
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "sw_core.hpp"

namespace elp {

constexpr uint64_t SW_SCRATCH_DEFAULT = 1ull << 30;  // bytes of chunk scratch a call takes at most (a larger single problem still runs);
                                                     // elp_set_tuning "sw_scratch_bytes"
constexpr uint64_t SW_MAX_PROBLEMS = 1ull << 31;

enum SwRefusal { SW_OK = 0, SW_REFUSE_ARG = 1, SW_REFUSE_UNSUPPORTED = 2 };
struct SwCheck {
  SwRefusal code = SW_OK;
  std::string text;
  uint64_t ops_bound = 0;  // sum of len_ref + len_alt + 2 over the problems: no result has more operations
};
inline SwCheck sw_refuse(SwRefusal code, const char *fmt, unsigned long long a = 0, unsigned long long b = 0) {
  char buf[200];
  snprintf(buf, sizeof buf, fmt, a, b);
  SwCheck r;
  r.code = code;
  r.text = buf;
  return r;
}
// the four parameters and the strategy
inline SwCheck sw_check_params(int32_t match, int32_t mismatch, int32_t gap_open, int32_t gap_extend, int strategy) {
  if (strategy < 0 || strategy > 3) return sw_refuse(SW_REFUSE_ARG, "strategy %llu is none of softclip, indel, leadingIndel, ignore", (unsigned long long)(unsigned)strategy);
  for (const int32_t v : {match, mismatch, gap_open, gap_extend})
    if (v > SW_MAX_PARAM || v < -SW_MAX_PARAM) return sw_refuse(SW_REFUSE_UNSUPPORTED, "a parameter beyond +-65535");
  return SwCheck{};
}
// a pool's offsets: n + 1 entries from 0 that do not decrease
inline SwCheck sw_check_pool(const char *which, uint64_t n_seq, const uint64_t *off) {
  if (n_seq == 0) return SwCheck{};
  if (!off) return sw_refuse(SW_REFUSE_ARG, which[0] == 'a' ? "a_off is NULL" : "b_off is NULL");
  if (off[0] != 0) return sw_refuse(SW_REFUSE_ARG, which[0] == 'a' ? "a_off[0] is not 0" : "b_off[0] is not 0");
  for (uint64_t k = 0; k < n_seq; k++)
    if (off[k + 1] < off[k]) return sw_refuse(SW_REFUSE_ARG, which[0] == 'a' ? "a_off decreases at %llu" : "b_off decreases at %llu", k);
  return SwCheck{};
}
// one sequence a problem uses: not empty (the reference's answer there is an accident of its loops: refused), at most SW_MAX_LEN
inline SwCheck sw_check_length(uint64_t problem, uint64_t len, bool is_ref) {
  if (len == 0) return sw_refuse(SW_REFUSE_ARG, is_ref ? "problem %llu uses an empty reference sequence" : "problem %llu uses an empty alternate sequence", problem);
  if (len > SW_MAX_LEN)
    return sw_refuse(SW_REFUSE_UNSUPPORTED, is_ref ? "problem %llu: a reference sequence of %llu bytes (at most 4095)" : "problem %llu: an alternate sequence of %llu bytes (at most 4095)",
                     problem, len);
  return SwCheck{};
}
// the index pairs of a batch against their pools; len_ref / len_alt receive the problems' lengths (n entries each)
inline SwCheck sw_check_batch(uint64_t n_a, const uint64_t *a_off, uint64_t n_b, const uint64_t *b_off, uint64_t n, const uint32_t *ref_of, const uint32_t *alt_of,
                              uint32_t *len_ref, uint32_t *len_alt) {
  if (n >= SW_MAX_PROBLEMS) return sw_refuse(SW_REFUSE_UNSUPPORTED, "more than 2^31 - 1 problems");
  SwCheck r = sw_check_pool("a", n_a, a_off);
  if (r.code) return r;
  r = sw_check_pool("b", n_b, b_off);
  if (r.code) return r;
  if (n && (!ref_of || !alt_of)) return sw_refuse(SW_REFUSE_ARG, "an index array is NULL");
  uint64_t bound = 0;
  for (uint64_t k = 0; k < n; k++) {
    if (ref_of[k] >= n_a) return sw_refuse(SW_REFUSE_ARG, "ref_of[%llu] = %llu is outside the reference pool", k, ref_of[k]);
    if (alt_of[k] >= n_b) return sw_refuse(SW_REFUSE_ARG, "alt_of[%llu] = %llu is outside the alternate pool", k, alt_of[k]);
    const uint64_t m = a_off[ref_of[k] + 1] - a_off[ref_of[k]], q = b_off[alt_of[k] + 1] - b_off[alt_of[k]];
    r = sw_check_length(k, m, true);
    if (r.code) return r;
    r = sw_check_length(k, q, false);
    if (r.code) return r;
    len_ref[k] = (uint32_t)m;
    len_alt[k] = (uint32_t)q;
    bound += m + q + 2;
  }
  r.ops_bound = bound;
  return r;
}

// ---- what a listed problem (one that missed the shortcut) needs in the chunk scratch, in units of the three arrays
struct SwNeed {
  uint64_t bt_cells;   // int16 backtrack cells: sw_bt_cells, a multiple of 4 (the strips' 8-byte stores stay aligned)
  uint64_t raw_words;  // uint32: len_ref + len_alt + 3 raw operations and, behind them, their number; rounded up to 2
  uint64_t edge_words; // int32: 3 per row where the alternate is wider than a tile, rounded up to 2; else 0
  uint64_t bytes() const { return bt_cells * 2 + raw_words * 4 + edge_words * 4; }
};
inline SwNeed sw_need(uint32_t m, uint32_t n) {
  SwNeed d;
  d.bt_cells = sw_bt_cells(m, n);
  d.raw_words = ((uint64_t)m + n + 3 + 1 + 1) & ~1ull;
  d.edge_words = n > SW_TILE ? ((3ull * m + 1) & ~1ull) : 0;
  return d;
}
// what the DP kernel gets per listed problem: its number in the batch and where its three regions begin in the chunk's arrays
struct SwProb {
  uint32_t k, pad;
  uint64_t bt_at, raw_at, edge_at;
};
// a chunk: listed problems [first, end), and what their regions add up to
struct SwChunkCut {
  uint64_t first, end, bt_cells, raw_words, edge_words;
};
// the chunk scratch: three arrays one behind the other, each from a multiple of 8 bytes (every count above is even in 4-byte units
// and a multiple of 4 in 2-byte units); `bytes` includes nothing else
struct SwChunk {
  uint64_t bt_at = 0, raw_at, edge_at, bytes;  // byte offsets
  explicit SwChunk(const SwChunkCut &c) {
    raw_at = bt_at + c.bt_cells * 2;
    edge_at = raw_at + c.raw_words * 4;
    bytes = edge_at + c.edge_words * 4;
  }
};
// cuts the listed problems, in order, into chunks of at most `budget` bytes; a problem larger than the budget is a chunk of its own.
// probs[i].k is given; the three offsets are filled in, relative to the chunk's arrays.
inline std::vector<SwChunkCut> sw_chunks(std::vector<SwProb> &probs, const uint32_t *len_ref, const uint32_t *len_alt, uint64_t budget) {
  std::vector<SwChunkCut> cuts;
  SwChunkCut cur{0, 0, 0, 0, 0};
  for (uint64_t i = 0; i < probs.size(); i++) {
    const SwNeed d = sw_need(len_ref[probs[i].k], len_alt[probs[i].k]);
    const uint64_t used = cur.bt_cells * 2 + cur.raw_words * 4 + cur.edge_words * 4;
    if (cur.end > cur.first && used + d.bytes() > budget) {
      cuts.push_back(cur);
      cur = SwChunkCut{i, i, 0, 0, 0};
    }
    probs[i].pad = 0;
    probs[i].bt_at = cur.bt_cells;
    probs[i].raw_at = cur.raw_words;
    probs[i].edge_at = cur.edge_words;
    cur.bt_cells += d.bt_cells;
    cur.raw_words += d.raw_words;
    cur.edge_words += d.edge_words;
    cur.end = i + 1;
  }
  if (cur.end > cur.first) cuts.push_back(cur);
  return cuts;
}

// ---- slot 1: per problem and per listed problem; every array from a multiple of 8 bytes
struct SwPerProblem {
  uint64_t miss, n_ops, scan, offset, cigar_off, probs, bytes;  // byte offsets
  SwPerProblem(uint64_t n, uint64_t n_listed) {
    auto up8 = [](uint64_t v) { return (v + 7) & ~7ull; };
    miss = 0;                                 // uint32[n]: 1 = the problem goes through the DP
    n_ops = up8(miss + 4 * n);                // uint32[n + 1]: operations of the result (entry n: 0)
    scan = up8(n_ops + 4 * (n + 1));          // uint32[n + 1]: their exclusive scan, chunk by chunk
    offset = up8(scan + 4 * (n + 1));         // int32[n]
    cigar_off = up8(offset + 4 * n);          // uint64[n + 1]
    probs = cigar_off + 8 * (n + 1);          // SwProb[n_listed]
    bytes = probs + sizeof(SwProb) * n_listed;
  }
};
// ---- slot 0 (and slot 4 for the alternates): a pool, its offsets and up to three index arrays
struct SwInputs {
  uint64_t seq, off, idx0, idx1, idx2, bytes;
  SwInputs(uint64_t pool_bytes, uint64_t n_seq, uint64_t n) {
    auto up8 = [](uint64_t v) { return (v + 7) & ~7ull; };
    seq = 0;
    off = up8(pool_bytes);           // uint64[n_seq + 1]
    idx0 = off + 8 * (n_seq + 1);    // uint32[n] each
    idx1 = up8(idx0 + 4 * n);
    idx2 = up8(idx1 + 4 * n);
    bytes = up8(idx2 + 4 * n);
  }
};

}  // namespace elp
