// sort_plan.hpp — the sorts' host arithmetic: the key format, the long runs' bounds, the scratch layout on side lane 1, the rank
// tables of the tie-break and how their fields are packed into 64-bit keys.  Nothing here touches the device or includes HIP: the
// header compiles with the host compiler alone (tests/sort_plan_host.cpp, tests/test_sort_plan_cpu.py).  The phases of sort.hip and
// qsort.hip take every size, offset, width and cut from here and compute none themselves; adapt.hip takes the key's width.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace elp {

// ---- sizes the plan shares with the kernels (sort.hip and qsort.hip describe each beside its kernel)
constexpr int TIE_SMALL = 48;                           // k_tie_small: runs up to this length are ranked by all-pairs comparison
constexpr uint32_t TIE_HEAD = 256;                      // run bounds that come with the first read-back
constexpr int TIE_MAX_PACKED = 96;                      // live positions up to which the coordinate sort uses rank keys
constexpr uint16_t QN_STATE = 0xFFFF, QN_LEN = 0xFFFE;  // the queryname key's fields that are no byte position: record state, name length

// ---- key format
// bits of a record index below n: the passes move words key << idx_bits | index where that fits 64 bits, else (key, index) pairs
inline int index_bits(uint64_t n) {
  int b = 1;
  while (b < 32 && (n >> b) != 0) b++;
  return b;
}
inline bool sort_words(int key_bits, int idx_bits, int sort_pairs /* the tuning key: 1 forces pairs */) {
  return key_bits >= 1 && key_bits + idx_bits <= 64 && sort_pairs != 1;
}
// the coordinate key {contig code, POS, strand}: POS in the width of the largest staged POS; contig codes 0 .. n_ref + 1 (unmapped,
// then the records that are not sorted at all)
struct KeyWidth { int pos_bits, ref_bits, key_bits; };
inline KeyWidth key_width(uint32_t max_pos, int32_t n_ref) {
  int pos_bits = 1;
  while (pos_bits < 32 && (max_pos >> pos_bits) != 0) pos_bits++;
  int ref_bits = 1;
  while (ref_bits < 32 && (((uint32_t)n_ref + 1u) >> ref_bits) != 0) ref_bits++;
  return KeyWidth{pos_bits, ref_bits, ref_bits + pos_bits + 1};
}

// ---- long runs (more than TIE_SMALL records of equal key): k_tie_small reports their first and last positions in two unordered lists
inline uint32_t bounds_cap(uint64_t n) { return (uint32_t)std::min<uint64_t>(n / TIE_SMALL + 16, (2 * n + 8 - 4) / 2); }
// the first read-back brings the two counts and `bounds_head` bounds of either list: all of them unless there are more than TIE_HEAD runs
inline uint32_t bounds_head(uint32_t cap) { return std::min<uint32_t>(TIE_HEAD, cap); }
inline bool bounds_in_head(uint32_t nr) { return nr <= TIE_HEAD; }
inline bool run_counts_ok(uint32_t n_starts, uint32_t n_ends, uint32_t cap) { return n_starts == n_ends && n_starts <= cap; }
// Runs are disjoint ranges, so the r-th smallest start belongs to the r-th smallest end.  first[r] = the number of run r's first member
// among all members, first[nr] = nu = their count.  false: an end before its start, or a start at or before the previous end.
struct LongRuns {
  std::vector<uint32_t> starts, ends, first;
  uint32_t nr = 0, nu = 0;
};
inline bool long_runs(std::vector<uint32_t> starts, std::vector<uint32_t> ends, LongRuns *out) {
  const uint32_t nr = (uint32_t)starts.size();
  if (ends.size() != starts.size()) return false;
  std::sort(starts.begin(), starts.end());
  std::sort(ends.begin(), ends.end());
  std::vector<uint32_t> first((size_t)nr + 1);
  uint64_t total = 0;
  for (uint32_t r = 0; r < nr; r++) {
    if (ends[r] < starts[r] || (r + 1 < nr && starts[r + 1] <= ends[r])) return false;
    first[r] = (uint32_t)total;
    total += (uint64_t)ends[r] - starts[r] + 1;
  }
  first[nr] = (uint32_t)total;
  out->nr = nr;
  out->nu = (uint32_t)total;
  out->starts = std::move(starts);
  out->ends = std::move(ends);
  out->first = std::move(first);
  return true;
}
// bits of the run id u_seg = 1 .. nr in front of a key; one run needs none
inline int segbits(uint32_t nr) {
  int s = 0;
  while (nr > 1 && (1u << s) <= nr) s++;
  return s;
}

// ---- the scratch blocks on side lane 1.  Who owns a slot of the lane's elp_ctx::scratch in which phase of a sort:
//   slot 0  kbuf      2 n + 8 x 8 bytes      coordinate sort, key passes .. short runs: the radix passes' two halves.  The pre-made key
//                                            passes (elp_sort_ahead) live here between calls, which is why the queryname sort keeps out
//   slot 1  vbuf      2 n + 8 words          coordinate sort: the pair passes' indices; short runs: the free half is the run members' list
//           kbuf      2 n + 8 x 8 bytes      queryname sort: the keys and the sort's second buffer
//   slot 2  bounds    2 n + 8 words          coordinate sort, short runs .. run bounds: [0] starts, [1] ends counted ([2], [3] zeroed with
//                                            them), [4 + k] the starts, [4 + cap + k] the ends, cap = bounds_cap(n)
//           vbuf      2 n + 8 words          queryname sort: the indices and the sort's second buffer
//   slot 3  u_pos | u_read | u_seg | uv0 | uv1 | d_start | d_first | rows     coordinate sort, long runs: nu words each, then nr and
//                                            nr + 1 words, then - word u_words on - the members' comparator strings, rw bytes each
//           d_vals | d_over | d_lut          queryname sort: the positions' value sets (+ the NUL word), the overflow word, the rank LUT
//   slot 4  uk0 | uk1  2 nu + 16 x 8 bytes   coordinate sort, long runs: the rounds' keys and the sort's second buffer
//   slot 5  d_vals | d_lut                   coordinate sort, rank tables: TIE_MAX_PACKED value sets of eight words, then the LUT rows
// Slots are grow-only, and a sort takes every size before the slot's first kernel.  Offsets are in elements of the slot's type.
struct SortScratch {  // by the record count: slots 0 .. 2 of the coordinate sort, slots 1 and 2 of the queryname sort
  size_t keys, vals, flags;  // elements of a slot; the second half of the first two begins at element n
  uint32_t cap;              // bounds_cap(n)
  size_t starts, ends;       // the two lists in `bounds`
  explicit SortScratch(uint64_t n) : keys(2 * (size_t)n + 8), vals(2 * (size_t)n + 8), flags(2 * (size_t)n + 8), cap(bounds_cap(n)), starts(4), ends(4 + (size_t)cap) {}
};
struct TieScratch {  // by the long runs' members nu, their number nr and the longest name maxq
  uint32_t m_bytes, rw;  // bytes of a comparator string (QNAME zero-padded to maxq + 15 bytes of fields); of a written-out row (16-byte steps)
  bool use_rows;         // the strings are written out if that takes at most 512 MB: else every kernel reads the columns
  size_t u_pos, u_read, u_seg, uv0, uv1, d_start, d_first, u_words, words3;  // slot 3 in words; rows begin at word u_words
  size_t uk0, uk1, words4;                                                   // slot 4 in 64-bit words
  size_t d_vals, d_lut, words5;                                              // slot 5 in words
  TieScratch(uint32_t nu, uint32_t nr, uint32_t maxq) : m_bytes(maxq + 15), rw((maxq + 15u + 15u) & ~15u), use_rows((uint64_t)nu * rw <= (512ull << 20)) {
    u_pos = 0;
    u_read = nu;
    u_seg = 2 * (size_t)nu;
    uv0 = 3 * (size_t)nu;
    uv1 = 4 * (size_t)nu;
    d_start = 5 * (size_t)nu;
    d_first = d_start + nr;
    u_words = ((size_t)5 * nu + 2 * (size_t)nr + 64 + 3) & ~(size_t)3;
    words3 = u_words + (use_rows ? ((size_t)nu * rw + 64) / 4 : 0);
    uk0 = 0;
    uk1 = nu;
    words4 = (size_t)2 * nu + 16;
    d_vals = 0;
    d_lut = (size_t)TIE_MAX_PACKED * 8;
    words5 = (size_t)TIE_MAX_PACKED * 8 + (size_t)TIE_MAX_PACKED * 64 + 64;
  }
};
struct QnScratch {  // slot 3 of the queryname sort, by the longest name
  size_t vwords, d_over, d_lut, lut_words, words3;  // d_vals at 0: maxq value sets and the NUL word; all in words
  explicit QnScratch(uint32_t maxq) : vwords((size_t)maxq * 8 + 1), d_over(vwords), d_lut(vwords + 1), lut_words(((size_t)maxq * 256 + 3) / 4), words3(vwords + 1 + lut_words) {}
};

// ---- rank tables.  A position's value set: 256 bits in eight words, bit v = byte value v occurs there.
inline int value_count(const uint32_t *set) {
  int cnt = 0;
  for (int w = 0; w < 8; w++) cnt += __builtin_popcount(set[w]);
  return cnt;
}
// row[v] = the rank of v among the values that occur (same order, fewer bits), 0 for the others; returns their number
inline int rank_row(const uint32_t *set, uint8_t *row /* 256 */) {
  int rank = 0;
  for (int v = 0; v < 256; v++) row[v] = ((set[v >> 5] >> (v & 31)) & 1u) ? (uint8_t)rank++ : (uint8_t)0;
  return rank;
}
inline int rank_bits(int nvalues) {  // (a single value gets one bit)
  int b = 1;
  while ((1 << b) < nvalues) b++;
  return b;
}
// the coordinate sort's live positions: the set bits of k_material_live's bitmap below m_bytes, ascending
inline std::vector<uint16_t> live_positions(const uint32_t *live, uint32_t m_bytes) {
  std::vector<uint16_t> lp;
  for (uint32_t j = 0; j < m_bytes; j++)
    if ((live[j >> 5] >> (j & 31)) & 1u) lp.push_back((uint16_t)j);
  return lp;
}
inline bool rank_keys_apply(size_t nlive) { return nlive != 0 && nlive <= (size_t)TIE_MAX_PACKED; }  // else the byte rounds

// The fields of a sort's keys, most significant first: field k is `pos[k]` (a byte position, or QN_STATE / QN_LEN), `bits[k]` wide,
// and a byte position's rank is lut[slot[k] * 256 + byte].
struct RankFields {
  std::vector<uint16_t> pos, slot;
  std::vector<int> bits;
  std::vector<uint8_t> lut;
  int n() const { return (int)pos.size(); }
  void add(uint16_t p, uint16_t s, int b) { pos.push_back(p); slot.push_back(s); bits.push_back(b); }
  void add_ranked(uint16_t p, const uint32_t *set) {
    const size_t s = lut.size() / 256;
    lut.resize((s + 1) * 256);
    add(p, (uint16_t)s, rank_bits(rank_row(set, lut.data() + s * 256)));
  }
};
// coordinate sort: every live position, from the value sets k_material_values collected (sets[k * 8 ..] for position lp[k])
inline RankFields tie_fields(const std::vector<uint16_t> &lp, const uint32_t *sets) {
  RankFields f;
  for (size_t k = 0; k < lp.size(); k++) f.add_ranked(lp[k], sets + k * 8);
  return f;
}
// queryname sort: the state (if any record is not output), the positions with more than one value, the length (if a name holds a NUL
// byte: sets[maxq * 8] != 0; lengths <= MAX_QNAME < 2^11)
inline RankFields qn_fields(const uint32_t *sets /* QnScratch::vwords */, uint32_t maxq, bool any_not_output) {
  RankFields f;
  if (any_not_output) f.add(QN_STATE, 0, 1);
  for (uint32_t p = 0; p < maxq; p++)
    if (value_count(sets + (size_t)p * 8) >= 2) f.add_ranked((uint16_t)p, sets + (size_t)p * 8);
  if (maxq > 0 && sets[(size_t)maxq * 8]) f.add(QN_LEN, 0, 11);
  return f;
}

// ---- packing: fields [lo, hi) as one key of `total` bits, lower fields in lower bits
struct FieldCut { int lo, hi, total; };
// the longest prefix of the fields that fits 64 bits beside `reserved` bits in front, 64 fields at most
inline FieldCut pack_prefix(const std::vector<int> &bits, int reserved) {
  int total = 0, hi = 0;
  while (hi < (int)bits.size() && hi < 64 && reserved + total + bits[hi] <= 64) total += bits[hi++];
  return FieldCut{0, hi, total};
}
// The coordinate sort's first round - run id and prefix in one key, the rest settled by comparison - is taken unless tie_rounds = 1.
// (The second condition is as the code always had it and can never be false: a run id has at most 27 bits, a rank at most 8.)
inline bool key_then_compare(int tie_rounds, int reserved, int first_bits) { return tie_rounds != 1 && reserved + first_bits <= 64; }
// stable LSD rounds over all fields, from the least significant up: each at most 64 bits and 64 fields
inline std::vector<FieldCut> lsd_cuts(const std::vector<int> &bits) {
  std::vector<FieldCut> cuts;
  for (int hi = (int)bits.size(); hi > 0;) {
    int total = 0, lo = hi;
    while (lo > 0 && total + bits[lo - 1] <= 64 && hi - lo < 64) { lo--; total += bits[lo]; }
    cuts.push_back(FieldCut{lo, hi, total});
    hi = lo;
  }
  return cuts;
}
// shift[k - lo] = the bit at which field k of the cut sits
inline void field_shifts(const std::vector<int> &bits, FieldCut cut, uint8_t *shift) {
  int sh = cut.total;
  for (int k = cut.lo; k < cut.hi; k++) {
    sh -= bits[k];
    shift[k - cut.lo] = (uint8_t)sh;
  }
}
inline int key_digits(int key_bits) { return (key_bits + 7) / 8; }  // radix passes of eight bits
// more than TIE_MAX_PACKED live positions: rounds on the bytes themselves, eight positions each, least significant first
inline std::vector<FieldCut> byte_cuts(size_t nlive) {
  std::vector<FieldCut> cuts;
  for (size_t hi = nlive; hi > 0;) {
    const size_t lo = hi >= 8 ? hi - 8 : 0;
    cuts.push_back(FieldCut{(int)lo, (int)hi, 8 * (int)(hi - lo)});
    hi = lo;
  }
  return cuts;
}

}  // namespace elp
