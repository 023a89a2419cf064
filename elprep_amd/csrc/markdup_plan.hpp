// markdup_plan.hpp — mark duplicates' launch plan as plain host arithmetic: every size, scratch offset and grid that the record count
// fixes for a call of elp_mark_duplicates, the tables sized by what it reads back, and which of its paths the mates take.  Nothing here touches the device or includes HIP: the header compiles
// with the host compiler alone (tests/markdup_plan_host.cpp, tests/test_markdup_plan_cpu.py).  markdup.hip's phases take their sizes
// and offsets from here and compute none themselves.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace elp {

// ---- sizes the plan shares with the kernels (markdup.hip describes each beside its kernel)
constexpr int MP_R = 1;                         // k_mate_pairs: records per thread
constexpr int PL_TILES = 8;                     // k_pair_list_*: 256-record tiles per workgroup
constexpr int PB_THREADS = 256;                 // k_pair_bucket
constexpr int PB_TARGET = 384;                  // the pair list is partitioned until a bucket holds at most this many entries on average
constexpr int PB_CAP = 1024;                    // k_pair_bucket's table slots in LDS
constexpr int FLI_CHUNK = 2048;                 // k_frag_list: records per round of a workgroup
constexpr int MF_THREADS = 320, MF_RECS = 312;  // k_md_front: five waves cover 312 records

inline unsigned md_blocks(uint64_t n, unsigned per_block) { return (unsigned)((n + per_block - 1) / per_block); }

// slots of an open-addressing table of record indices that holds n of them at most half full: a power of two, 1024 at least
inline uint64_t table_size_for(uint64_t n) {
  uint64_t t = 1024;
  while (t < 2 * n + 16) t <<= 1;
  return t;
}

// ---- everything the record count fixes
struct MdSizes {
  uint64_t n, T;           // records; the mate table's slots
  int bbits, ndig, sbits;  // the pair list (at most n / 2 pairs) is partitioned by bbits hash bits, in ndig radix passes over sbits = 8 ndig bits;
  size_t nb;               // nb = 2^bbits buckets.  ndig == 0: one bucket, whose bounds k_pair_bounds writes; else the last radix pass reports them
  uint64_t bw;             // Bloom filter words: ~2 bits per record, at most 4 MiB (what one XCD's L2 holds)
  uint32_t tab_cap;        // a list of k_mate_pairs' deferred inserts: its share of the workgroups x their records (64 lists)
  uint64_t npmax;          // pair entries and holes, whatever the mates' order turns out to be
  uint32_t nfx;            // the neighbour pairs' fixed slots: record i's entry goes to slot i >> 1
  // workgroups: of 256 records, of k_frag_list (before the cap by CUs), k_md_front, k_mate_pairs, k_bloom_coarse, k_pair_list_table, k_pair_bounds
  unsigned grid, frag_list_blocks, front_grid, mate_grid, coarse_grid, list_grid, bounds_grid;
  explicit MdSizes(uint64_t records) : n(records), T(table_size_for(records)), bbits(0), bw(1024), npmax(records + 2), nfx((uint32_t)((records + 1) / 2)) {
    while (bbits < 24 && ((n / 2 + 1) >> bbits) > (uint64_t)PB_TARGET) bbits++;
    ndig = (bbits + 7) / 8;
    sbits = 8 * ndig;
    nb = (size_t)1 << bbits;
    while (bw < n / 16 && bw < (1u << 20)) bw <<= 1;
    grid = md_blocks(n, 256);
    frag_list_blocks = md_blocks(n, FLI_CHUNK);
    front_grid = md_blocks(n, MF_RECS);
    mate_grid = md_blocks(n, 256 * MP_R);
    coarse_grid = md_blocks(bw / 16, 256);
    list_grid = md_blocks(n, 256 * PL_TILES);
    bounds_grid = md_blocks(npmax, 256);
    tab_cap = (uint32_t)((mate_grid + 63) / 64) * 256u * MP_R;
  }
  unsigned frag_list_grid(int n_cu) const { return std::min<unsigned>(frag_list_blocks, (unsigned)n_cu * 8); }  // a few persistent workgroups
};

// ---- the scratch blocks.  Who owns a slot of elp_ctx::scratch in which phase of a call (front -> fragments -> mates -> big groups -> pairs):
//   slot 0  table     T words                   the mate table: mates (its first Tm slots; refilled for the overflow retry)
//   slot 1  rep | flist, 2 n + 16 words         front .. fragments: every true fragment's representative, the list of true fragments
//           bounds, 2 nb + 8 words              pairs: the buckets' first and last entries (2 nb + 8 <= 2 n + 16 for every n: no reallocation)
//   slot 2  best      n + 16 x 8 bytes          front .. fragments: a fragment group's best score, bit 63 = a true pair has the key
//           bk        2 n + 8 x 8 bytes         big groups: the members' sort keys and the sort's second buffer
//   slot 3  winner    n + 16 words              front .. fragments: a fragment group's winner
//           bv        2 n + 8 words             big groups: the members and the sort's second buffer
//   slot 5  fkey      n + 8 x 16 bytes          front .. pairs: every record's fragment key
//   slot 6  bloom | coarse | hash32 | code | tab_list | hash_lo    front .. pairs (code, tab_list), the others front .. mates
//   slot 7  pk | pv | ftable | fbits            sized when the number of true fragments is back: ftable, fbits front; pk, pv front .. pairs
// Slots are grow-only and every size above is taken before the slot's first kernel of the call, with one exception: the big-groups
// phase (keys with more than two records: rare) asks slots 2 and 3 for 2 n + 8 elements where the front pass asked for n + 16, so the
// first such call on a context reallocates them in mid-call - `best` and `winner` are dead by then.
// Offsets are 32-bit words from the slot's start.  (ftable = word 6 npmax is 16-byte aligned for even n only, and k_frag_bits loads it
// 16 bytes at a time: as it was; moving it is a change of its own.)
struct MdScratch {
  size_t table, best, winner, fkey, big;  // elements of slots 0, 2, 3, 5; of slots 2 and 3 in the big-groups phase
  size_t flist, words1, bounds_words;     // slot 1: rep [0, n) | flist [n + 8, 2 n + 8); later first entries [0, nb) | last entries [nb, 2 nb)
  size_t coarse, hash32, code, tab_list, hash_lo, words6;  // slot 6, bloom at 0; `code` holds n bytes from word `code` on
  uint64_t npmax;
  explicit MdScratch(const MdSizes &s) : npmax(s.npmax) {
    const size_t n = (size_t)s.n;
    table = (size_t)s.T;
    best = winner = n + 16;
    fkey = n + 8;
    big = 2 * n + 8;
    flist = n + 8;
    words1 = flist + n + 8;
    bounds_words = 2 * s.nb + 8;
    coarse = (size_t)s.bw;                            // one bit per 16 words of the filter
    hash32 = coarse + (size_t)s.bw / 512 + 16;        // the high half of the key hashes
    code = hash32 + n + 8;
    tab_list = code + 8 + (n + 16) / 4;               // k_mate_pairs' deferred table inserts (aligner order): 64 lists of tab_cap
    hash_lo = tab_list + 64 * (size_t)s.tab_cap + 8;  // the low half of the key hashes
    words6 = hash_lo + 8 + n + 16;
  }
  // slot 7, for a fragment table of Tf slots: pk [0, 2 npmax) in 64-bit words (the pair list and the sort's second buffer), then
  // pv [4 npmax, 6 npmax) | ftable, Tf words | fbits, Tf / 32 words
  struct Pairs { size_t pv, ftable, fbits, words64; };  // words64: the slot's size in 64-bit words
  Pairs pairs(uint64_t Tf) const {
    const size_t pv = 4 * (size_t)npmax, ftable = pv + 2 * (size_t)npmax, fbits = ftable + (size_t)Tf;
    return Pairs{pv, ftable, fbits, (fbits + (size_t)Tf / 32 + 64) / 2 + 8};
  }
};

// ---- the fragments' table, sized when the number of true fragments is back.  Sparse: most look-ups of the pairs end at an empty slot
inline uint64_t frag_table_size(uint32_t nf, uint64_t T) { return nf ? std::min<uint64_t>(T, table_size_for(4ull * nf)) : 0; }

// ---- the mates' path, decided when the number n_tab of records that are not exactly-two-neighbours is back.
//   fixed   aligner order (few candidates need a table; mate_path = 0): the neighbour pairs' entries go to nfixed fixed slots, the table's
//           pairs behind them, and the table only has to hold the n_tab records plus the neighbour pairs a Bloom-filter hit sends there
//           (at most as many again, in practice a fraction): it is sized by their number, not by n.  n < 8 is never fixed (n / 8 = 0).
//   fast    fixed and nobody announced a key: the front pass's neighbour pairs stand, no mate kernel runs and nothing goes through the
//           table, so the pair phase lists nothing either.  (That phase used to ask for "fast and no key with more than two records";
//           only the mate kernels find such keys and they do not run when fast holds, so the two were one predicate.)
//   listed  fixed with a few records on the table path: their inserts are listed and made by a dense pass; list_n bounds the lists'
//           members (the records the front pass counted plus the neighbour pairs a filter hit sent along)
//   else    coordinate-ordered or shuffled input, or mate_path = 2: every candidate goes through the full table.
struct MatePlan {
  bool fixed, fast, listed;
  uint64_t nfixed, Tm, list_n;  // Tm: the table's slots at the first attempt (an overflow repeats it with all T)
};
inline MatePlan mate_plan(uint64_t n, uint32_t n_tab, int mate_path, uint64_t T) {
  const bool fixed = (uint64_t)n_tab < n / 8 && mate_path == 0;
  return MatePlan{fixed, fixed && n_tab == 0, fixed && n_tab != 0, fixed ? (n + 1) / 2 : 0,
                  fixed ? std::min<uint64_t>(T, table_size_for(std::min<uint64_t>(n, 4ull * n_tab + 1024))) : T, std::min<uint64_t>(n, 2ull * n_tab + 4096)};
}

}  // namespace elp
