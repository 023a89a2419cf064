// apply_plan.hpp — ApplyBQSR's decisions as plain host arithmetic: which kernel takes a read set and with which row dictionary, how that
// dictionary and the one-length kernel's scratch are laid out, and what the launches look like.  Nothing here touches the device or includes
// HIP: the header compiles with the host compiler alone (tests/apply_plan_host.cpp, tests/test_apply_plan_cpu.py).  The kernels' static LDS
// comes in as arguments; each value is a constexpr defined beside its kernel's __shared__ declarations (apply_flat.hip, apply3.hip).
// elp_bqsr_apply (bqsr_apply.hip) and the upload's lut_uploaded (bqsr_lut.hip) both ask apply_plan: the conditions stand here only.
#pragma once
#include "bqsr_plan.hpp"

namespace elp {

constexpr int A3_ROW = 20;       // apply3.hip: bytes between two level-2 rows in LDS (17 used)
constexpr int A3_NT = 512;       // apply3.hip: threads of k_bqsr_apply3; three workgroups per CU around three copies of the LUT (~50 KB each): six waves per SIMD
constexpr int A3_MAXCOV = 256;   // apply3.hip: covariates the split's counts hold
constexpr int A3_RBLOCKS = 1024; // apply3.hip: workgroups of the split's two record passes at most
constexpr uint32_t LUT_T2_CAP = 3855;   // distinct rows one dictionary holds: 16-bit byte offsets
constexpr uint32_t LUT_PC_ROWS = 256;   // rows apart of two covariates' dictionaries (one dictionary per covariate)
constexpr size_t LUT_MAX_ROWS = (size_t)1 << 22;  // rows of the resident part a dictionary is built over at most

// ---- ApplyBQSR for read sets of one length (apply3.hip).  LDS of a launch: level 1 + room for 256 level-2 rows (their number is not read
// back in front of the launch); 1 = does not fit
inline int apply3_bytes(int n_cov, int n_qi, int lmax, size_t static_lds, size_t *dyn_out) {
  const size_t n1 = (size_t)n_cov * (size_t)(6 + n_qi + 1) * (size_t)(2 * lmax + 1);
  const size_t dyn = ((n1 + 15) & ~(size_t)15) + (size_t)256 * A3_ROW + 16;
  *dyn_out = dyn;
  return dyn + static_lds <= LDS_CU ? 0 : 1;
}

// ---- what the choice depends on
struct ApplyShape {
  uint64_t n;                       // staged reads
  int n_cov;                        // read-group covariates
  uint32_t max_l_seq, uniform_len;  // longest staged read; the one length of the staged reads, 0 = ragged
  int max_cycle;                    // --max-cycle
  int qlo, qhi;                     // the quality hint: smallest and largest sampled quality >= 6 (qhi = -1: none)
  int apply_kernel, apply_wgs, n_cu;  // elp_set_tuning (twice); CUs
  size_t lds_flat, lds_apply3, lds_apply3_split;  // APPLY_LDS (apply_flat.hip), APPLY3_LDS, APPLY3_LDS_SPLIT (apply3.hip)
};

// How apply3.hip (read sets of one length) takes a LUT: 0 not at all, 1 the level-1 tables of every covariate in one workgroup's LDS,
// 2 split by covariate (their level 1 does not fit - many read groups -, or elp_set_tuning "apply_kernel" = 3): a workgroup holds one
// covariate's tables at a time
inline int apply3_form(const ApplyShape &s, int n_qi, int lmax, size_t *dyn_out) {
  if (s.apply_kernel != 3 && apply3_bytes(s.n_cov, n_qi, lmax, s.lds_apply3, dyn_out) == 0) return 1;
  if (apply3_bytes(1, n_qi, lmax, s.lds_apply3, dyn_out) == 0) return 2;
  return 0;
}

// ---- everything elp_bqsr_apply knows in front of its first launch
struct ApplyPlan {
  int n_cov, max_cycle;  // (of the shape: what a dictionary built for this plan depends on besides the fields below)
  bool chk;              // a read can exceed --max-cycle: the kernel checks every cycle
  bool want3;            // the read set is one the one-length kernel takes
  int qlo, n_qi, lmax;   // the resident qualities [qlo, qlo + n_qi) (qlo = 6 under want3) and cycles [-lmax, lmax]
  size_t n_rows, n1;     // rows of the resident part; level-1 entries (one more row per covariate: "not resident")
  int a3; size_t dyn3;   // the first one-length form (apply3_form), with its dynamic LDS
  bool flat_lds_lut;     // the general kernel can hold a two-level LUT in LDS (how large its level 2 is shows when the dictionary is built)
};
inline ApplyPlan apply_plan(const ApplyShape &s) {
  ApplyPlan p{};
  p.n_cov = s.n_cov; p.max_cycle = s.max_cycle;
  p.lmax = (int)std::max<uint32_t>(s.max_l_seq, 1);
  p.chk = (int64_t)s.max_l_seq > (int64_t)s.max_cycle;
  // apply3.hip takes read sets of one length (elp_set_tuning "apply_kernel" = 1 forces k_bqsr_apply_flat: A/B measurements) and works in
  // whole 16-byte blocks; its level-1 table is resident from quality 6 on, whatever the smallest sampled quality was
  p.want3 = s.apply_kernel != 1 && !p.chk && s.uniform_len >= 16 && s.qhi >= 0;
  p.qlo = p.want3 ? 6 : s.qlo;
  p.n_qi = s.qhi - p.qlo + 1;
  const size_t w = 2 * (size_t)p.lmax + 1;
  p.n_rows = (size_t)s.n_cov * (size_t)std::max(p.n_qi, 0) * w;
  p.n1 = (size_t)s.n_cov * (size_t)(p.n_qi + 1) * w;
  const bool rows_ok = p.lmax <= s.max_cycle && p.n_rows < LUT_MAX_ROWS;
  p.a3 = (p.want3 && rows_ok) ? apply3_form(s, p.n_qi, p.lmax, &p.dyn3) : 0;
  p.flat_lds_lut = !p.chk && s.qhi >= 0 && rows_ok && p.n1 + s.lds_flat <= LDS_CU;
  return p;
}
// the form after form `a3` met more distinct rows than one-byte ids hold (error bit 512): one dictionary per covariate (a covariate's rows
// are the n_cov-th part) if one covariate's tables fit; else 0, the general kernel
inline int apply3_after_overflow(const ApplyShape &s, const ApplyPlan &p, int a3, size_t *dyn3) {
  return (a3 == 1 && s.n_cov > 1 && apply3_bytes(1, p.n_qi, p.lmax, s.lds_apply3, dyn3) == 0) ? 2 : 0;
}

// ---- the general kernel's launch (apply_flat.hip) once the number of distinct rows is known (NO_DICT: no dictionary was built).
// mode 1: one-byte ids, level-2 rows 32 bytes apart; mode 2: 16-bit byte offsets, rows 17 bytes apart; mode 0: the dense LUT in HBM / L2
constexpr uint32_t NO_DICT = 0xFFFFFFFFu;
struct FlatLaunch { int mode; size_t dyn; unsigned per_cu, grid; };
inline FlatLaunch flat_launch_plan(const ApplyShape &s, const ApplyPlan &p, uint32_t n_dict, uint64_t nsteps) {
  FlatLaunch f{0, 0, 8, 0};
  if (p.flat_lds_lut && n_dict < LUT_T2_CAP) {
    const int m = n_dict + 1 <= 256 ? 1 : 2;
    const size_t bytes = ((p.n1 * (size_t)m + 15) & ~(size_t)15) + (size_t)(n_dict + 1) * (m == 1 ? 32 : 17) + 16;
    if (bytes + s.lds_flat <= LDS_CU) {
      f.mode = m; f.dyn = bytes;
      f.per_cu = (unsigned)std::max<size_t>(1, std::min<size_t>(3, LDS_CU / (bytes + s.lds_flat)));
    }
  }
  f.grid = (unsigned)std::min<uint64_t>(nsteps, (uint64_t)s.n_cu * f.per_cu);
  return f;
}

// ---- the row dictionary's block of 32-bit words (bqsr_lut.hip): counter | slots | slot_id | row_slot | t1 | t2
//   counter   [256] distinct rows (per covariate with one dictionary each); own words: the err_flag mailbox other stages use is not touched
//             from the upload thread
//   slots     [n_slots] open-addressing table of row indices, a power of two >= 2 n_rows
//   slot_id   [n_slots] dense id of an occupied slot
//   row_slot  [n_rows] the slot of a row
//   t1        [n1] 16-bit ids, level 1
//   t2        17-byte rows, level 2: LUT_T2_CAP + 1 of one dictionary, or LUT_PC_ROWS per covariate
struct LutDictLayout {
  uint32_t n_slots;
  size_t n_rows, n1, t2_bytes, words;
  size_t counter, slots, slot_id, row_slot, t1, t2;  // word offsets
  LutDictLayout(int n_cov, int n_qi, int lmax) {
    const size_t w = 2 * (size_t)lmax + 1;
    n_rows = (size_t)n_cov * (size_t)std::max(n_qi, 0) * w;
    n1 = (size_t)n_cov * (size_t)(n_qi + 1) * w;
    for (n_slots = 1024; n_slots < 2 * n_rows;) n_slots <<= 1;
    t2_bytes = std::max<size_t>((size_t)(LUT_T2_CAP + 1) * 17, (size_t)n_cov * LUT_PC_ROWS * 17);
    counter = 0; slots = 256; slot_id = slots + n_slots; row_slot = slot_id + n_slots;
    t1 = row_slot + n_rows; t2 = t1 + ((n1 + 1) >> 1);
    words = 256 + (size_t)2 * n_slots + n_rows + n1 + t2_bytes / 4 + 64 + 16;
  }
};

// ---- the dictionary built ahead of the call (behind the LUT's upload): what it was built for.  form: 0 none, 1 one dictionary, 2 one per covariate
struct LutDictBuilt {
  int form = 0, qlo = 0, n_qi = 0, lmax = 0, max_cycle = 0, n_cov = 0;
  static LutDictBuilt of(const ApplyPlan &p) { return LutDictBuilt{p.a3, p.qlo, p.n_qi, p.lmax, p.max_cycle, p.n_cov}; }
  // it is the one this plan starts from (never if the LUT came with the call: the dictionary is of the uploaded LUT)
  bool serves(const ApplyPlan &p, bool lut_in_call) const {
    return !lut_in_call && form != 0 && form == p.a3 && qlo == p.qlo && n_qi == p.n_qi && lmax == p.lmax && max_cycle == p.max_cycle && n_cov == p.n_cov;
  }
};

// ---- the one-length kernel's launch (apply3.hip) and its scratch (slot 5): records | dump | staging indices | cw | per-workgroup counts
//   records   8 bytes per staged read
//   dump      16 bytes per lane of the launch: where lanes without a block store
//   ridx      (split) the staging index of a record
//   cw        (split) [256] counts per covariate | [257] offsets | [256] cursors
//   blk       (split) [A3_RBLOCKS][256] the record passes' counts per workgroup
struct Apply3Launch {
  uint32_t group, rpi;  // lanes that share reads: A3_NT (reads packed over the whole workgroup) or 64 (whole reads per wave); reads per trip
  unsigned per_cu;
  int grid;
  size_t recs, dump, ridx, cw, blk, size8;  // byte offsets (ridx, cw, blk: used with `split` only); the slot's size in 8-byte units
  Apply3Launch(uint64_t n, uint32_t len, int n_cu, size_t dyn, bool split, int apply_wgs, size_t lds_apply3, size_t lds_apply3_split) {
    const uint32_t bpr = (len + 15u) >> 4;
    // reads packed over the whole workgroup unless that puts the last two blocks of some read (which overlap when the length is not a
    // multiple of 16) into different waves: then whole reads per wave
    group = A3_NT;
    if ((len & 15u) && bpr > 1)
      for (uint32_t slot = 0; slot < A3_NT / bpr; slot++)
        if (((slot * bpr + bpr - 1u) & 63u) == 0) group = 64;
    rpi = (group / bpr) * (A3_NT / group);
    per_cu = (unsigned)std::max<size_t>(1, std::min<size_t>(3, LDS_CU / (dyn + lds_apply3 + (split ? lds_apply3_split : 0))));
    if (apply_wgs >= 1 && apply_wgs <= 3) per_cu = std::min(per_cu, (unsigned)apply_wgs);
    grid = (int)std::min<uint64_t>((n + rpi - 1) / rpi, (uint64_t)n_cu * per_cu);
    const size_t rec8 = (size_t)((n + 4 + 1) & ~(uint64_t)1), dump8 = (size_t)grid * A3_NT * 2;
    recs = 0; dump = rec8 * 8; ridx = dump + dump8 * 8;
    cw = ridx + (size_t)((n + 1) & ~(uint64_t)1) * 4;
    blk = cw + (3 * A3_MAXCOV + 8) * 4;
    size8 = rec8 + dump8 + (split ? (size_t)((n + 1) / 2) + 2 * A3_MAXCOV + 8 + (size_t)A3_RBLOCKS * A3_MAXCOV / 2 : 0) + 8;
  }
};

}  // namespace elp
