// bqsr_apply.hip — ApplyBQSR on the HBM column store: the LUT's way to the device, the row dictionary of its resident part, and the general
// apply kernel (any read lengths; apply3.hip takes read sets of one length).
//
// Reference: BaseRecalibratorTables.ApplyBQSR (filters/bqsr.go:936-1005); the covariates' device helpers are in bqsr_dev.hpp.
//
//   k_bqsr_apply_flat   flat stream over QUAL/SEQ (flat.hpp), one lane per 16 bases, QUAL rewritten in place.  MODE 0: a byte gather per
//                       base from the dense LUT in HBM / L2; MODE 1, 2: from a two-level LUT in LDS (ids of distinct rows | the rows)
//   k_lut_rows_*        the distinct 17-byte rows of the resident part of the dense LUT (LutDict: one dictionary, or one per covariate)
//   k_lut_expand_rows   the dense LUT from its rows form (elp_bqsr_lut_upload_rows)
//   elp_bqsr_lut_upload, elp_bqsr_lut_upload_rows   the LUT ahead of the apply call, on the copy stream; lut_uploaded builds the dictionary
//                       behind it when the facts it depends on are known
//   elp_bqsr_apply      apply3.hip where it applies (one dictionary, then one per covariate), else k_bqsr_apply_flat
#include "bqsr_common.hpp"

namespace elp {

struct ApDesc { uint16_t left, right, len; uint8_t cov; uint8_t fl; };  // fl: BQ_ELIGIBLE recalibrate, BQ_REVERSED, BQ_LAST
static_assert(sizeof(ApDesc) == 8, "ApDesc is staged as one 8-byte word");

struct ApplyArgs {
  uint64_t n, qual_bytes;
  const uint64_t *qual_off, *seq_off;
  uint8_t *qual;
  const uint8_t *seq4;
  // per-read facts the stage step turns into the 8-byte descriptor (there is no prologue kernel and no descriptor column any more)
  const uint16_t *flag, *rgid, *rg_cov;
  const uint32_t *l_seq;
  const uint64_t *qbounds;
  const uint8_t *cov_present;
  const uint32_t *tile_first;
  const uint8_t *lut;  // [n_cov][94][2*max_cycle+1][17]
  int max_cycle;
  uint32_t *err;
  // LDS-resident two-level LUT (MODE 1 / 2): t1 [n_cov][n_qi + 1][2*lmax+1] ids of distinct 17-byte LUT rows (qi = quality - qlo;
  // row n_qi = "not resident"), t2 [n_dict + 1][17] the rows themselves (row n_dict = 0x80 everywhere)
  const uint16_t *t1;
  const uint8_t *t2;
  int n_cov, n_qi, qlo, lmax, n_dict;
};

// ApplyBQSR (bqsr.go:936-1005): every base with quality >= 6 of a record with a known read group is replaced by the LUT value
// of (read group, quality, cycle, context); cycle and context are taken on the full, unclipped read.
//
// MODE 0: one byte gather per base from the dense LUT in HBM / L2.
// MODE 1, 2: two-level LUT in LDS.  The dense LUT is a table of 17-byte rows (one per (read group, quality, cycle); 16 contexts +
// "no context"), and few of them are distinct: estimateHierarchicalBayesianQuality (bqsr.go:901-919) adds the cycle entry's and
// the context entry's integer empirical qualities to a prior that depends on (read group, quality) only, so a row is determined by
// (read group, quality, empirical quality of the cycle entry).  Level 1 maps (read group, quality in [qlo, qhi], cycle) to a row id
// (MODE 1: one byte, at most 255 rows, level 2 rows 32 bytes apart; MODE 2: the row's byte offset in 16 bits), level 2 holds the
// distinct rows.  A few tens of KB instead of the 143 KB of the rows spelled out, so three workgroups share a CU (one before), and
// ~40 distinct qualities x 4 read groups still fit (the spelled-out table did not: HBM gathers).  Qualities below qlo read row qlo
// (they are < 6 and put back by a byte mask), qualities above qhi read the "not resident" row: bit 7 of the result sends them to
// the rolled fix-up loop (dense LUT, or the error for qualities > 93).
template <bool CHECK_CYCLE, int MODE>
struct ApplyBody {
  // 128 KiB steps in groups of up to 512 reads (12 B of LDS per read)
  static constexpr int NT = FL_THREADS, TILES = 4, RMAX = 512;
  static constexpr bool TILE_ENDS = false;
  static constexpr int ES = MODE == 1 ? 1 : 2;  // bytes per level-1 entry
  const uint64_t *__restrict__ seq_off;
  const uint64_t *__restrict__ qual_off;
  uint8_t *__restrict__ qual;
  const uint8_t *__restrict__ seq4;
  const uint16_t *__restrict__ flag;
  const uint16_t *__restrict__ rgid;
  const uint16_t *__restrict__ rg_cov;
  const uint32_t *__restrict__ l_seq;
  const uint64_t *__restrict__ qbounds;
  const uint8_t *__restrict__ cov_present;
  const uint8_t *__restrict__ lut;
  int max_cycle;
  uint64_t *s_desc;
  uint32_t *s_seq;
  uint32_t t1_at, t2_at;  // LDS byte addresses of the two levels (MODE != 0); t1_at already has qlo's rows subtracted
  int lmax, rows_w;       // rows_w = (n_qi + 1) * (2 * lmax + 1): level-1 entries per read group
  uint32_t w_es;          // (2 * lmax + 1) * ES
  uint32_t qlo, qhi1;     // resident quality range [qlo, qhi1 - 1]; qhi1 reads the "not resident" row
  uint64_t seq_base;
  uint32_t err;
  Chunk out;              // the block processed last: stored by retire()
  uint64_t out_at;
  int out_nb;

  // the read's descriptor {left, right, len, cov, flags} (ApDesc) straight from the columns: which reads ApplyBQSR touches
  // (bqsr.go:947-958) and the low-quality-tail bounds of computeStrandedClippedSeq (:316-332) that adapt_score left per read
  __device__ __forceinline__ void stage(uint32_t g0, uint32_t ng) {
    seq_base = seq_off[g0];
    for (uint32_t k = threadIdx.x; k < ng; k += NT) {
      const uint64_t i = (uint64_t)g0 + k;
      // all column loads first (one memory latency instead of one per test)
      const uint16_t rg = rgid[i], f = flag[i];
      const int len = (int)l_seq[i];
      const uint64_t q0 = qual_off[i], q1 = qual_off[i + 1], qb = qbounds[i], so = seq_off[i];
      uint64_t d = 0;
      if (rg == ELP_NIL16) err |= 32u;                               // readGroupCovariate panics, bqsr.go:38
      else {
        const uint32_t cov = rg_cov[rg];
        if (cov_present[cov]) {                                      // else: read group absent from the tables, read untouched (:953-955)
          if ((uint64_t)len != q1 - q0) err |= 64u;
          else if (len > MAX_DESC_READ) err |= 2u;
          else {
            const uint32_t hi1 = (uint32_t)qb;
            const int left = hi1 ? (int)(qb >> 32) : len, right = hi1 ? (int)hi1 - 1 : len - 1;
            const uint32_t fl = BQ_ELIGIBLE | ((f & F_REVERSED) ? BQ_REVERSED : 0) | ((f & F_LAST) ? BQ_LAST : 0);
            d = (uint64_t)(uint16_t)left | ((uint64_t)(uint16_t)(right < 0 ? 0xFFFF : right) << 16) | ((uint64_t)(uint16_t)len << 32) | ((uint64_t)(cov & 0xFFu) << 48) |
                ((uint64_t)fl << 56);
          }
        }
      }
      s_desc[k] = d;
      s_seq[k] = (uint32_t)(so - seq_base);
    }
  }
  // dense LUT in HBM/L2: one byte gather per base
  template <int I>
  __device__ __forceinline__ uint32_t base(const Chunk &ch, int nb, uint32_t vw, uint32_t cw, uint32_t Q, int st, int cyc0, int ci, uint32_t qstride) {
    constexpr int sh = 4 * (I & 7);
    const uint32_t q = ch.get<I>();
    bool act = I < nb && q >= 6u;
    err |= (act && q >= (uint32_t)ELP_NQUAL) ? 8u : 0u;
    act = act && q < (uint32_t)ELP_NQUAL;
    if (CHECK_CYCLE) {
      const int cyc = cyc0 + I * ci;
      const bool out = act && (cyc > max_cycle || cyc < -max_cycle);
      err |= out ? 16u : 0u;
      act = act && !out;
    }
    const uint32_t cx = ((cw >> sh) & 15u) | ((((~vw) >> sh) & 1u) << 4);  // 16 = no context
    const uint32_t idx = Q + (uint32_t)(I * st) + q * qstride + cx;
    const uint32_t v = lut[act ? idx : 0u];
    return act ? v : q;
  }
  // two-level LUT in LDS: two dependent LDS reads per base, no select.  bpi = level-1 address of (read group, quality 0 + qlo
  // folded in, cycle of base I); cxw: context index (0..15, 16 = none) of four bases, one byte each.  Bases past the read's end
  // are looked up too (their bytes are never stored), qualities < 6 are put back by a byte-mask select over the result words.
  template <int I>
  __device__ __forceinline__ uint32_t base_lds(const Chunk &ch, uint32_t cxw, uint32_t bp, int ci_es) {
    constexpr int bs = 8 * ((I & 7) >> 1);
    uint32_t qc;
    const uint32_t q = ch.get<I>();
    asm("v_med3_u32 %0, %1, %2, %3" : "=v"(qc) : "v"(q), "v"(qlo), "v"(qhi1));
    const uint32_t a1 = __umul24(qc, w_es) + (bp + (uint32_t)(I * ci_es));
    uint32_t id;
    if (MODE == 1) id = *reinterpret_cast<const __attribute__((address_space(3))) uint8_t *>((uintptr_t)a1);
    else id = *reinterpret_cast<const __attribute__((address_space(3))) uint16_t *>((uintptr_t)a1);
    const uint32_t cx = t2_at + ((cxw >> bs) & 0xFFu);
    const uint32_t a2 = MODE == 1 ? lshl_add_u32<5>(id, cx) : id + cx;
    return *reinterpret_cast<const __attribute__((address_space(3))) uint8_t *>((uintptr_t)a2);
  }
  // word of result bytes where the original quality is >= 6, original bytes elsewhere (ApplyBQSR leaves qualities < 6 alone)
  __device__ __forceinline__ static uint32_t keep_low(uint32_t orig, uint32_t res) {
    const uint32_t t = ((orig | 0x80808080u) - 0x06060606u) & 0x80808080u;  // bit 7 of a byte: (quality & 127) >= 6
    const uint32_t m = (t - (t >> 7)) | t;
    return (res & m) | (orig & ~m);
  }
  // bases of a block whose lookup hit the 0x80 row (bases past nb may have raised the flag falsely): quality > 93 -> error;
  // quality above the resident range -> dense LUT.  Rolled loop over the original bytes.
  __device__ __forceinline__ void fixup(Chunk &ch, const Chunk &orig, int nb, uint64_t CV, uint64_t CX, uint32_t Q, int st, int cyc0, int ci) {
    uint64_t lo = (uint64_t)ch.w0 | ((uint64_t)ch.w1 << 32), hi = (uint64_t)ch.w2 | ((uint64_t)ch.w3 << 32);
    const uint64_t olo = (uint64_t)orig.w0 | ((uint64_t)orig.w1 << 32), ohi = (uint64_t)orig.w2 | ((uint64_t)orig.w3 << 32);
    const uint32_t qstride = (uint32_t)(2 * max_cycle + 1) * 17u;
#pragma unroll 1
    for (int i = 0; i < nb; i++) {
      const int bs = 8 * (i & 7);
      const uint32_t q = (uint32_t)(((i & 8) ? ohi : olo) >> bs) & 0xFFu;
      if (q < 6u) continue;                                      // put back by keep_low
      uint64_t v = q;
      if (q >= (uint32_t)ELP_NQUAL) err |= 8u;
      else if (q < qhi1) continue;                               // resident: done by the straight-line code
      else {
        if (CHECK_CYCLE) {
          const int cyc = cyc0 + i * ci;
          if (cyc > max_cycle || cyc < -max_cycle) { err |= 16u; continue; }
        }
        const uint32_t cx = ((uint32_t)(CX >> (4 * i)) & 15u) | ((((uint32_t)(~CV >> (4 * i))) & 1u) << 4);
        v = (uint64_t)lut[Q + (uint32_t)(i * st) + q * qstride + cx];
      }
      const uint64_t m = ~(0xFFull << bs);
      lo = (i & 8) ? lo : ((lo & m) | (v << bs));
      hi = (i & 8) ? ((hi & m) | (v << bs)) : hi;
    }
    ch.w0 = (uint32_t)lo; ch.w1 = (uint32_t)(lo >> 32); ch.w2 = (uint32_t)hi; ch.w3 = (uint32_t)(hi >> 32);
  }

  struct Pre {
    Chunk ch;
    uint64_t v0, v1;  // SEQ window
    uint64_t qpos;
    uint32_t rl;
    int k0, nb;
  };
  __device__ __forceinline__ bool prefetch(uint32_t rl, int k0, int nb, uint64_t qpos, uint32_t, Pre &p) {
    const uint32_t fl = (uint32_t)(s_desc[rl] >> 56);
    if (!(fl & BQ_ELIGIBLE)) return false;
    p.rl = rl; p.k0 = k0; p.nb = nb; p.qpos = qpos;
    p.ch.load(qual + qpos);
    seq_load(seq4 + seq_base + s_seq[rl], k0, p.v0, p.v1);
    return true;
  }
  __device__ __forceinline__ void process(Pre &p) {
    const uint32_t rl = p.rl;
    const int k0 = p.k0, nb = p.nb;
    const uint64_t qpos = p.qpos;
    const uint64_t dw = s_desc[rl];
    const uint32_t fl = (uint32_t)(dw >> 56);
    const int left = (int)(dw & 0xFFFFu), right = ((dw >> 16) & 0xFFFFu) == 0xFFFFu ? -1 : (int)((dw >> 16) & 0xFFFFu);
    const int len = (int)((dw >> 32) & 0xFFFFu);
    const uint32_t cov = (uint32_t)(dw >> 48) & 0xFFu;
    const bool rev = fl & BQ_REVERSED;
    Chunk ch = p.ch;
    uint64_t S, N;
    seq_unpack(p.v0, p.v1, k0, rev, S, N);
    uint64_t ohS, cS, ohN, cN;
    nib_classify(S, ohS, cS);
    nib_classify(N, ohN, cN);
    const int cl = left + (rev ? 0 : 1), cr = right - (rev ? 1 : 0);
    int rhi = cr - k0 + 1;
    rhi = rhi < nb ? rhi : nb;
    const uint64_t CV = ohS & ohN & nib_range_clamped(cl - k0, rhi);
    const uint64_t CX = ((cN | (cS << 2)) ^ (rev ? NIBF : 0ull)) & nib_fill(CV);
    const int rof = (fl & BQ_LAST) ? -1 : 1;
    const int cf = rof + (rev ? (len - 1) * rof : 0), ci = rev ? -rof : rof;
    const int cyc0 = cf + k0 * ci, st = 17 * ci;
    const int ncyc = 2 * max_cycle + 1;
    const uint32_t Q = (uint32_t)((int)cov * ELP_NQUAL * ncyc * 17 + (cyc0 + max_cycle) * 17);
    const uint32_t v0 = (uint32_t)CV, v1 = (uint32_t)(CV >> 32), c0 = (uint32_t)CX, c1 = (uint32_t)(CX >> 32);
    uint32_t b0, b1, b2, b3, b4, b5, b6, b7, b8, b9, b10, b11, b12, b13, b14, b15;
    const Chunk orig = ch;
    if (MODE) {
      const uint32_t bp = t1_at + (uint32_t)((int)cov * rows_w + (cyc0 + lmax)) * (uint32_t)ES;
      const int ci_es = ci * ES;
      // context index per base, one byte each: even bases in ce, odd bases in co
      constexpr uint64_t EVN = 0x0F0F0F0F0F0F0F0Full;
      const uint64_t NV = ~CV & NIB1;
      const uint64_t ce = (CX & EVN) | ((NV & (NIB1 & EVN)) << 4), co = ((CX >> 4) & EVN) | (NV & (NIB1 & ~EVN));
      const uint32_t e0 = (uint32_t)ce, e1 = (uint32_t)(ce >> 32), d0 = (uint32_t)co, d1 = (uint32_t)(co >> 32);
      b0 = base_lds<0>(ch, e0, bp, ci_es); b1 = base_lds<1>(ch, d0, bp, ci_es); b2 = base_lds<2>(ch, e0, bp, ci_es); b3 = base_lds<3>(ch, d0, bp, ci_es);
      b4 = base_lds<4>(ch, e0, bp, ci_es); b5 = base_lds<5>(ch, d0, bp, ci_es); b6 = base_lds<6>(ch, e0, bp, ci_es); b7 = base_lds<7>(ch, d0, bp, ci_es);
      b8 = base_lds<8>(ch, e1, bp, ci_es); b9 = base_lds<9>(ch, d1, bp, ci_es); b10 = base_lds<10>(ch, e1, bp, ci_es); b11 = base_lds<11>(ch, d1, bp, ci_es);
      b12 = base_lds<12>(ch, e1, bp, ci_es); b13 = base_lds<13>(ch, d1, bp, ci_es); b14 = base_lds<14>(ch, e1, bp, ci_es); b15 = base_lds<15>(ch, d1, bp, ci_es);
    } else {
      const uint32_t qstride = (uint32_t)ncyc * 17u;
      b0 = base<0>(ch, nb, v0, c0, Q, st, cyc0, ci, qstride); b1 = base<1>(ch, nb, v0, c0, Q, st, cyc0, ci, qstride);
      b2 = base<2>(ch, nb, v0, c0, Q, st, cyc0, ci, qstride); b3 = base<3>(ch, nb, v0, c0, Q, st, cyc0, ci, qstride);
      b4 = base<4>(ch, nb, v0, c0, Q, st, cyc0, ci, qstride); b5 = base<5>(ch, nb, v0, c0, Q, st, cyc0, ci, qstride);
      b6 = base<6>(ch, nb, v0, c0, Q, st, cyc0, ci, qstride); b7 = base<7>(ch, nb, v0, c0, Q, st, cyc0, ci, qstride);
      b8 = base<8>(ch, nb, v1, c1, Q, st, cyc0, ci, qstride); b9 = base<9>(ch, nb, v1, c1, Q, st, cyc0, ci, qstride);
      b10 = base<10>(ch, nb, v1, c1, Q, st, cyc0, ci, qstride); b11 = base<11>(ch, nb, v1, c1, Q, st, cyc0, ci, qstride);
      b12 = base<12>(ch, nb, v1, c1, Q, st, cyc0, ci, qstride); b13 = base<13>(ch, nb, v1, c1, Q, st, cyc0, ci, qstride);
      b14 = base<14>(ch, nb, v1, c1, Q, st, cyc0, ci, qstride); b15 = base<15>(ch, nb, v1, c1, Q, st, cyc0, ci, qstride);
    }
    ch.w0 = b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
    ch.w1 = b4 | (b5 << 8) | (b6 << 16) | (b7 << 24);
    ch.w2 = b8 | (b9 << 8) | (b10 << 16) | (b11 << 24);
    ch.w3 = b12 | (b13 << 8) | (b14 << 16) | (b15 << 24);
    if (MODE) {
      const uint32_t any = (ch.w0 | ch.w1) | (ch.w2 | ch.w3);
      ch.w0 = keep_low(orig.w0, ch.w0); ch.w1 = keep_low(orig.w1, ch.w1); ch.w2 = keep_low(orig.w2, ch.w2); ch.w3 = keep_low(orig.w3, ch.w3);
      if (any & 0x80808080u) fixup(ch, orig, nb, CV, CX, Q, st, cyc0, ci);
    }
    out = ch; out_at = qpos; out_nb = nb;
  }
  __device__ __forceinline__ void slots(uint32_t) {}
  __device__ __forceinline__ void retire() {
    if (out_nb) out.store(qual + out_at, out_nb);
    out_nb = 0;
  }
  __device__ __forceinline__ void group_end(uint32_t, uint32_t) {}
  __device__ __forceinline__ void tile_end(uint32_t, uint64_t) {}
};

// The static LDS elp_bqsr_apply sets aside for k_bqsr_apply_flat: the kernel's __shared__ arrays, term by term (the kernel asserts the sum
// against its own declarations), and a margin.
constexpr int APPLY_RMAX = ApplyBody<false, 1>::RMAX;
constexpr size_t APPLY_LDS_ARRAYS = sizeof(FlatLds<APPLY_RMAX>) + sizeof(uint64_t[APPLY_RMAX]) + sizeof(uint32_t[APPLY_RMAX]);
constexpr size_t APPLY_LDS = APPLY_LDS_ARRAYS + 512;
static_assert(APPLY_LDS == sizeof(FlatLds<APPLY_RMAX>) + (size_t)APPLY_RMAX * 12 + 512, "the budget the plan was written around");

template <bool CHECK_CYCLE, int MODE>
__global__ __launch_bounds__(FL_THREADS, MODE ? 6 : 4) void k_bqsr_apply_flat(ApplyArgs A) {
  typedef ApplyBody<CHECK_CYCLE, MODE> AB;
  constexpr int RMAX = AB::RMAX;
  __shared__ FlatLds<RMAX> L;
  __shared__ uint64_t s_desc[RMAX];
  __shared__ uint32_t s_seq[RMAX];
  static_assert(RMAX == APPLY_RMAX && sizeof(L) + sizeof(s_desc) + sizeof(s_seq) == APPLY_LDS_ARRAYS, "APPLY_LDS_ARRAYS lists the kernel's __shared__ arrays: add a new one there too");
  extern __shared__ __attribute__((aligned(16))) uint8_t llut[];
  const int w = 2 * A.lmax + 1, n1 = A.n_cov * (A.n_qi + 1) * w;
  const int t1_bytes = (n1 * AB::ES + 15) & ~15;
  if (MODE) {
    // level 1: ids -> one byte (MODE 1) or the row's byte offset (MODE 2)
    for (int k = threadIdx.x; k < n1; k += AB::NT) {
      const uint32_t id = A.t1[k];
      if (MODE == 1) llut[k] = (uint8_t)id;
      else reinterpret_cast<uint16_t *>(llut)[k] = (uint16_t)(id * 17u);
    }
    // level 2: rows 32 (MODE 1) or 17 (MODE 2) bytes apart
    const int n2 = (A.n_dict + 1) * 17;
    for (int k = threadIdx.x; k < n2; k += AB::NT) {
      const int row = k / 17, cx = k - 17 * row;
      llut[t1_bytes + (MODE == 1 ? 32 * row + cx : k)] = A.t2[k];
    }
    __syncthreads();
  }
  AB B;
  B.seq_off = A.seq_off; B.qual_off = A.qual_off; B.qual = A.qual; B.seq4 = A.seq4; B.lut = A.lut;
  B.flag = A.flag; B.rgid = A.rgid; B.rg_cov = A.rg_cov; B.l_seq = A.l_seq; B.qbounds = A.qbounds; B.cov_present = A.cov_present;
  B.max_cycle = A.max_cycle; B.s_desc = s_desc; B.s_seq = s_seq;
  B.lmax = A.lmax; B.rows_w = (A.n_qi + 1) * w; B.w_es = (uint32_t)(w * AB::ES);
  B.qlo = (uint32_t)A.qlo; B.qhi1 = (uint32_t)(A.qlo + A.n_qi);
  B.t1_at = lds_address(llut) - (uint32_t)A.qlo * B.w_es;
  B.t2_at = lds_address(llut) + (uint32_t)t1_bytes;
  B.err = 0;
  B.out_nb = 0; B.out_at = 0; B.out.w0 = B.out.w1 = B.out.w2 = B.out.w3 = 0;
  flat_run(A.qual_off, A.n, A.qual_bytes, A.tile_first, L, B);
  uint32_t my_err = B.err;
  if (__any(my_err != 0)) {
    for (int d = 32; d >= 1; d >>= 1) my_err |= __shfl_xor(my_err, d, 64);
    if ((threadIdx.x & 63) == 0) atomicOr(&A.err[0], my_err);
  }
}

// ---- distinct rows of the dense LUT over (read group, quality in [qlo, qlo + n_qi), cycle in [-lmax, lmax]) ----
// per_cov (round 5, apply3's covariate split): one dictionary PER covariate - rows of different covariates never share an id, the ids
// count from 0 in every covariate (counter[cov]), covariate c's rows lie at t2 + c * LUT_PC_ROWS * 17
constexpr uint32_t LUT_PC_ROWS = 256;
struct LutRows { const uint8_t *lut; int n_cov, qlo, n_qi, lmax, max_cycle, per_cov; };
__device__ __forceinline__ const uint8_t *lut_row(const LutRows &R, int r) {  // r = (cov * n_qi + qi) * w + x
  const int w = 2 * R.lmax + 1, ncyc = 2 * R.max_cycle + 1;
  const int x = r % w, qi = (r / w) % R.n_qi, cov = r / (w * R.n_qi);
  return R.lut + (((size_t)cov * ELP_NQUAL + (size_t)(R.qlo + qi)) * ncyc + (size_t)(x - R.lmax + R.max_cycle)) * 17;
}
__device__ __forceinline__ int lut_row_cov(const LutRows &R, int r) { return r / ((2 * R.lmax + 1) * R.n_qi); }
__device__ __forceinline__ bool row_eq(const uint8_t *a, const uint8_t *b) {
  bool eq = true;
#pragma unroll
  for (int k = 0; k < 17; k++) eq &= a[k] == b[k];
  return eq;
}
// every row finds or becomes the representative of its content in an open-addressing table of row indices
__global__ __launch_bounds__(256) void k_lut_rows_insert(LutRows R, int n_rows, uint32_t *slots, uint32_t mask, uint32_t *__restrict__ row_slot) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_rows) return;
  const uint8_t *mine = lut_row(R, r);
  const int my_cov = R.per_cov ? lut_row_cov(R, r) : 0;
  uint64_t h = 0x9e3779b97f4a7c15ull + (uint64_t)my_cov;
#pragma unroll
  for (int k = 0; k < 17; k++) h = (h ^ mine[k]) * 0x100000001b3ull;
  uint32_t s = (uint32_t)mix64(h) & mask;
  for (;;) {
    uint32_t cur = __hip_atomic_load(&slots[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == 0xFFFFFFFFu) {
      cur = atomicCAS(&slots[s], 0xFFFFFFFFu, (uint32_t)r);
      if (cur == 0xFFFFFFFFu) break;
    }
    if ((!R.per_cov || lut_row_cov(R, (int)cur) == my_cov) && row_eq(lut_row(R, (int)cur), mine)) break;
    s = (s + 1) & mask;
  }
  row_slot[r] = s;
}
// occupied slots get dense ids; the representative's row becomes row `id` of level 2
__global__ __launch_bounds__(256) void k_lut_rows_number(LutRows R, const uint32_t *__restrict__ slots, uint32_t n_slots, uint32_t *__restrict__ slot_id,
                                                         uint32_t *counter, uint8_t *__restrict__ t2, uint32_t t2_cap) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_slots) return;
  const uint32_t rep = slots[s];
  if (rep == 0xFFFFFFFFu) return;
  const int cov = R.per_cov ? lut_row_cov(R, (int)rep) : 0;
  const uint32_t id = atomicAdd(counter + cov, 1u);
  slot_id[s] = id;
  if (id < t2_cap) {
    const uint8_t *src = lut_row(R, (int)rep);
    uint8_t *dst = t2 + ((size_t)cov * LUT_PC_ROWS + id) * 17;  // (cov = 0 without per_cov)
    for (int k = 0; k < 17; k++) dst[k] = src[k];
  }
}
// level 1 [cov][n_qi + 1][w]: ids; the extra row per read group and (below) the extra level-2 row stand for "not resident"
__global__ __launch_bounds__(256) void k_lut_rows_index(LutRows R, const uint32_t *__restrict__ row_slot, const uint32_t *__restrict__ slot_id,
                                                        const uint32_t *__restrict__ counter, uint16_t *__restrict__ t1, uint8_t *__restrict__ t2,
                                                        uint32_t t2_cap) {
  const int w = 2 * R.lmax + 1, n1 = R.n_cov * (R.n_qi + 1) * w;
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < 17 * (R.per_cov ? R.n_cov : 1)) {  // the 0x80 row behind (every covariate's) distinct rows
    const int cv = k / 17;
    const uint32_t nd = counter[cv];
    if (nd < t2_cap) t2[((size_t)cv * LUT_PC_ROWS + nd) * 17 + (k - 17 * cv)] = 0x80;
  }
  if (k >= n1) return;
  const int x = k % w, qi = (k / w) % (R.n_qi + 1), cov = k / (w * (R.n_qi + 1));
  const uint32_t n_dict = counter[R.per_cov ? cov : 0];
  t1[k] = qi == R.n_qi ? (uint16_t)n_dict : (uint16_t)slot_id[row_slot[(cov * R.n_qi + qi) * w + x]];
}

// the dense LUT [n_cov][94][ncyc][17] from its rows form: rows [n_cov][nq][ncyc][17] for the qualities with a slot, the default byte else
__global__ __launch_bounds__(256) void k_lut_expand_rows(const uint8_t *__restrict__ rows, const uint8_t *__restrict__ defaults, const uint8_t *__restrict__ slot_of /* [94], 255 = none */,
                                                        int n_cov, int nq, int ncyc, uint8_t *__restrict__ lut) {
  const size_t row_b = (size_t)ncyc * 17, k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= (size_t)n_cov * ELP_NQUAL * row_b) return;
  const size_t r = k / row_b, w = k - r * row_b, cv = r / ELP_NQUAL, q = r % ELP_NQUAL;
  const uint8_t sl = slot_of[q];
  lut[k] = sl == 255 ? defaults[r] : rows[((cv * (size_t)nq + sl) * row_b) + w];
}

// Distinct rows of the resident part of the dense LUT (three small kernels): wk = counters | slots | slot ids | row -> slot | t1 | t2.
struct LutDict { uint32_t *slots, *slot_id, *row_slot, *counter; uint16_t *t1; uint8_t *t2; uint32_t n_slots; size_t n_rows, n1; };
constexpr uint32_t LUT_T2_CAP = 3855;  // 16-bit byte offsets
static size_t lut_dict_words(int n_cov, int n_qi, int lmax, uint32_t *n_slots_out) {
  const size_t w = 2 * (size_t)lmax + 1, n_rows = (size_t)n_cov * (size_t)std::max(n_qi, 0) * w, n1 = (size_t)n_cov * (size_t)(n_qi + 1) * w;
  uint32_t n_slots = 1024;
  while (n_slots < 2 * n_rows) n_slots <<= 1;
  *n_slots_out = n_slots;
  const size_t t2_bytes = std::max<size_t>((size_t)(LUT_T2_CAP + 1) * 17, (size_t)n_cov * LUT_PC_ROWS * 17);  // one dictionary, or one per covariate
  return 256 + (size_t)2 * n_slots + n_rows + n1 + t2_bytes / 4 + 64 + 16;
}
static LutDict lut_dict_layout(uint32_t *wk, int n_cov, int n_qi, int lmax, uint32_t n_slots) {
  const size_t w = 2 * (size_t)lmax + 1, n_rows = (size_t)n_cov * (size_t)std::max(n_qi, 0) * w, n1 = (size_t)n_cov * (size_t)(n_qi + 1) * w;
  LutDict D;
  D.n_slots = n_slots; D.n_rows = n_rows; D.n1 = n1;
  D.counter = wk;  // [256] (own words: the err_flag mailbox other stages use is not touched from the upload thread)
  D.slots = wk + 256; D.slot_id = D.slots + n_slots; D.row_slot = D.slots + 2 * (size_t)n_slots;
  D.t1 = reinterpret_cast<uint16_t *>(D.row_slot + n_rows);
  D.t2 = reinterpret_cast<uint8_t *>(D.t1 + ((n1 + 1) & ~(size_t)1));
  return D;
}
// (plain launches, no profiling brackets: also called from the upload thread while the context's own stream is busy)
static int lut_dict_build(elp_ctx *c, hipStream_t st, const LutDict &D, const uint8_t *dl, int qlo, int n_qi, int lmax, int max_cycle, bool per_cov) {
  ELP_HIP(c, hipMemsetAsync(D.slots, 0xFF, (size_t)D.n_slots * 4, st));
  ELP_HIP(c, hipMemsetAsync(D.counter, 0, 256 * 4, st));
  LutRows R{dl, c->n_cov, qlo, n_qi, lmax, max_cycle, per_cov ? 1 : 0};
  const uint32_t cap = per_cov ? LUT_PC_ROWS : LUT_T2_CAP;
  hipLaunchKernelGGL(k_lut_rows_insert, dim3(blocks_for(D.n_rows, 256)), dim3(256), 0, st, R, (int)D.n_rows, D.slots, D.n_slots - 1, D.row_slot);
  hipLaunchKernelGGL(k_lut_rows_number, dim3(blocks_for(D.n_slots, 256)), dim3(256), 0, st, R, (const uint32_t *)D.slots, D.n_slots, D.slot_id, D.counter, D.t2, cap);
  hipLaunchKernelGGL(k_lut_rows_index, dim3(blocks_for(std::max<size_t>(D.n1, 17 * 256), 256)), dim3(256), 0, st, R, (const uint32_t *)D.row_slot, (const uint32_t *)D.slot_id,
                     (const uint32_t *)D.counter, D.t1, D.t2, cap);
  ELP_HIP(c, hipGetLastError());
  return 0;
}
// How apply3.hip (read sets of one length) takes a LUT: 0 not at all, 1 the level-1 tables of every covariate in one workgroup's LDS,
// 2 split by covariate (their level 1 does not fit - many read groups -, or elp_set_tuning "apply_kernel" = 3): a workgroup holds one
// covariate's tables at a time
static int apply3_mode(const elp_ctx *c, int n_qi, int lmax, size_t *dyn_out) {
  if (c->tune.apply_kernel != 3 && apply3_bytes(c->n_cov, n_qi, lmax, APPLY3_STATIC_LDS, dyn_out) == 0) return 1;
  if (apply3_bytes(1, n_qi, lmax, APPLY3_STATIC_LDS, dyn_out) == 0) return 2;
  return 0;
}
// the resident quality range of ApplyBQSR's LDS tables, from the quality hint (-1: no quality >= 6 seen)
static void lut_quality_range(const elp_ctx *c, int *qlo, int *qhi) {
  *qlo = 0; *qhi = -1;
  for (int q = 6; q < ELP_NQUAL; q++)
    if ((q < 64 ? (c->qual_present[0] >> q) : (c->qual_present[1] >> (q - 64))) & 1ull) { if (*qhi < 0) *qlo = q; *qhi = q; }
}

}  // namespace elp

using namespace elp;

extern "C" {

// The LUT's way to the device ahead of the apply call: from the thread that built it, on the context's copy stream, while the context's
// own stream still runs the sort / metrics pass (6.4 MB at --max-cycle 500: ~0.2 ms that elp_bqsr_apply otherwise spends in front of its
// first kernel).  The LUT lives in a buffer of its own (not in the scratch pool: other stages are running).
static int lut_uploaded(elp_ctx *c, int max_cycle);
int elp_bqsr_lut_upload(elp_ctx *c, int max_cycle, const uint8_t *lut, const uint8_t *cov_present) {
  if (!c || !lut || !cov_present || max_cycle < 1) return set_error(c, ELP_ERR_ARG, "elp_bqsr_lut_upload: bad arguments");
  ELP_HIP(c, hipSetDevice(c->device));
  const size_t lut_bytes = (size_t)c->n_cov * ELP_NQUAL * (2 * (size_t)max_cycle + 1) * 17, all = lut_bytes + (size_t)c->n_cov;
  if (c->lut_ev) ELP_HIP(c, hipEventSynchronize(c->lut_ev));  // (a previous upload still in flight reads the pinned buffer)
  // a LUT that already sits in page-locked memory (elp_pinned_alloc) is copied from where it is - with many read groups the LUT is tens of
  // megabytes and the staging copy below was the longest part of the host's table path; the caller then leaves it alone until the
  // elp_bqsr_apply that uses it has been called and the context synchronised
  hipPointerAttribute_t pa;
  const bool caller_pinned = hipPointerGetAttributes(&pa, lut) == hipSuccess && pa.type == hipMemoryTypeHost;
  if (!caller_pinned) (void)hipGetLastError();  // (ordinary memory: the query fails, by design)
  const size_t staged = caller_pinned ? (size_t)c->n_cov : all;
  if (staged > c->lut_pinned_cap) {
    if (c->lut_pinned) (void)hipHostFree(c->lut_pinned);
    c->lut_pinned = nullptr; c->lut_pinned_cap = 0;
    ELP_HIP(c, hipHostMalloc(&c->lut_pinned, staged, hipHostMallocDefault));
    c->lut_pinned_cap = staged;
  }
  ELP_TRY(ensure(c, c->lut_dev, all + 64));
  if (!caller_pinned) memcpy(c->lut_pinned, lut, lut_bytes);
  memcpy(static_cast<uint8_t *>(c->lut_pinned) + (caller_pinned ? 0 : lut_bytes), cov_present, (size_t)c->n_cov);
  if (!c->lut_ev) ELP_HIP(c, hipEventCreateWithFlags(&c->lut_ev, hipEventDisableTiming));
  if (!c->copy_stream) ELP_HIP(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));  // (not the NULL stream all contexts share)
  if (c->apply_ev) ELP_HIP(c, hipStreamWaitEvent(c->copy_stream, c->apply_ev, 0));  // an apply that still reads the previous LUT
  if (caller_pinned) {
    ELP_HIP(c, hipMemcpyAsync(c->lut_dev.p, lut, lut_bytes, hipMemcpyHostToDevice, c->copy_stream));
    ELP_HIP(c, hipMemcpyAsync(c->lut_dev.p + lut_bytes, c->lut_pinned, (size_t)c->n_cov, hipMemcpyHostToDevice, c->copy_stream));
  } else {
    ELP_HIP(c, hipMemcpyAsync(c->lut_dev.p, c->lut_pinned, all, hipMemcpyHostToDevice, c->copy_stream));
  }
  return lut_uploaded(c, max_cycle);
}

// behind the LUT's arrival in lut_dev on the copy stream: the row dictionary apply3 works from - if what it depends on is known now (the
// quality hint of the gather that produced these tables, a read set of one length): 0.25 ms that elp_bqsr_apply otherwise spends in front of
// its kernel - and the event the apply waits for
static int lut_uploaded(elp_ctx *c, int max_cycle) {
  c->dict_ready = false;
  const bool force_old = c->tune.apply_kernel == 1;
  if (!force_old && c->derived.have_qual_present && c->derived.uniform_n == c->n && c->uniform_len >= 16 && c->n > 0 && (int64_t)c->max_l_seq <= (int64_t)max_cycle) {
    int qlo, qhi;
    lut_quality_range(c, &qlo, &qhi);
    const int lmax = (int)std::max<uint32_t>(c->max_l_seq, 1);
    size_t dyn3 = 0;
    const int a3 = qhi >= 0 ? apply3_mode(c, qhi - 6 + 1, lmax, &dyn3) : 0;
    if (a3) {
      const int n_qi = qhi - 6 + 1;  // (apply3: resident from quality 6 on)
      uint32_t n_slots = 0;
      const size_t words = lut_dict_words(c->n_cov, n_qi, lmax, &n_slots);
      if ((size_t)c->n_cov * (size_t)n_qi * (size_t)(2 * lmax + 1) < (1u << 22)) {
        ELP_TRY(ensure(c, c->lut_wk, words));
        const LutDict D = lut_dict_layout(c->lut_wk.p, c->n_cov, n_qi, lmax, n_slots);
        ELP_TRY(lut_dict_build(c, c->copy_stream, D, c->lut_dev.p, 6, n_qi, lmax, max_cycle, a3 == 2));
        c->dict_qlo = 6; c->dict_nqi = n_qi; c->dict_lmax = lmax; c->dict_cycle = max_cycle; c->dict_ncov = c->n_cov; c->dict_per_cov = a3 == 2;
        c->dict_ready = true;
      }
    }
  }
  ELP_HIP(c, hipEventRecord(c->lut_ev, c->copy_stream));
  c->lut_uploaded_cycle = max_cycle;
  return 0;
}

// elp_bqsr_lut_upload for the LUT in rows form (the host library's elp_bqsr_tables_build_lut_rows): n_cov x n_quals rows + one default byte
// per other row instead of n_cov x 94 rows - with 16 read groups 1.9 MB instead of 25.6 MB over PCIe (and 13 x less for the host to fill);
// a kernel on the copy stream expands it into the dense LUT every apply kernel reads.
int elp_bqsr_lut_upload_rows(elp_ctx *c, int max_cycle, const uint8_t *quals, int n_quals, const uint8_t *rows, const uint8_t *defaults, const uint8_t *cov_present) {
  if (!c || max_cycle < 1 || n_quals < 0 || n_quals > ELP_NQUAL || (n_quals && (!quals || !rows)) || !defaults || !cov_present)
    return set_error(c, ELP_ERR_ARG, "elp_bqsr_lut_upload_rows: bad arguments");
  uint8_t slot_of[ELP_NQUAL];
  memset(slot_of, 255, sizeof slot_of);
  for (int k = 0; k < n_quals; k++) {
    if (quals[k] >= ELP_NQUAL || slot_of[quals[k]] != 255) return set_error(c, ELP_ERR_ARG, "elp_bqsr_lut_upload_rows: quality list");
    slot_of[quals[k]] = (uint8_t)k;
  }
  ELP_HIP(c, hipSetDevice(c->device));
  const size_t ncyc = 2 * (size_t)max_cycle + 1, row_b = ncyc * 17;
  const size_t rows_bytes = (size_t)c->n_cov * (size_t)n_quals * row_b, def_bytes = (size_t)c->n_cov * ELP_NQUAL;
  const size_t lut_bytes = (size_t)c->n_cov * ELP_NQUAL * row_b, small = def_bytes + ELP_NQUAL + (size_t)c->n_cov;  // defaults | slot_of | cov_present
  if (c->lut_ev) ELP_HIP(c, hipEventSynchronize(c->lut_ev));  // (a previous upload still in flight reads the pinned buffer)
  hipPointerAttribute_t pa;
  const bool caller_pinned = rows_bytes && hipPointerGetAttributes(&pa, rows) == hipSuccess && pa.type == hipMemoryTypeHost;
  if (!caller_pinned) (void)hipGetLastError();
  const size_t staged = small + (caller_pinned ? 0 : rows_bytes);
  if (staged > c->lut_pinned_cap) {
    if (c->lut_pinned) (void)hipHostFree(c->lut_pinned);
    c->lut_pinned = nullptr; c->lut_pinned_cap = 0;
    ELP_HIP(c, hipHostMalloc(&c->lut_pinned, staged, hipHostMallocDefault));
    c->lut_pinned_cap = staged;
  }
  uint8_t *hp = static_cast<uint8_t *>(c->lut_pinned);
  memcpy(hp, defaults, def_bytes);
  memcpy(hp + def_bytes, slot_of, ELP_NQUAL);
  memcpy(hp + def_bytes + ELP_NQUAL, cov_present, (size_t)c->n_cov);
  if (!caller_pinned && rows_bytes) memcpy(hp + small, rows, rows_bytes);
  ELP_TRY(ensure(c, c->lut_dev, lut_bytes + (size_t)c->n_cov + 64));
  ELP_TRY(ensure(c, c->lut_rows_dev, rows_bytes + small + 64));
  if (!c->lut_ev) ELP_HIP(c, hipEventCreateWithFlags(&c->lut_ev, hipEventDisableTiming));
  if (!c->copy_stream) ELP_HIP(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
  if (c->apply_ev) ELP_HIP(c, hipStreamWaitEvent(c->copy_stream, c->apply_ev, 0));  // an apply that still reads the previous LUT
  uint8_t *d_small = c->lut_rows_dev.p, *d_rows = c->lut_rows_dev.p + ((small + 63) & ~(size_t)63);
  ELP_HIP(c, hipMemcpyAsync(d_small, hp, small, hipMemcpyHostToDevice, c->copy_stream));
  if (rows_bytes) ELP_HIP(c, hipMemcpyAsync(d_rows, caller_pinned ? rows : hp + small, rows_bytes, hipMemcpyHostToDevice, c->copy_stream));
  hipLaunchKernelGGL(k_lut_expand_rows, dim3(blocks_for(lut_bytes, 256)), dim3(256), 0, c->copy_stream, (const uint8_t *)d_rows, (const uint8_t *)d_small,
                     (const uint8_t *)(d_small + def_bytes), c->n_cov, n_quals, (int)ncyc, c->lut_dev.p);
  ELP_HIP(c, hipGetLastError());
  ELP_HIP(c, hipMemcpyAsync(c->lut_dev.p + lut_bytes, d_small + def_bytes + ELP_NQUAL, (size_t)c->n_cov, hipMemcpyDeviceToDevice, c->copy_stream));
  return lut_uploaded(c, max_cycle);
}

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
  const size_t ncyc = 2 * (size_t)max_cycle + 1;
  const size_t lut_bytes = (size_t)c->n_cov * ELP_NQUAL * ncyc * 17;
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
  const uint64_t n = c->n;
  if (n) {
    if (c->qual_bytes) {
      typedef ApplyBody<false, 1> AB;
      const uint64_t nsteps = flat_steps<AB>(c->qual_bytes);
      ELP_TRY(ensure_flat_index(c));
      ELP_TRY(ensure_qual_present(c));  // the resident quality range comes from a sample of the column (a hint: qualities outside it take the fix-up path)
      int qlo = 0, qhi = -1;
      lut_quality_range(c, &qlo, &qhi);
      const int lmax = (int)std::max<uint32_t>(c->max_l_seq, 1);
      const bool chk = (int64_t)c->max_l_seq > (int64_t)max_cycle;
      // apply3.hip takes read sets of one length (elp_set_tuning "apply_kernel" = 1 forces k_bqsr_apply_flat: A/B measurements); its level-1 table is
      // resident from quality 6 on, whatever the smallest sampled quality was
      const bool force_old = c->tune.apply_kernel == 1;  // elp_set_tuning
      ELP_TRY(ensure_uniform_len(c));
      const bool want3 = !force_old && !chk && c->uniform_len >= 16 && qhi >= 0;  // (apply3 works in whole 16-byte blocks)
      if (want3) qlo = 6;
      ApplyArgs A{n, c->qual_bytes, c->qual_off.p, c->seq_off.p, c->qual.p, c->seq4.p, c->flag.p, c->rgid.p, c->rg_cov.p, c->l_seq.p, c->qbounds.p,
                  dl + lut_bytes, c->tile_first.p, dl, max_cycle, c->err_flag.p, nullptr, nullptr, c->n_cov, 0, 0, lmax, 0};
      int mode = 0;
      size_t dyn = 0;
      const int n_qi = qhi - qlo + 1, w = 2 * lmax + 1;
      const size_t static_lds = APPLY_LDS;
      const size_t n_rows = (size_t)c->n_cov * (size_t)std::max(n_qi, 0) * (size_t)w, n1 = (size_t)c->n_cov * (size_t)(n_qi + 1) * (size_t)w;
      // apply3.hip first: the distinct rows of the resident part of the LUT (one dictionary, or - covariate split - one per covariate), built
      // behind the LUT's upload if that was possible (elp_bqsr_lut_upload), else here; the number(s) of distinct rows stay on the device: if
      // there are more than the one-byte ids hold the kernel says so and leaves without touching a byte - the next form takes over
      size_t dyn3 = 0;
      int a3 = (want3 && lmax <= max_cycle && n_rows < (1u << 22)) ? apply3_mode(c, n_qi, lmax, &dyn3) : 0;
      int dict_form = 0;  // the dictionary in `wk`: 0 none, 1 one for all covariates, 2 one per covariate
      uint32_t n_slots = 0;
      const size_t dict_words = lut_dict_words(c->n_cov, std::max(n_qi, 0), lmax, &n_slots);
      const bool prebuilt = !lut && c->dict_ready && c->dict_qlo == qlo && c->dict_nqi == n_qi && c->dict_lmax == lmax && c->dict_cycle == max_cycle &&
                            c->dict_ncov == c->n_cov;
      // the general kernel can hold a two-level LUT in LDS (how large its level 2 is shows when the dictionary is built)
      const bool flat_lds_lut = !chk && qhi >= 0 && lmax <= max_cycle && n1 + static_lds <= LDS_CU && n_rows < (1u << 22);
      uint32_t *wk = c->lut_wk.p;
      if (prebuilt) dict_form = c->dict_per_cov ? 2 : 1;
      else if (a3 || flat_lds_lut) ELP_TRY(scratch(c, 4, dict_words, &wk));
      while (a3) {
        const LutDict D = lut_dict_layout(wk, c->n_cov, n_qi, lmax, n_slots);
        if (dict_form != a3) {
          c->dict_ready = false;  // (a prebuilt dictionary of the other form is overwritten)
          ELP_TRY(lut_dict_build(c, c->stream, D, dl, qlo, n_qi, lmax, max_cycle, a3 == 2));
          dict_form = a3;
        }
        ELP_TRY(apply3_launch(c, max_cycle, dl, dl + lut_bytes, D.t1, D.t2, D.counter, n_qi, lmax, dyn3, a3 == 2));
        uint32_t e3[4];
        ELP_TRY(fetch_err(c, e3));
        if ((e3[0] & ~512u) != 0) return bqsr_error(c, e3[0] & ~512u);
        if (!(e3[0] & 512u)) {
          c->derived.qual_changed();
          return 0;
        }
        ELP_HIP(c, hipMemsetAsync(c->err_flag.p, 0, 4, c->stream));
        // too many distinct rows for one dictionary: one per covariate (a covariate's rows are the n_cov-th part); else the general kernel
        a3 = (a3 == 1 && c->n_cov > 1 && apply3_bytes(1, n_qi, lmax, APPLY3_STATIC_LDS, &dyn3) == 0) ? 2 : 0;
      }
      if (flat_lds_lut) {
        const LutDict D = lut_dict_layout(wk, c->n_cov, n_qi, lmax, n_slots);
        if (dict_form != 1) {
          c->dict_ready = false;
          ELP_TRY(lut_dict_build(c, c->stream, D, dl, qlo, n_qi, lmax, max_cycle, false));
        }
        uint32_t *counter = D.counter;
        uint16_t *t1 = D.t1;
        uint8_t *t2 = D.t2;
        const uint32_t t2_cap = LUT_T2_CAP;
        uint32_t n_dict = 0;
        ELP_HIP(c, hipMemcpyAsync(&n_dict, counter, 4, hipMemcpyDeviceToHost, c->stream));
        ELP_HIP(c, elp::stream_wait(c->stream));
        if (n_dict < t2_cap) {
          const int m = n_dict + 1 <= 256 ? 1 : 2;
          const size_t bytes = ((n1 * (size_t)m + 15) & ~(size_t)15) + (size_t)(n_dict + 1) * (m == 1 ? 32 : 17) + 16;
          if (bytes + static_lds <= LDS_CU) {
            mode = m;
            dyn = bytes;
            A.t1 = t1; A.t2 = t2; A.n_qi = n_qi; A.qlo = qlo; A.n_dict = (int)n_dict;
          }
        }
      }
      if (mode) {
        const unsigned per_cu = (unsigned)std::max<size_t>(1, std::min<size_t>(3, LDS_CU / (dyn + static_lds)));
        const unsigned g1 = (unsigned)std::min<uint64_t>(nsteps, (uint64_t)c->n_cu * per_cu);
        if (mode == 1) {
          ELP_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void *>(&k_bqsr_apply_flat<false, 1>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn));
          ELP_LAUNCH(c, "bqsr_apply", (k_bqsr_apply_flat<false, 1>), dim3(g1), dim3(FL_THREADS), dyn, A);
        } else {
          ELP_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void *>(&k_bqsr_apply_flat<false, 2>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn));
          ELP_LAUNCH(c, "bqsr_apply", (k_bqsr_apply_flat<false, 2>), dim3(g1), dim3(FL_THREADS), dyn, A);
        }
      } else {
        const unsigned grid = (unsigned)std::min<uint64_t>(nsteps, (uint64_t)c->n_cu * 8);
        if (chk) ELP_LAUNCH(c, "bqsr_apply", (k_bqsr_apply_flat<true, 0>), dim3(grid), dim3(FL_THREADS), 0, A);
        else ELP_LAUNCH(c, "bqsr_apply", (k_bqsr_apply_flat<false, 0>), dim3(grid), dim3(FL_THREADS), 0, A);
      }
    }
  }
  uint32_t e[4];
  ELP_TRY(fetch_err(c, e));
  if (e[0]) return bqsr_error(c, e[0]);
  c->derived.qual_changed();  // (the scores and the quality hint; the keys do not read QUAL)
  return 0;
}

}  // extern "C"
