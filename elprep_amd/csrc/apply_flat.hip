// apply_flat.hip — ApplyBQSR's general kernel (any read lengths; apply3.hip takes read sets of one length).
// Reference: BaseRecalibratorTables.ApplyBQSR (filters/bqsr.go:936-1005); the covariates' device helpers are in bqsr_dev.hpp.
//   k_bqsr_apply_flat   flat stream over QUAL/SEQ (flat.hpp), one lane per 16 bases, QUAL rewritten in place.  MODE 0: a byte gather per
//                       base from the dense LUT in HBM / L2; MODE 1, 2: from a two-level LUT in LDS (ids of distinct rows | the rows)
//   apply_flat_launch   the instantiation and launch the plan names (apply_plan.hpp: flat_launch_plan)
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

// The static LDS the plan (apply_plan.hpp: ApplyShape.lds_flat) sets aside for k_bqsr_apply_flat: the kernel's __shared__ arrays, term by
// term (the kernel asserts the sum against its own declarations), and a margin.
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

extern const size_t APPLY_STATIC_LDS = APPLY_LDS;

int apply_flat_launch(elp_ctx *c, const ApplyShape &s, const ApplyPlan &p, const uint8_t *d_lut, const uint8_t *d_cov_present, const uint16_t *t1, const uint8_t *t2,
                      uint32_t n_dict) {
  const FlatLaunch f = flat_launch_plan(s, p, n_dict, flat_steps<ApplyBody<false, 1>>(c->qual_bytes));
  ApplyArgs A{};
  A.n = c->n; A.qual_bytes = c->qual_bytes;
  A.qual_off = c->qual_off.p; A.seq_off = c->seq_off.p; A.qual = c->qual.p; A.seq4 = c->seq4.p;
  A.flag = c->flag.p; A.rgid = c->rgid.p; A.rg_cov = c->rg_cov.p; A.l_seq = c->l_seq.p; A.qbounds = c->qbounds.p;
  A.cov_present = d_cov_present; A.tile_first = c->tile_first.p; A.lut = d_lut;
  A.max_cycle = p.max_cycle; A.err = c->err_flag.p;
  A.n_cov = c->n_cov; A.lmax = p.lmax;
  if (f.mode) { A.t1 = t1; A.t2 = t2; A.n_qi = p.n_qi; A.qlo = p.qlo; A.n_dict = (int)n_dict; }
  void (*const k)(ApplyArgs) = f.mode == 1 ? k_bqsr_apply_flat<false, 1> : f.mode == 2 ? k_bqsr_apply_flat<false, 2> : p.chk ? k_bqsr_apply_flat<true, 0> : k_bqsr_apply_flat<false, 0>;
  if (f.mode) ELP_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)f.dyn));
  ELP_LAUNCH(c, "bqsr_apply", k, dim3(f.grid), dim3(FL_THREADS), f.dyn, A);
  return 0;
}

}  // namespace elp
