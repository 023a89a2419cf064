// bqsr_count.hip — the general count kernel of the BQSR gather (any read lengths; count3.hip takes read sets of one length), the sum that
// makes the QualityScores table, and the small kernels that lay out count3.hip's records (segment sizes, the other region's sort).
//
// Reference: BaseRecalibrator.Recalibrate's per-base loop (filters/bqsr.go:505-538) over the descriptors bqsr_prologue.hip left.
//
//   k_bqsr_count   flat stream over QUAL/SEQ (flat.hpp): one lane per 16 bases.  Per chunk, SWAR in nibble space gives the
//                  eligible-base flags, the SNP flags (one XOR of 16 read nibbles with 16 nibbles of the 4-bit packed
//                  reference), the cycle parameters and the 16 context keys; then per counted base ONE packed 32-bit LDS
//                  atomic into the workgroup-private cycle table and ONE 64-bit LDS atomic into the private context table.
//                  Private tables are added into the dense int64 tables in HBM with global atomics when a workgroup is done
//                  and at the end of an index tile behind which enough reads have passed (CountBody::tile_end).
//                  Forms: 512 threads (two or three workgroups per CU), 1024 threads (one), and MG; bqsr_plan.hpp chooses,
//                  count_general_launch dispatches.
//   k_bqsr_qual_from_cycle   QualityScores is the sum of the Cycles table over cycles
//   k_c3_seg_*, k_c3_other_* the class-1 segments' first slots; the other region sorted by covariate (covariate split)
#include "bqsr_common.hpp"

namespace elp {

// private table of one workgroup: per covariate n_q + CT_XROWS rows of rs words - [0, CT_CYC) sixteen context cells of 32 | 32
// bits (observations | mismatches), then the cycle cells of 16 | 16 bits at word CT_CYC + ((17 * (cycle + lmax)) >> 4) (the 17/16
// stretch keeps the blocks of one read, sixteen cycles apart, out of each other's LDS banks); CT_PAD words behind the last row
// take the zero-adds of bases outside the read.  16-bit cycle counters are safe because a read touches a cycle cell at most once and
// the table is flushed (atomic adds into the dense int64 tables in HBM) before 2^16 reads have passed (CountBody::tile_end).
// (CT_CYC, CT_XROWS, CT_PAD: bqsr_plan.hpp)

// MG ("mismatches global"): the cycle cells hold observations only, 16 bits each, two per word, and the (rare) mismatches of the
// cycle table go straight to the dense table in HBM with one global atomic each - the private table shrinks from 4 to 2 bytes per
// (quality, cycle), so that ~40 qualities x 4 read groups x 150-base reads fit ONE workgroup's LDS in ONE pass.
template <bool CHECK_CYCLE, bool REFLDS, int NTV = FL_THREADS, bool MG = false>
struct CountBody {
  // groups of 256 reads: the per-read LDS (44 B) competes with the private tables for the 80 KB that let two workgroups share a CU
  // (with four read groups and six qualities the tables take 50 KB); 256 KiB steps save the per-step restart of the pipeline.
  // NTV = 1024: one workgroup per CU shares one big table (many qualities x read groups): same waves per SIMD as two of 512
  static constexpr int NT = NTV, TILES = 8, RMAX = NTV == 1024 ? 512 : 256;
  static constexpr bool TILE_ENDS = true;  // the private table is flushed at the end of an index tile, not of a step (tile_end)
  // kernel arguments (scalar copies: a reference to the argument struct would keep this object in scratch memory)
  const uint64_t *__restrict__ seq_off;
  const uint8_t *__restrict__ qual;
  const uint8_t *__restrict__ seq4;
  const uint4 *__restrict__ desc;
  const uint32_t *__restrict__ cigar;
  const uint32_t *__restrict__ cig_scratch;
  const uint8_t *__restrict__ skipbits;
  uint8_t *const *__restrict__ ref_seq;
  const int64_t *__restrict__ ref_seq_len;
  unsigned long long *cycle_tbl, *ctx_tbl;
  int n_cov, n_q, lmax, rs, max_cycle;
  uint32_t cov0;           // first covariate of this pass (n_cov = covariates of the pass)
  // LDS
  const uint64_t *s_refp;  // [REF_LDS] packed-contig pointers and lengths (REFLDS: n_ref <= REF_LDS; else they are read from HBM)
  const int64_t *s_refl;
  uint64_t *s_rp;          // [RMAX] per read of the group: its contig's packed bases and length (resolved once per read at
  int32_t *s_rl;           //           stage time, so that a block's loads depend on ONE LDS round trip after the read is known)
  uint4 *s_desc;
  uint32_t *s_seq;
  const uint32_t *qrow;    // [256] quality -> LDS byte address of its row in covariate 0
  const uint8_t *slot_q;
  uint32_t *tbl;
  uint32_t real_end;       // LDS byte address behind the last real row of covariate 0
  uint32_t rpc_bytes;      // bytes of one covariate's rows
  uint64_t seq_base;
  uint32_t err;
  uint32_t reads_since_flush;
  uint64_t bases_since_flush;

  __device__ __forceinline__ void ref_of(int32_t refid, const uint8_t *__restrict__ &rp, int64_t &rlen) const {
    if (REFLDS) { rp = (const uint8_t *)(const __attribute__((address_space(1))) uint8_t *)s_refp[refid]; rlen = s_refl[refid]; }
    else { rp = ref_seq[refid]; rlen = ref_seq_len[refid]; }
  }
  __device__ __forceinline__ void stage(uint32_t g0, uint32_t ng) {
    const uint4 *src = desc + 2 * (size_t)g0;
    for (uint32_t k = threadIdx.x; k < 2 * ng; k += NT) s_desc[k] = src[k];
    seq_base = seq_off[g0];
    for (uint32_t k = threadIdx.x; k < ng; k += NT) {
      s_seq[k] = (uint32_t)(seq_off[g0 + k] - seq_base);
      const uint4 dx = src[2 * k], dy = src[2 * k + 1];
      const uint8_t *rp = nullptr;
      int64_t rlen = 0;
      if ((dy.w >> 8) & BQ_ELIGIBLE) ref_of((int32_t)dx.w, rp, rlen);
      s_rp[k] = reinterpret_cast<uint64_t>(rp);
      s_rl[k] = (int32_t)rlen;
    }
  }
  __device__ __forceinline__ void ref_of_read(uint32_t rl, const uint8_t *__restrict__ &rp, int64_t &rlen) const {
    rp = (const uint8_t *)(const __attribute__((address_space(1))) uint8_t *)s_rp[rl];
    rlen = s_rl[rl];
  }

  // One base, branch-free and without a select: a base that is not counted adds ZERO to whatever cell its quality and cycle
  // point at (a cell of the table, of the row pad behind it, or of the static arrays in front of it - harmless everywhere), so
  // the sixteen bases of a block are straight-line code of ~11 VALU instructions each.  Qualities that are not counted at all
  // (< 6, or not in this pass) have a row of their own that the flush throws away; qualities > 93 and qualities without a table
  // slot count into two more rows behind the real ones (they become error bits at flush time).
  // z: (counted | mismatch << 16) of four bases, 4 bits apart; fv / ev: counted-with-context / its mismatch, 4 bits apart
  template <int I>
  __device__ __forceinline__ void base(uint32_t z, uint32_t fv, uint32_t ev, uint32_t cw, uint32_t ro, int t, uint32_t rowb, int cyc) {
    constexpr int sh = 4 * (I & 7), zs = 4 * (I & 3);
    uint32_t v1 = (z >> zs) & 0x10001u;
    uint32_t lo = bfe_u32<sh, 1>(fv), hi = bfe_u32<sh, 1>(ev);
    if (CHECK_CYCLE) {  // checkCycleCovariate, bqsr.go:364-369
      const bool out = v1 != 0 && ro < real_end && (cyc > max_cycle || cyc < -max_cycle);
      err |= out ? 16u : 0u;
      v1 = out ? 0u : v1; lo = out ? 0u : lo; hi = out ? 0u : hi;
    }
    const uint32_t row = ro + rowb;
    if (MG) lds_add_u32(lshl_add_u32<2>((uint32_t)(t >> 5), row), (v1 & 1u) << (t & 16));  // cell (t >> 4): word cell / 2, half cell & 1
    else lds_add_u32(lshl_add_u32<2>((uint32_t)(t >> 4), row), v1);
    lds_add_u64(lshl_add_u32<3>(bfe_u32<sh, 4>(cw), row), lo, hi);
  }
  // MG: the mismatches of the block's counted bases -> cycle table in HBM.  E: flag nibbles (bit 4b = base b counted and mismatching)
  __device__ __forceinline__ void mismatches_global(uint64_t E, const Chunk &ch, uint32_t cov, int cyc0, int ci) {
    const uint64_t qlo = (uint64_t)ch.w0 | ((uint64_t)ch.w1 << 32), qhi = (uint64_t)ch.w2 | ((uint64_t)ch.w3 << 32);
    const int ncyc_g = 2 * max_cycle + 1;
    while (E) {
      const int b = __builtin_ctzll(E) >> 2;
      E &= E - 1;
      const uint32_t q = (uint32_t)(((b & 8) ? qhi : qlo) >> (8 * (b & 7))) & 0xFFu;
      const int cyc = cyc0 + b * ci;
      if (qrow[q] < real_end && cyc >= -max_cycle && cyc <= max_cycle)  // a real row of this pass (not "not counted" / bad / missing)
        atomicAdd(cycle_tbl + (((size_t)cov * ELP_NQUAL + q) * ncyc_g + (size_t)(cyc + max_cycle)) * 2 + 1, 1ull);
    }
  }

  struct Pre {
    Chunk ch;            // QUAL bytes
    uint32_t skipw;      // 32 skip bits starting at bit (qpos & ~7)
    uint64_t v0, v1;     // SEQ window
    uint64_t r0, r1;     // reference window of the first piece
    int rsn;
    uint32_t rl, qlow;
    int k0, nb;
  };
  // every global load of the block is issued here: QUAL, skip bits, SEQ window, reference window
  __device__ __forceinline__ bool prefetch(uint32_t rl, int k0, int nb, uint64_t qpos, uint32_t, Pre &p) {
    const uint4 dy = s_desc[2 * rl + 1];
    const uint32_t fl = (dy.w >> 8) & 0xFFu;
    if (!(fl & BQ_ELIGIBLE)) return false;
    if ((dy.w & 0xFFu) - cov0 >= (uint32_t)n_cov) return false;  // a covariate of another pass
    const int a = (int)(dy.y & 0xFFFFu), len = (int)(dy.y >> 16);
    const int cbase = k0 - a;   // clipped base index of block bit 0
    if ((cbase < 0 ? -cbase : 0) >= (len - cbase < nb ? len - cbase : nb)) return false;  // no clipped base in the block
    const uint4 dx = s_desc[2 * rl];
    p.rl = rl; p.k0 = k0; p.nb = nb; p.qlow = (uint32_t)(qpos & 7);
    p.ch.load(qual + qpos);
    __builtin_memcpy(&p.skipw, skipbits + (qpos >> 3), 4);
    seq_load(seq4 + seq_base + s_seq[rl], k0, p.v0, p.v1);
    const uint8_t *__restrict__ rp;
    int64_t rlen;
    ref_of_read(rl, rp, rlen);
    const int32_t D0 = (int32_t)dx.x;
    p.rsn = ref_load(rp, rlen, ((fl & BQ_COMPLEX) || D0 == BQ_NOREF) ? (int64_t)0 : (int64_t)D0 + cbase, p.r0, p.r1);
    return true;
  }

  __device__ __forceinline__ void process(Pre &p) {
    const uint32_t rl = p.rl;
    const int k0 = p.k0, nb = p.nb;
    const uint4 dy = s_desc[2 * rl + 1];
    const uint4 dx = s_desc[2 * rl];
    const uint32_t fl = (dy.w >> 8) & 0xFFu;
    const int a = (int)(dy.y & 0xFFFFu), len = (int)(dy.y >> 16);
    const int cbase = k0 - a;
    int blo = -cbase, bhi = len - cbase;
    blo = blo > 0 ? blo : 0;
    bhi = bhi < nb ? bhi : nb;
    const int32_t D0 = (int32_t)dx.x, D1 = (int32_t)dx.y, D2 = (int32_t)dx.z;
    const int b1 = (int)(dy.x & 0xFFFFu), b2 = (int)(dy.x >> 16);
    const int left = (int)(dy.z & 0xFFFFu), right = (dy.z >> 16) == 0xFFFFu ? -1 : (int)(dy.z >> 16);
    const uint32_t cov = dy.w & 0xFFu;
    const bool rev = fl & BQ_REVERSED;
    const bool complex_read = fl & BQ_COMPLEX;
    const Chunk ch = p.ch;
    const uint32_t skipw = p.skipw >> p.qlow;  // known-site skip bits of the block's bases: bit (qpos + b) of the skip column
    uint64_t S, N;
    seq_unpack(p.v0, p.v1, k0, rev, S, N);
    const uint64_t R0 = ref_unpack(p.r0, p.r1, p.rsn);
    const uint64_t inw = nib_range(blo, bhi);
    uint64_t ohS, cS, ohN, cN;
    nib_classify(S, ohS, cS);
    nib_classify(N, ohN, cN);
    const uint64_t F = inw & ohS & ~nib_spread16(skipw);
    if (F == 0) return;
    // context covariate (bqsr.go:87-146): base and its predecessor in sequencing direction inside [left, right]
    const int cl = left + (rev ? 0 : 1), cr = right - (rev ? 1 : 0);
    const uint64_t CV = ohS & ohN & inw & nib_range_clamped(cl - cbase, cr - cbase + 1);
    const uint64_t CX = (cN | (cS << 2)) ^ (rev ? NIBF : 0ull);  // only read where CV is set
    // SNP events (computeSnpEvents, bqsr.go:254-285): read nibble vs reference nibble
    uint64_t X;
    {
      uint64_t R = 0;
      if (!complex_read) {
        const int B1 = b1 - cbase, B2 = b2 - cbase;  // piece boundaries in block bits (0xFFFF - cbase >= 16 when unused)
        {
          const int hi = bhi < B1 ? bhi : B1;
          if (blo < hi) {
            const uint64_t m = nib_fill(nib_range(blo, hi));
            R |= (D0 == BQ_NOREF ? S : R0) & m;
          }
        }
        if (B1 < bhi) {
          const uint8_t *__restrict__ rp;
          int64_t rlen;
          ref_of_read(rl, rp, rlen);
          const int lo = blo > B1 ? blo : B1, hi = bhi < B2 ? bhi : B2;
          if (lo < hi) {
            const uint64_t m = nib_fill(nib_range(lo, hi));
            R |= (D1 == BQ_NOREF ? S : ref_nibbles(rp, rlen, (int64_t)D1 + cbase)) & m;
          }
          if (B2 < bhi) {
            const int lo2 = blo > B2 ? blo : B2;
            if (lo2 < bhi) {
              const uint64_t m = nib_fill(nib_range(lo2, bhi));
              R |= (D2 == BQ_NOREF ? S : ref_nibbles(rp, rlen, (int64_t)D2 + cbase)) & m;
            }
          }
        }
      } else {
        const uint8_t *__restrict__ rp;
        int64_t rlen;
        ref_of_read(rl, rp, rlen);
        const uint32_t *cg = ((fl & BQ_CIG_SCRATCH) ? cig_scratch : cigar) + (uint32_t)D0;
        R = ref_nibbles_complex(cg, b1, (int64_t)D2, cbase, blo, bhi, rp, rlen, S);
      }
      X = nib_code_differs(S ^ R);  // only read where F is set
    }
    // cycle covariate (bqsr.go:376-387) of block bit b: cf + (cbase + b) * ci
    const int rof = (fl & BQ_LAST) ? -1 : 1;
    const int cf = rof + (rev ? (len - 1) * rof : 0), ci = rev ? -rof : rof;
    const int cyc0 = cf + cbase * ci;
    const uint32_t rowb = (cov - cov0) * rpc_bytes;                      // the covariate's rows
    // cycle cell (in words from the row start): (P + b * st) >> 4;  MG: two cells per word, word (P + b * st) >> 5 (CT_CYC doubled in P)
    const int P = (CT_CYC << (MG ? 5 : 4)) + 17 * (cyc0 + lmax), st = 17 * ci;

    const uint64_t E = X & F, FV = F & CV, EV = E & CV;
    const uint32_t f0 = (uint32_t)F, e0 = (uint32_t)E, f1 = (uint32_t)(F >> 32), e1 = (uint32_t)(E >> 32);
    const uint32_t za = (f0 & 0x1111u) | (e0 << 16), zb = (f0 >> 16) | (e0 & 0x11110000u);
    const uint32_t zc = (f1 & 0x1111u) | (e1 << 16), zd = (f1 >> 16) | (e1 & 0x11110000u);
    const uint32_t fv0 = (uint32_t)FV, ev0 = (uint32_t)EV, fv1 = (uint32_t)(FV >> 32), ev1 = (uint32_t)(EV >> 32);
    const uint32_t c0 = (uint32_t)CX, c1 = (uint32_t)(CX >> 32);
    // groups of eight bases between scheduling barriers: enough independent work to cover the LDS latency without letting the
    // scheduler hoist all sixteen address computations at once (register pressure => occupancy)
#define ELP_B(I, Z, FVW, EVW, CW, R) base<I>(Z, FVW, EVW, CW, R, P + (I) * st, rowb, cyc0 + (I) * ci)
    {
      const uint32_t r0 = qrow[ch.get<0>()], r1 = qrow[ch.get<1>()], r2 = qrow[ch.get<2>()], r3 = qrow[ch.get<3>()];
      const uint32_t r4 = qrow[ch.get<4>()], r5 = qrow[ch.get<5>()], r6 = qrow[ch.get<6>()], r7 = qrow[ch.get<7>()];
      ELP_B(0, za, fv0, ev0, c0, r0); ELP_B(1, za, fv0, ev0, c0, r1); ELP_B(2, za, fv0, ev0, c0, r2); ELP_B(3, za, fv0, ev0, c0, r3);
      ELP_B(4, zb, fv0, ev0, c0, r4); ELP_B(5, zb, fv0, ev0, c0, r5); ELP_B(6, zb, fv0, ev0, c0, r6); ELP_B(7, zb, fv0, ev0, c0, r7);
      __builtin_amdgcn_sched_barrier(0);
    }
    {
      const uint32_t r8 = qrow[ch.get<8>()], r9 = qrow[ch.get<9>()], r10 = qrow[ch.get<10>()], r11 = qrow[ch.get<11>()];
      const uint32_t r12 = qrow[ch.get<12>()], r13 = qrow[ch.get<13>()], r14 = qrow[ch.get<14>()], r15 = qrow[ch.get<15>()];
      ELP_B(8, zc, fv1, ev1, c1, r8); ELP_B(9, zc, fv1, ev1, c1, r9); ELP_B(10, zc, fv1, ev1, c1, r10); ELP_B(11, zc, fv1, ev1, c1, r11);
      ELP_B(12, zd, fv1, ev1, c1, r12); ELP_B(13, zd, fv1, ev1, c1, r13); ELP_B(14, zd, fv1, ev1, c1, r14); ELP_B(15, zd, fv1, ev1, c1, r15);
      __builtin_amdgcn_sched_barrier(0);
    }
#undef ELP_B
    if (MG && E) mismatches_global(E, ch, cov, cyc0, ci);
  }
  __device__ __forceinline__ void slots(uint32_t) {}
  __device__ __forceinline__ void retire() {}
  __device__ __forceinline__ void group_end(uint32_t, uint32_t) {}

  // adds the private table into the dense int64 tables (cycle: [cov][94][2*max_cycle+1][2], context: [cov][94][16][2]) and clears it;
  // the extra rows per covariate: bad and missing qualities become error bits, the row of the qualities that are not counted is dropped
  __device__ __forceinline__ void flush() {
    __syncthreads();
    const int rpc = n_q + CT_XROWS, rows = n_cov * rpc;
    const int ncyc_l = 2 * lmax + 1, ncyc_g = 2 * max_cycle + 1;
    if (MG) {
      // words of two observation cells: cell c = 2 w + half holds cycle index x with (17 x) >> 4 == c, i.e. x = c - c / 17
      const int nw = (((17 * (ncyc_l - 1)) >> 4) >> 1) + 1;
      for (int k = threadIdx.x; k < rows * nw; k += NT) {
        const int row = k / nw, w = k % nw;
        uint32_t *cell = &tbl[row * rs + CT_CYC + w];
        const uint32_t v = *cell;
        if (v) {
          *cell = 0;
          const int cov = (int)cov0 + row / rpc, slot = row % rpc;
          if (slot >= n_q) {
            err |= slot == n_q ? 8u : (slot == n_q + 1 ? 128u : 0u);
          } else {
            const int q = slot_q[slot];
#pragma unroll
            for (int half = 0; half < 2; half++) {
              const uint32_t obs = (v >> (16 * half)) & 0xFFFFu;
              const int c = 2 * w + half, cyc = c - c / 17 - lmax;
              if (obs && cyc >= -max_cycle && cyc <= max_cycle)
                atomicAdd(cycle_tbl + (((size_t)cov * ELP_NQUAL + q) * ncyc_g + (size_t)(cyc + max_cycle)) * 2, (unsigned long long)obs);
            }
          }
        }
      }
    } else
    for (int k = threadIdx.x; k < rows * ncyc_l; k += NT) {
      const int row = k / ncyc_l, x = k % ncyc_l;
      uint32_t *cell = &tbl[row * rs + CT_CYC + ((17 * x) >> 4)];
      const uint32_t v = *cell;
      if (v) {
        *cell = 0;
        const int cov = (int)cov0 + row / rpc, slot = row % rpc;
        const int cyc = x - lmax;
        if (slot >= n_q) {
          err |= slot == n_q ? 8u : (slot == n_q + 1 ? 128u : 0u);
        } else if (cyc >= -max_cycle && cyc <= max_cycle) {
          const int q = slot_q[slot];
          unsigned long long *g = cycle_tbl + (((size_t)cov * ELP_NQUAL + q) * ncyc_g + (size_t)(cyc + max_cycle)) * 2;
          atomicAdd(g, (unsigned long long)(v & 0xFFFFu));
          if (v >> 16) atomicAdd(g + 1, (unsigned long long)(v >> 16));
        }
      }
    }
    for (int k = threadIdx.x; k < rows * 16; k += NT) {
      const int row = k >> 4, cx = k & 15;
      unsigned long long *cell = reinterpret_cast<unsigned long long *>(&tbl[row * rs + 2 * cx]);
      const unsigned long long v = *cell;
      if (v) {
        *cell = 0;
        const int cov = (int)cov0 + row / rpc, slot = row % rpc;
        if (slot < n_q) {
          const int q = slot_q[slot];
          // cx = prev | cur << 2 is exactly (key >> 4) & 15 of keyFromContext (bqsr.go:64-76)
          unsigned long long *g = ctx_tbl + (((size_t)cov * ELP_NQUAL + q) * ELP_NCTX + (size_t)cx) * 2;
          atomicAdd(g, v & 0xFFFFFFFFull);
          if (v >> 32) atomicAdd(g + 1, v >> 32);
        }
      }
    }
    __syncthreads();
  }
  // a cycle cell (16 | 16 bits) takes at most one count per read, a context cell (32 | 32 bits) at most one per base; a tile
  // starts at most FL_TILE reads and holds at most FL_TILE + FL_MAX_READ bases.  The table is flushed at the end of the first index
  // tile behind which more than 30000 reads have started since the last flush: a cycle cell holds at most 30000 + FL_TILE = 62768.
  // (flat_run ends a span of tiles where tile_due says so - a step of eight tiles of one-base reads starts 262144 reads.)
  __device__ __forceinline__ bool tile_due(uint32_t nreads, uint64_t nbases) const {
    return reads_since_flush + nreads > 30000u || bases_since_flush + nbases > (1ull << 31);
  }
  __device__ __forceinline__ void tile_end(uint32_t nreads, uint64_t nbases) {
    reads_since_flush += nreads;
    bases_since_flush += nbases;
    if (reads_since_flush > 30000u || bases_since_flush > (1ull << 31)) { flush(); reads_since_flush = 0; bases_since_flush = 0; }
  }
};

// The static LDS the plan sets aside for k_bqsr_count with groups of RMAX reads: the kernel's __shared__ arrays below, term by term (the
// kernel asserts the sum against its own declarations), and COUNT_LDS_SLACK for the padding between them and a margin.
constexpr size_t COUNT_LDS_SLACK = 64 + 8 + (size_t)CT_PAD * 4;
template <int RMAX>
constexpr size_t COUNT_LDS_ARRAYS = sizeof(FlatLds<RMAX>) + sizeof(uint4[2 * RMAX]) + sizeof(uint32_t[RMAX]) + sizeof(uint32_t[256]) + sizeof(uint8_t[96]) +
                                    sizeof(uint64_t[REF_LDS]) + sizeof(int64_t[REF_LDS]) + sizeof(uint64_t[RMAX]) + sizeof(int32_t[RMAX]);
template <int RMAX>
constexpr size_t COUNT_LDS = COUNT_LDS_ARRAYS<RMAX> + COUNT_LDS_SLACK;

template <bool CHECK_CYCLE, bool REFLDS, int NTV, bool MG = false>
__global__ __launch_bounds__(NTV, 4) void k_bqsr_count(CountArgs A, QMap qm) {
  constexpr int RMAX = CountBody<CHECK_CYCLE, REFLDS, NTV, MG>::RMAX;
  __shared__ FlatLds<RMAX> L;
  __shared__ uint4 s_desc[2 * RMAX];
  __shared__ uint32_t s_seq[RMAX];
  __shared__ uint32_t qrow[256];
  __shared__ uint8_t slot_q[96];
  __shared__ uint64_t s_refp[REF_LDS];
  __shared__ int64_t s_refl[REF_LDS];
  __shared__ uint64_t s_rp[RMAX];
  __shared__ int32_t s_rl[RMAX];
  extern __shared__ __attribute__((aligned(16))) uint32_t tbl[];
  static_assert(sizeof(L) + sizeof(s_desc) + sizeof(s_seq) + sizeof(qrow) + sizeof(slot_q) + sizeof(s_refp) + sizeof(s_refl) + sizeof(s_rp) + sizeof(s_rl) ==
                    COUNT_LDS_ARRAYS<RMAX>, "COUNT_LDS_ARRAYS lists the kernel's __shared__ arrays: add a new one there too");
  const int n_all = A.n_cov * (A.n_q + CT_XROWS) * A.rs + CT_PAD;
  const uint32_t tbl_at = lds_address(tbl);
  if (REFLDS)
    for (int r = threadIdx.x; r < A.n_ref; r += NTV) { s_refp[r] = reinterpret_cast<uint64_t>(A.ref_seq[r]); s_refl[r] = A.ref_seq_len[r]; }
  for (int k = threadIdx.x; k < n_all; k += NTV) tbl[k] = 0;
  for (int q = threadIdx.x; q < 256; q += NTV) {
    int row;
    if (q < 6) row = A.n_q + 2;                // not counted (bqsr.go:301-305)
    else if (q >= ELP_NQUAL) row = A.n_q;      // bad quality
    else {
      const uint8_t s = qm.slot[q];
      row = s == 255 ? A.n_q + 2 : (s == 254 ? A.n_q + 1 : (int)s);  // counted in another pass / not in the table
      if (s < 254) slot_q[s] = (uint8_t)q;
    }
    qrow[q] = tbl_at + (uint32_t)(row * A.rs) * 4u;
  }
  __syncthreads();
  CountBody<CHECK_CYCLE, REFLDS, NTV, MG> B;
  B.seq_off = A.seq_off; B.qual = A.qual; B.seq4 = A.seq4; B.desc = reinterpret_cast<const uint4 *>(A.desc);
  B.cigar = A.cigar; B.cig_scratch = A.cig_scratch; B.skipbits = A.skipbits; B.ref_seq = A.ref_seq; B.ref_seq_len = A.ref_seq_len;
  B.cycle_tbl = A.cycle_tbl; B.ctx_tbl = A.ctx_tbl;
  B.n_cov = A.n_cov; B.n_q = A.n_q; B.lmax = A.lmax; B.rs = A.rs; B.max_cycle = A.max_cycle; B.cov0 = (uint32_t)A.cov0;
  B.s_desc = s_desc; B.s_seq = s_seq; B.qrow = qrow; B.slot_q = slot_q; B.tbl = tbl;
  B.s_refp = s_refp; B.s_refl = s_refl; B.s_rp = s_rp; B.s_rl = s_rl;
  B.real_end = tbl_at + (uint32_t)(A.n_q * A.rs) * 4u;
  B.rpc_bytes = (uint32_t)((A.n_q + CT_XROWS) * A.rs) * 4u;
  B.err = 0;
  B.reads_since_flush = 0;
  B.bases_since_flush = 0;
  flat_run(A.qual_off, A.n, A.qual_bytes, A.tile_first, L, B);
  B.flush();
  uint32_t my_err = B.err;
  if (__any(my_err != 0)) {
    for (int d = 32; d >= 1; d >>= 1) my_err |= __shfl_xor(my_err, d, 64);
    if ((threadIdx.x & 63) == 0) atomicOr(&A.err[0], my_err);
  }
}

// QualityScores[cov][q] = sum over cycles of Cycles[cov][q][*]
__global__ __launch_bounds__(256) void k_bqsr_qual_from_cycle(int n_rows, int ncyc_g, const unsigned long long *__restrict__ cycle_tbl,
                                                              unsigned long long *__restrict__ qual_tbl) {
  const int row = blockIdx.x;  // one workgroup per (cov, q)
  if (row >= n_rows) return;
  __shared__ unsigned long long so[256], se[256];
  unsigned long long o = 0, e = 0;
  for (int c = threadIdx.x; c < ncyc_g; c += 256) { o += cycle_tbl[((size_t)row * ncyc_g + c) * 2]; e += cycle_tbl[((size_t)row * ncyc_g + c) * 2 + 1]; }
  so[threadIdx.x] = o; se[threadIdx.x] = e;
  __syncthreads();
  for (int d = 128; d >= 1; d >>= 1) {
    if ((int)threadIdx.x < d) { so[threadIdx.x] += so[threadIdx.x + d]; se[threadIdx.x] += se[threadIdx.x + d]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) { qual_tbl[2 * row] = so[0]; qual_tbl[2 * row + 1] = se[0]; }
}

typedef CountBody<false, true> CB;
typedef CountBody<false, true, 1024> CB1;
extern const size_t COUNT_STATIC_LDS = COUNT_LDS<CB::RMAX>, COUNT_STATIC_LDS_1024 = COUNT_LDS<CB1::RMAX>;
static_assert(COUNT_LDS<CB::RMAX> == sizeof(FlatLds<CB::RMAX>) + (size_t)CB::RMAX * (sizeof(BqDesc) + 4) + 1024 + 96 + 64 + 8 + (size_t)CT_PAD * 4 + (size_t)REF_LDS * 16 + (size_t)CB::RMAX * 12 &&
              COUNT_LDS<CB1::RMAX> == sizeof(FlatLds<CB1::RMAX>) + (size_t)CB1::RMAX * (sizeof(BqDesc) + 4) + 1024 + 96 + 64 + 8 + (size_t)CT_PAD * 4 + (size_t)REF_LDS * 16 + (size_t)CB1::RMAX * 12,
              "the budget the plan was written around");

template <bool CC, bool RL, int NTV, bool MG>
static int count_launch_as(elp_ctx *c, const CountArgs &A, const QMap &qm, int grid, size_t dyn) {
  ELP_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void *>(&k_bqsr_count<CC, RL, NTV, MG>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn));
  ELP_LAUNCH(c, "bqsr_count", (k_bqsr_count<CC, RL, NTV, MG>), dim3(grid), dim3(NTV), dyn, A, qm);
  return 0;
}
template <bool CC, bool RL>
static int count_launch_form(elp_ctx *c, const CountArgs &A, const QMap &qm, const CountPlan &p, int grid, size_t dyn) {
  if (p.big && p.mg) return count_launch_as<CC, RL, 1024, true>(c, A, qm, grid, dyn);
  if (p.big) return count_launch_as<CC, RL, 1024, false>(c, A, qm, grid, dyn);
  return count_launch_as<CC, RL, FL_THREADS, false>(c, A, qm, grid, dyn);
}
// one pass of the general kernel in the form the plan chose: p.wg_per_cu workgroups per CU share the column's steps
int count_general_launch(elp_ctx *c, const CountArgs &A, const QMap &qm, const CountPlan &p, size_t dyn) {
  const int grid = (int)std::min<uint64_t>(flat_steps<CB>(c->qual_bytes), (uint64_t)p.wg_per_cu * (uint64_t)c->n_cu);
  const bool check_cycle = A.lmax > A.max_cycle, ref_lds = A.n_ref <= REF_LDS;
  if (check_cycle && ref_lds) return count_launch_form<true, true>(c, A, qm, p, grid, dyn);
  if (check_cycle) return count_launch_form<true, false>(c, A, qm, p, grid, dyn);
  if (ref_lds) return count_launch_form<false, true>(c, A, qm, p, grid, dyn);
  return count_launch_form<false, false>(c, A, qm, p, grid, dyn);
}

int qual_from_cycle_launch(elp_ctx *c, int ncyc_g, const unsigned long long *cycle_tbl, unsigned long long *qual_tbl) {
  ELP_LAUNCH(c, "bqsr_qual_from_cycle", k_bqsr_qual_from_cycle, dim3(c->n_cov * ELP_NQUAL), dim3(256), 0, c->n_cov * ELP_NQUAL, ncyc_g, cycle_tbl, qual_tbl);
  return 0;
}

// The "other" region of the count kernel's records (reads with indels, clipped windows, descriptors; appended by three kernels in
// arrival order) sorted by covariate for the covariate-split count: counts per covariate, offsets, a scatter into a second region.
constexpr int CO_TILE = 1024;  // (CO_MAXCOV: bqsr_plan.hpp)
__global__ __launch_bounds__(256) void k_c3_other_hist(const uint4 *__restrict__ recs, const uint32_t *__restrict__ n_dev, uint32_t *__restrict__ cnt /* [CO_MAXCOV] */) {
  __shared__ uint32_t h[CO_MAXCOV];
  const uint32_t n = *n_dev;
  if ((uint64_t)blockIdx.x * CO_TILE >= n) return;
  h[threadIdx.x] = 0;
  __syncthreads();
  for (uint32_t k = blockIdx.x * CO_TILE + threadIdx.x; k < n && k < (blockIdx.x + 1u) * CO_TILE; k += 256) atomicAdd(&h[recs[2 * (size_t)k + 1].y & (CO_MAXCOV - 1)], 1u);
  __syncthreads();
  if (h[threadIdx.x]) atomicAdd(&cnt[threadIdx.x], h[threadIdx.x]);
}
__global__ void k_c3_other_offsets(const uint32_t *__restrict__ cnt, uint32_t *__restrict__ off /* [CO_MAXCOV + 1] */, uint32_t *__restrict__ cursor) {
  uint32_t at = 0;
  for (int c = 0; c < CO_MAXCOV; c++) { off[c] = at; cursor[c] = at; at += cnt[c]; }
  off[CO_MAXCOV] = at;
}
__global__ __launch_bounds__(256) void k_c3_other_scatter(const uint4 *__restrict__ recs, const uint32_t *__restrict__ n_dev, uint32_t *cursor, uint4 *__restrict__ out) {
  __shared__ uint32_t h[CO_MAXCOV], base[CO_MAXCOV];
  const uint32_t n = *n_dev;
  if ((uint64_t)blockIdx.x * CO_TILE >= n) return;
  h[threadIdx.x] = 0;
  __syncthreads();
  uint32_t my[CO_TILE / 256], cv[CO_TILE / 256];
#pragma unroll
  for (int j = 0; j < CO_TILE / 256; j++) {
    const uint32_t k = blockIdx.x * CO_TILE + j * 256 + threadIdx.x;
    cv[j] = k < n ? (recs[2 * (size_t)k + 1].y & (CO_MAXCOV - 1)) : 0u;
    my[j] = k < n ? atomicAdd(&h[cv[j]], 1u) : 0u;
  }
  __syncthreads();
  base[threadIdx.x] = h[threadIdx.x] ? atomicAdd(&cursor[threadIdx.x], h[threadIdx.x]) : 0u;
  __syncthreads();
#pragma unroll
  for (int j = 0; j < CO_TILE / 256; j++) {
    const uint32_t k = blockIdx.x * CO_TILE + j * 256 + threadIdx.x;
    if (k < n) {
      const size_t to = (size_t)base[cv[j]] + my[j];
      out[2 * to] = recs[2 * (size_t)k];
      out[2 * to + 1] = recs[2 * (size_t)k + 1];
    }
  }
}

// Covariate-split class-1 segments (RecOut, round 5): how many records segment (wave % groups) * ncs + covariate can receive at most - the
// reads of that covariate among the records the first prologue pass's workgroups of that group handle - and the
// segments' first slots as the prefix sums of those counts (or, fixed != 0: a fixed stride apart).  Workgroup b covers the records of the
// prologue's workgroup b.
__global__ __launch_bounds__(256) void k_c3_seg_hist(uint64_t n, const uint16_t *__restrict__ rgid, const uint16_t *__restrict__ rg_cov, uint32_t groups, uint32_t ncs,
                                                     uint32_t *__restrict__ seg_cap /* [groups * ncs] */) {
  __shared__ uint32_t h[C3_MAXSEG];
  h[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t i0 = (uint64_t)blockIdx.x * PF_TILES * 256 + threadIdx.x;
  for (int tile = 0; tile < PF_TILES; tile++) {
    const uint64_t i = i0 + (uint64_t)tile * 256;
    if (i0 - threadIdx.x + (uint64_t)tile * 256 >= n) break;  // (uniform: the whole tile lies behind the last record)
    const uint16_t rg = i < n ? rgid[i] : (uint16_t)ELP_NIL16;
    const uint32_t cov = rg == ELP_NIL16 ? 0xFFFFu : (uint32_t)(rg_cov[rg] & 0xFFu);
    // (every lane adds its one in the LDS: cheaper than forming the wave's groups by covariate first, apply3.hip k_apply_cov_hist)
    if (cov < ncs) atomicAdd(&h[(blockIdx.x % groups) * ncs + cov], 1u);  // (workgroup b covers the records of the prologue's workgroup b)
  }
  __syncthreads();
  if (threadIdx.x < groups * ncs && h[threadIdx.x]) atomicAdd(&seg_cap[threadIdx.x], h[threadIdx.x]);
}
__global__ void k_c3_seg_offsets(const uint32_t *__restrict__ seg_cap, uint32_t nseg, uint32_t fixed, uint32_t *__restrict__ seg_base /* [nseg + 1] */) {
  uint32_t at = 0;
  for (uint32_t s2 = 0; s2 < nseg; s2++) { seg_base[s2] = at; at += fixed ? fixed : seg_cap[s2]; }
  seg_base[nseg] = at;
}

// clears the record counters and leaves the class-1 segments' first slots: ncs == 0 a fixed S.cap_s1 apart, else (covariate split) the
// prefix sums of the exact counts
int c3_segments_launch(elp_ctx *c, const GatherScratch &S, uint32_t *block, uint32_t nseg, uint32_t ncs) {
  uint32_t *seg_cap = block + S.seg_cap;
  ELP_HIP(c, hipMemsetAsync(block + S.rec_cnt, 0, (size_t)(C3_MAXSEG + 1) * C3_CSTRIDE * sizeof(uint32_t), c->stream));
  if (ncs) {
    ELP_HIP(c, hipMemsetAsync(seg_cap, 0, (size_t)C3_MAXSEG * sizeof(uint32_t), c->stream));
    ELP_LAUNCH(c, "bqsr_seg_hist", k_c3_seg_hist, dim3(S.pf_grid), dim3(256), 0, c->n, (const uint16_t *)c->rgid.p, (const uint16_t *)c->rg_cov.p, nseg / ncs, ncs, seg_cap);
  }
  ELP_LAUNCH(c, "bqsr_seg_offsets", k_c3_seg_offsets, dim3(1), dim3(1), 0, (const uint32_t *)seg_cap, nseg, ncs ? 0u : (uint32_t)S.cap_s1, block + S.seg_base);
  return 0;
}

// the other region sorted by covariate into `sorted`; cw: [CO_MAXCOV] counts | [CO_MAXCOV + 1] offsets | [CO_MAXCOV] cursors, cleared by the caller
int c3_other_sort_launch(elp_ctx *c, const uint4 *other, const uint32_t *n_other, uint32_t *cw, uint4 *sorted) {
  uint32_t *ooff = cw + CO_MAXCOV;
  const unsigned og = blocks_for(c->n, CO_TILE);  // (launched for the worst case; blocks behind the region's end leave at once)
  ELP_LAUNCH(c, "bqsr_other_hist", k_c3_other_hist, dim3(og), dim3(256), 0, other, n_other, cw);
  ELP_LAUNCH(c, "bqsr_other_offsets", k_c3_other_offsets, dim3(1), dim3(1), 0, (const uint32_t *)cw, ooff, ooff + CO_MAXCOV + 1);
  ELP_LAUNCH(c, "bqsr_other_scatter", k_c3_other_scatter, dim3(og), dim3(256), 0, other, n_other, ooff + CO_MAXCOV + 1, sorted);
  return 0;
}

}  // namespace elp
