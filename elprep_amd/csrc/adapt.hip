// adapt.hip — the adapt stage: unclipped 5' position, Phred-sum score and low-quality-tail bounds, the coordinate key column; the
// tile index and the one-length check of the staged QUAL column; the sample of the quality values that occur.
//
// Reference: computeUnclippedPosition / computePhredScore (filters/mark-duplicates.go:57-110); the key's order is sam.CoordinateLess
// (sam/sam-types.go:429-438).  The key's width is host arithmetic (sort_plan.hpp: key_width).
#include <cstdlib>

#include "apply_rec.hpp"
#include "common.hpp"
#include "flat.hpp"
#include "sort_plan.hpp"

namespace elp {

// ------------------------------------------------------------------ adapt
// fixed-field part: unclipped 5' position (computeUnclippedPosition :79-110) and the CoordinateLess primary key
__global__ __launch_bounds__(256) void k_adapt_fixed(uint64_t n, const int32_t *__restrict__ pos, const int32_t *__restrict__ refid,
                                                     const uint16_t *__restrict__ flag, const uint64_t *__restrict__ cigar_off,
                                                     const uint32_t *__restrict__ cigar, int32_t *__restrict__ upos, int32_t *__restrict__ score,
                                                     uint64_t *__restrict__ key, uint32_t n_ref, int pos_bits,
                                                     const uint8_t *__restrict__ has_sr) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint16_t f = flag[i];
  const int32_t p = pos[i];
  const int32_t r = refid[i];
  // CoordinateLess primary key: REFID ascending with negative last (:429-432), POS (:433-436), forward before reverse (:437-438)
  // The key is packed into as few bits as the data needs (unmapped = one code above the last contig; POS in pos_bits bits, the
  // width of the largest staged POS), so that the LSD radix sort has as few live digit positions as possible.
  // Records with the sr tag are dropped behind the mark-duplicates filter (RemoveOptionalReads, cmd/filter.go:803) and never reach
  // the sort: they get one more code above "unmapped", i.e. the tail of the permutation (elp_num_sorted()).
  const uint64_t ru = has_sr[i] ? (uint64_t)n_ref + 1 : (r < 0 ? (uint64_t)n_ref : (uint64_t)(uint32_t)r);
  key[i] = (ru << (pos_bits + 1)) | ((uint64_t)(uint32_t)p << 1) | ((f & F_REVERSED) ? 1ull : 0ull);
  int32_t up = 0;
  if ((f & (F_UNMAPPED | F_SECONDARY | F_SUPPLEMENTARY)) == 0) {  // mark-duplicates.go:427,436
    const uint64_t c0 = cigar_off[i], c1 = cigar_off[i + 1];
    up = p;
    if (c1 > c0) {
      if (f & F_REVERSED) {  // :90-100
        int32_t clipped = 1;
        up--;
        for (uint64_t k = c1; k-- > c0;) {
          const uint32_t c = cigar[k];
          const uint32_t op = c & 0xF;
          const int32_t isclip = (op == OP_S || op == OP_H) ? 1 : 0;
          const int32_t isref = op_consumes_ref(op) ? 1 : 0;
          clipped *= isclip;
          up += (isref | clipped) * (int32_t)(c >> 4);
        }
      } else {  // :101-108
        for (uint64_t k = c0; k < c1; k++) {
          const uint32_t c = cigar[k];
          const uint32_t op = c & 0xF;
          if (!(op == OP_S || op == OP_H)) break;
          up -= (int32_t)(c >> 4);
        }
      }
    }
  }
  upos[i] = up;
  score[i] = 0;
}

// byte mask (0xFF per byte) for the first n bytes (n unclamped) of a 32-bit word
__device__ __forceinline__ uint32_t first_bytes32(int n) { return n <= 0 ? 0u : (n >= 4 ? 0xFFFFFFFFu : (0xFFFFFFFFu >> (32 - 8 * n))); }

// computePhredScore :57-68 as a flat stream over the QUAL column: sum of qualities >= 15 per duplicate-marking candidate;
// any quality > 93 in a candidate is an error.  SWAR over the lane's 16 bytes, v_sad_u8 for the byte sums.
struct ScoreBody {
  static constexpr int NT = FL_THREADS, TILES = 4, RMAX = 1024;
  static constexpr bool TILE_ENDS = false;
  const uint16_t *__restrict__ flag;
  const uint8_t *__restrict__ qual;
  int32_t *score;
  uint64_t *qbounds;
  int32_t *acc;    // LDS [RMAX]: per-read partial sums of this group (LDS atomics; one global store per read)
  uint32_t *lo;    // LDS [RMAX]: index of the first quality > 2 of the read (0xFFFFFFFF: none yet)
  uint32_t *hi;    // LDS [RMAX]: 1 + index of the last quality > 2 (0: none yet)
  uint8_t *cand;   // LDS [RMAX]: duplicate-marking candidate?
  const uint4 *mask;  // LDS [17]: byte masks of the first nb bytes of a block, one 16-byte read instead of sixteen instructions
  uint32_t bad;

  __device__ __forceinline__ void stage(uint32_t g0, uint32_t ng) {
    for (uint32_t k = threadIdx.x; k < ng; k += NT) {
      acc[k] = 0;
      lo[k] = 0xFFFFFFFFu;
      hi[k] = 0u;
      cand[k] = (flag[g0 + k] & (F_UNMAPPED | F_SECONDARY | F_SUPPLEMENTARY)) == 0;
    }
  }
  // Byte tests of a word by ONE add: for bytes below 128 - 113 (every legal quality is) adding 113 / 125 / 34 sets bit 7 of exactly the
  // bytes >= 15 / > 2 / >= 94 without a carry into the next byte; a byte that does carry is >= 94 in the first place and is reported as
  // such (`bad`, checked on the same word).  The words are masked to the block's bytes first, so no test needs the mask again.
  static __device__ __forceinline__ uint32_t part(uint32_t x, uint32_t s) {  // s + the sum of the bytes >= 15
    const uint32_t ge15 = ((x + 0x71717171u) & 0x80808080u) >> 7;
    return __builtin_amdgcn_sad_u8(x & (ge15 * 0xFFu), 0u, s);
  }
  static __device__ __forceinline__ uint32_t gt2(uint32_t x) { return (((x | 0x80808080u) - 0x03030303u) | x) & 0x80808080u; }  // bit 7 of every byte > 2, whatever the bytes (a missing-QUAL filler of 0xFF in a non-candidate must not spill into its neighbour's test)
  static __device__ __forceinline__ uint32_t ge94(uint32_t x) { return x | (x + 0x22222222u); }           // bit 7 of every byte >= 94 (or >= 128)
  struct Pre { Chunk ch; uint32_t rl; int nb; int k0; };
  __device__ __forceinline__ bool prefetch(uint32_t rl, int k0, int nb, uint64_t qpos, uint32_t, Pre &p) {
    p.rl = rl; p.nb = nb; p.k0 = k0;
    p.ch.load(qual + qpos);
    return true;
  }
  __device__ __forceinline__ void process(Pre &p) {
    const uint4 mk = mask[p.nb];
    const uint32_t x0 = p.ch.w0 & mk.x, x1 = p.ch.w1 & mk.y, x2 = p.ch.w2 & mk.z, x3 = p.ch.w3 & mk.w;
    // low-quality-tail bounds: first / last quality > 2 of the read
    const uint64_t glo = (uint64_t)gt2(x0) | ((uint64_t)gt2(x1) << 32);
    const uint64_t ghi = (uint64_t)gt2(x2) | ((uint64_t)gt2(x3) << 32);
    if (glo | ghi) {
      const int first = glo ? (__builtin_ctzll(glo) >> 3) : 8 + (__builtin_ctzll(ghi) >> 3);
      const int last = ghi ? 8 + ((63 - __builtin_clzll(ghi)) >> 3) : ((63 - __builtin_clzll(glo)) >> 3);
      atomicMin(&lo[p.rl], (uint32_t)(p.k0 + first));
      atomicMax(&hi[p.rl], (uint32_t)(p.k0 + last + 1));
    }
    if (!cand[p.rl]) return;
    // a quality >= 94 (or a byte whose carry could have spoilt a neighbour's test) in a duplicate-marking candidate: the error bit
    bad |= (ge94(x0) | ge94(x1) | ge94(x2) | ge94(x3)) & 0x80808080u;
    const uint32_t s = part(x3, part(x2, part(x1, part(x0, 0u))));
    if (s) atomicAdd(&acc[p.rl], (int32_t)s);
  }
  __device__ __forceinline__ void group_end(uint32_t g0, uint32_t ng) {
    for (uint32_t k = threadIdx.x; k < ng; k += NT) {  // a read belongs to exactly one group
      score[g0 + k] = acc[k];
      qbounds[g0 + k] = (uint64_t)hi[k] | ((uint64_t)lo[k] << 32);  // all-zero = no quality > 2
    }
  }
  __device__ __forceinline__ void slots(uint32_t) {}
  __device__ __forceinline__ void retire() {}
  __device__ __forceinline__ void tile_end(uint32_t, uint64_t) {}
};

__global__ __launch_bounds__(FL_THREADS) void k_score_flat(uint64_t n, const uint64_t *__restrict__ qual_off, const uint8_t *__restrict__ qual,
                                                           uint64_t qual_bytes, const uint32_t *__restrict__ tile_first,
                                                           const uint16_t *__restrict__ flag, int32_t *score, uint64_t *qbounds, uint32_t *err) {
  __shared__ FlatLds<ScoreBody::RMAX> L;
  __shared__ int32_t acc[ScoreBody::RMAX];
  __shared__ uint32_t lo[ScoreBody::RMAX], hi[ScoreBody::RMAX];
  __shared__ uint8_t cand[ScoreBody::RMAX];
  __shared__ uint4 mask[17];
  if (threadIdx.x <= 16) {
    const int nb = (int)threadIdx.x;
    mask[nb] = make_uint4(first_bytes32(nb), first_bytes32(nb - 4), first_bytes32(nb - 8), first_bytes32(nb - 12));
  }
  __syncthreads();
  ScoreBody B{flag, qual, score, qbounds, acc, lo, hi, cand, mask, 0u};
  flat_run(qual_off, n, qual_bytes, tile_first, L, B);
  if (__any(B.bad != 0) && (threadIdx.x & 63) == 0) atomicOr(&err[0], 1u);
}

// computePhredScore + the low-quality-tail bounds for read sets of ONE length (what a sequencer writes; ensure_uniform_len): a READ per
// lane.  A wave copies the QUAL bytes of 64 consecutive reads - one contiguous, 64-byte-aligned span - into its own LDS tile with
// coalesced 16-byte loads and every lane then walks the words of its read: the sums, the error test and the positions of the first /
// last quality > 2 stay in the lane's registers.  k_score_flat spreads a read over ~10 lanes and combines them through three LDS
// atomics per 16-byte block on the read's cells (PMC, round 3: 79 % of its LDS cycles were bank conflicts of exactly those).
constexpr int SU_WAVES = 8, SU_MAX_LEN = 250;  // a read touches at most 64 words (the bitmap of words with a quality > 2)
__device__ __forceinline__ uint32_t su_gt2(uint32_t x) { return (((x | 0x80808080u) - 0x03030303u) | x) & 0x80808080u; }  // bit 7 of every byte > 2, any byte value
template <int R>
__global__ __launch_bounds__(64 * SU_WAVES) void k_score_uniform(uint64_t n, uint32_t L, const uint8_t *__restrict__ qual, const uint16_t *__restrict__ flag,
                                                                 int32_t *__restrict__ score, uint64_t *__restrict__ qbounds, uint32_t *err,
                                                                 uint32_t qstride /* every qstride-th group of 64 reads notes the quality values it holds */,
                                                                 unsigned long long *qmask, const uint16_t *__restrict__ rgid, const uint16_t *__restrict__ rg_cov,
                                                                 uint2 *__restrict__ arecs /* not null: ApplyBQSR's per-read records (apply_rec.hpp) */) {
  extern __shared__ __attribute__((aligned(16))) uint32_t su_lds[];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t tile_bytes = 64u * L, tile_words = tile_bytes / 4u + 4u;
  uint32_t *tile = su_lds + (size_t)wave * tile_words;
  const uint32_t s = lane * L, w0 = s >> 2, skip = s & 3u;  // the read's first word and the bytes of it in front of the read
  const uint32_t nw = (skip + L + 3u) >> 2, tail = (skip + L) & 3u;
  const uint32_t m_first = 0xFFFFFFFFu << (8u * skip), m_last = tail ? 0xFFFFFFFFu >> (32u - 8u * tail) : 0xFFFFFFFFu;
  uint32_t bad = 0;
  uint32_t qm[3] = {0, 0, 0};  // bits 0 .. 95: quality values seen by the sampled groups (the BQSR gather's sizing hint, ensure_qual_present)
  const uint64_t ngroups = (n + 63) / 64;
  for (uint64_t g = (uint64_t)blockIdx.x * SU_WAVES + wave; g < ngroups; g += (uint64_t)gridDim.x * SU_WAVES) {
    const uint64_t r0 = g * 64;
    const uint8_t *base = qual + r0 * L;
    const uint64_t have = (n - r0 < 64 ? n - r0 : 64) * (uint64_t)L;  // the last group may be short
    uint4 v[R];
#pragma unroll
    for (int k = 0; k < R; k++) {
      const uint32_t off = (uint32_t)k * 1024u + lane * 16u;
      v[k] = make_uint4(0u, 0u, 0u, 0u);
      if (off < have) v[k] = *reinterpret_cast<const uint4 *>(base + off);  // (the column is padded: the last chunk may read past `have`)
    }
#pragma unroll
    for (int k = 0; k < R; k++) {
      const uint32_t off = (uint32_t)k * 1024u + lane * 16u;
      if (off < tile_bytes) *reinterpret_cast<uint4 *>(tile + off / 4u) = v[k];
    }
    // (the tile is the wave's own, and a wave's LDS operations execute in order: no barrier)
    const uint64_t r = r0 + lane;
    if (r < n) {
      const uint16_t f = flag[r];
      const bool cand = (f & (F_UNMAPPED | F_SECONDARY | F_SUPPLEMENTARY)) == 0;
      const uint16_t rg = arecs ? rgid[r] : (uint16_t)ELP_NIL16;
      const uint32_t *rw = tile + w0;
      uint32_t x = rw[0] & m_first;
      if (nw == 1) x &= m_last;
      // per word: the sum of the bytes >= 15 (six operations), the OR of all words (the > 93 test is made ONCE on it: a byte of the OR is
      // at least the byte of every word, so a clean OR clears the read - legal qualities stay below 64, whose ORs stay below 94 - and only a
      // flagged OR is looked at word by word), and the first / last word that holds a quality > 2 as two running indices (round 6: five
      // vector instructions fewer per word than a 64-bit bitmap of such words and a > 93 test per word; measured on the same box: no change
      // in the kernel's time - 73 % vector issue by PMC, but the LDS tile's round trip is what a wave waits for)
      constexpr uint32_t NONE = 0xFFFFFFFFu;
      uint32_t sum = ScoreBody::part(x, 0u), orx = x;
      uint32_t kf = su_gt2(x) ? 0u : NONE, kl = 0u;
#pragma unroll 8
      for (uint32_t k = 1; k + 1 < nw; k++) {
        x = rw[k];
        sum = ScoreBody::part(x, sum);
        orx |= x;
        const bool gk = su_gt2(x) != 0u;
        kf = min(kf, gk ? k : NONE);
        kl = gk ? k : kl;
      }
      if (nw > 1) {
        x = rw[nw - 1] & m_last;
        sum = ScoreBody::part(x, sum);
        orx |= x;
        const bool gk = su_gt2(x) != 0u;
        kf = min(kf, gk ? nw - 1 : NONE);
        kl = gk ? nw - 1 : kl;
      }
      uint32_t bd = ScoreBody::ge94(orx) & 0x80808080u;
      if (bd) {  // (rare) exactly, word by word
        bd = 0;
        for (uint32_t k = 0; k < nw; k++) {
          uint32_t xw = rw[k];
          if (k == 0) xw &= m_first;
          if (k == nw - 1) xw &= m_last;
          bd |= ScoreBody::ge94(xw);
        }
      }
      uint32_t lo = 0xFFFFFFFFu, hi = 0u;
      if (kf != NONE) {
        uint32_t xf = rw[kf], xl = rw[kl];
        if (kf == 0) xf &= m_first;
        if (kf == nw - 1) xf &= m_last;
        if (kl == 0) xl &= m_first;
        if (kl == nw - 1) xl &= m_last;
        lo = kf * 4u + ((uint32_t)__builtin_ctz(su_gt2(xf)) >> 3) - skip;
        hi = kl * 4u + ((31u - (uint32_t)__builtin_clz(su_gt2(xl))) >> 3) - skip + 1u;
      }
      score[r] = cand ? (int32_t)sum : 0;
      qbounds[r] = (uint64_t)hi | ((uint64_t)lo << 32);
      if (cand) bad |= bd & 0x80808080u;
      if (arecs) arecs[r] = rg == ELP_NIL16 ? make_uint2(AR_NO_RG, 0u) : apply_record(L, (int)L, f, (uint64_t)hi | ((uint64_t)lo << 32), rg_cov[rg]);
      if ((uint32_t)g % qstride == 0) {  // (wave-uniform)
        for (uint32_t k = 0; k < nw; k++) {
          const uint32_t vm = (k == 0 ? m_first : 0xFFFFFFFFu) & (k + 1 == nw ? m_last : 0xFFFFFFFFu), xw = rw[k];
#pragma unroll
          for (int b = 0; b < 4; b++) {
            const uint32_t q = (xw >> (8 * b)) & 0xFFu, bit = ((vm >> (8 * b)) & 1u) << (q & 31u), ws = q >> 5;
            qm[0] |= ws == 0 ? bit : 0u;
            qm[1] |= ws == 1 ? bit : 0u;
            qm[2] |= ws == 2 ? bit : 0u;
          }
        }
      }
    }
  }
  if (__any(bad != 0) && lane == 0) atomicOr(&err[0], 1u);
  if (__any((qm[0] | qm[1] | qm[2]) != 0)) {
    for (int d = 32; d >= 1; d >>= 1) {
      qm[0] |= __shfl_xor(qm[0], d, 64);
      qm[1] |= __shfl_xor(qm[1], d, 64);
      qm[2] |= __shfl_xor(qm[2], d, 64);
    }
    if (lane == 0) {
      const unsigned long long lo = (unsigned long long)qm[0] | ((unsigned long long)qm[1] << 32);
      if (lo) atomicOr(&qmask[0], lo);
      if (qm[2]) atomicOr(&qmask[1], (unsigned long long)qm[2]);
    }
  }
}
// LDS bank conflicts of the per-lane walk: lanes are L bytes apart; if that is a whole number of words with a large power of two in it,
// many lanes sit on one bank - those lengths stay with k_score_flat
static bool score_uniform_ok(uint32_t L) {
  if (L < 16 || L > (uint32_t)SU_MAX_LEN) return false;
  if (L % 4u) return true;
  return ((L / 4u) % 4u) != 0;  // at most two lanes more per bank than the 64-lanes-on-32-banks minimum
}
template <int R>
static int score_uniform_launch(elp_ctx *c) {
  const uint32_t L = c->uniform_len;
  const size_t dyn = (size_t)SU_WAVES * ((size_t)64 * L + 16);
  const unsigned per_cu = (unsigned)std::max<size_t>(1, (160 * 1024) / (dyn + 256));
  const uint64_t ngroups = (c->n + 63) / 64;
  const unsigned grid = (unsigned)std::min<uint64_t>((ngroups + SU_WAVES - 1) / SU_WAVES, (uint64_t)c->n_cu * per_cu);
  ELP_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void *>(&k_score_uniform<R>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn));
  // ApplyBQSR's records on the way (apply3.hip takes whole 16-byte blocks of reads of one length)
  uint2 *arecs = nullptr;
  if (L >= 16 && L <= 0x7FFF && c->n_rg > 0) {
    ELP_TRY(ensure(c, c->apply_recs, c->n + 4));
    arecs = c->apply_recs.p;
  }
  // the sample of the quality values: everything up to ~500 K reads (the hint is then exact, as k_qual_present_sample's is), one group in
  // up to 128 of longer columns
  const uint32_t qstride = (uint32_t)std::min<uint64_t>(128, std::max<uint64_t>(1, ngroups / 8192));
  ELP_LAUNCH(c, "adapt_score", k_score_uniform<R>, dim3(grid), dim3(64 * SU_WAVES), dyn, c->n, L, (const uint8_t *)c->qual.p, (const uint16_t *)c->flag.p,
             c->score.p, c->qbounds.p, c->adapt_err.p, qstride, reinterpret_cast<unsigned long long *>(c->adapt_err.p + 2), (const uint16_t *)c->rgid.p,
             (const uint16_t *)c->rg_cov.p, arecs);
  c->derived.adapt_sampled = true;
  c->derived.apply_recs_valid = arecs != nullptr;
  c->apply_recs_lmax = (int)L;
  return 0;
}
static int score_uniform(elp_ctx *c) {
  switch ((c->uniform_len + 15u) / 16u) {  // 16-byte load rounds of a wave's tile
#define ELP_SU(R) case R: return score_uniform_launch<R>(c);
    ELP_SU(1) ELP_SU(2) ELP_SU(3) ELP_SU(4) ELP_SU(5) ELP_SU(6) ELP_SU(7) ELP_SU(8) ELP_SU(9) ELP_SU(10) ELP_SU(11) ELP_SU(12) ELP_SU(13) ELP_SU(14)
    ELP_SU(15) ELP_SU(16)
#undef ELP_SU
  }
  return set_error(c, ELP_ERR_ARG, "score_uniform: read length %u", c->uniform_len);
}

// Set of quality values present, from a sample of the tiles (every `stride`-th).  It is a sizing hint for the BQSR gather's
// LDS tables, not a correctness input: k_bqsr_count reports any counted quality it has no table slot for and the host retries.
// `span`: bytes looked at per sampled tile (the exact set after a miss: stride 1, whole tiles)
__global__ __launch_bounds__(256) void k_qual_present_sample(const uint8_t *__restrict__ qual, uint64_t qual_bytes, uint64_t stride, uint64_t span,
                                                             unsigned long long *qmask) {
  const uint64_t ntiles = (qual_bytes + FL_TILE - 1) / FL_TILE;
  uint32_t m[3] = {0, 0, 0};  // bits 0..95
  for (uint64_t t = (uint64_t)blockIdx.x * stride; t < ntiles; t += (uint64_t)gridDim.x * stride) {
    const uint64_t tb = t * FL_TILE, te = (tb + span < qual_bytes) ? tb + span : qual_bytes;
    for (uint64_t p = tb + (uint64_t)threadIdx.x * 16; p < te; p += 256 * 16) {
      Chunk ch;
      ch.load(qual + p);
      const int nv = (int)((te - p) < 16 ? (te - p) : 16);
#pragma unroll
      for (int i = 0; i < 16; i++) {
        const uint32_t wv = (i >> 2) == 0 ? ch.w0 : ((i >> 2) == 1 ? ch.w1 : ((i >> 2) == 2 ? ch.w2 : ch.w3));
        const uint32_t q = (wv >> (8 * (i & 3))) & 0xFFu;
        const uint32_t bit = (i < nv) ? (1u << (q & 31u)) : 0u;
        const uint32_t wsel = q >> 5;
        m[0] |= wsel == 0 ? bit : 0u;
        m[1] |= wsel == 1 ? bit : 0u;
        m[2] |= wsel == 2 ? bit : 0u;
      }
    }
  }
  for (int d = 32; d >= 1; d >>= 1) {
    m[0] |= __shfl_xor(m[0], d, 64);
    m[1] |= __shfl_xor(m[1], d, 64);
    m[2] |= __shfl_xor(m[2], d, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    const unsigned long long lo = (unsigned long long)m[0] | ((unsigned long long)m[1] << 32);
    if (lo) atomicOr(&qmask[0], lo);
    if (m[2]) atomicOr(&qmask[1], (unsigned long long)m[2]);
  }
}

// tile_first[t] = first read r (0 <= r <= n) with qual_off[r] >= t * FL_TILE, for t in [0, ntiles); tile_first[ntiles] = n
__global__ __launch_bounds__(256) void k_flat_index(const uint64_t *__restrict__ qual_off, uint64_t n_reads, uint64_t ntiles,
                                                    uint32_t *__restrict__ tile_first) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t > ntiles) return;
  if (t == ntiles) { tile_first[t] = (uint32_t)n_reads; return; }
  const uint64_t x = t * FL_TILE;
  uint64_t lo = 0, hi = n_reads;  // answer in [lo, hi]: qual_off[n_reads] = qual_bytes > x
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (qual_off[mid] >= x) hi = mid; else lo = mid + 1;
  }
  tile_first[t] = (uint32_t)lo;
}

int ensure_flat_index(elp_ctx *c) {
  if (c->derived.has_flat_index(c->n, c->qual_bytes)) return 0;
  const uint64_t ntiles = (c->qual_bytes + FL_TILE - 1) / FL_TILE;
  ELP_TRY(ensure(c, c->tile_first, ntiles + 2));
  if (c->n)
    ELP_LAUNCH(c, "flat_index", k_flat_index, dim3(blocks_for(ntiles + 1, 256)), dim3(256), 0, (const uint64_t *)c->qual_off.p, c->n, ntiles,
               c->tile_first.p);
  c->derived.flat_index_n = c->n;
  c->derived.flat_index_bytes = c->qual_bytes;
  return 0;
}

// Do all staged reads have one length?  (every QUAL offset i * len, every SEQ offset SEQ_FRONT + i * ((len + 1) / 2)): then the per-base
// kernels need no offsets at all (count3.hip).  A fact of the staged columns: checked once per staging, like the tile index.
__global__ __launch_bounds__(256) void k_uniform_check(uint64_t n, const uint64_t *__restrict__ qual_off, const uint64_t *__restrict__ seq_off,
                                                       const uint32_t *__restrict__ l_seq, uint64_t len, uint64_t sb, uint64_t seq_front, uint32_t *bad) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool b = false;
  if (i < n) b = qual_off[i] != i * len || seq_off[i] != seq_front + i * sb || (uint64_t)l_seq[i] != len;
  if (i == n) b = qual_off[n] != n * len || seq_off[n] != seq_front + n * sb;
  if (__any(b) && (threadIdx.x & 63) == 0) atomicOr(bad, 1u);
}
int ensure_uniform_len(elp_ctx *c) {
  if (c->derived.has_uniform(c->n, c->qual_bytes)) return 0;
  c->uniform_len = 0;
  c->derived.uniform_n = c->n;
  c->derived.uniform_bytes = c->qual_bytes;
  if (!c->n || c->qual_bytes % c->n) return 0;
  const uint64_t len = c->qual_bytes / c->n;
  if (len == 0 || len > 0x3FFFFFull) return 0;
  uint32_t *bad = c->err_flag.p + 2;
  ELP_HIP(c, hipMemsetAsync(bad, 0, 4, c->stream));
  ELP_LAUNCH(c, "uniform_check", k_uniform_check, dim3(blocks_for(c->n + 1, 256)), dim3(256), 0, c->n, (const uint64_t *)c->qual_off.p,
             (const uint64_t *)c->seq_off.p, (const uint32_t *)c->l_seq.p, len, (len + 1) / 2, (uint64_t)elp_ctx::SEQ_FRONT, bad);
  uint32_t hb = 0;
  ELP_HIP(c, hipMemcpyAsync(&hb, bad, 4, hipMemcpyDeviceToHost, c->stream));
  ELP_HIP(c, elp::stream_wait(c->stream));
  ELP_HIP(c, hipMemsetAsync(bad, 0, 4, c->stream));
  if (!hb) c->uniform_len = (uint32_t)len;
  return 0;
}

int adapt_quality_error(elp_ctx *c) {
  return set_error(c, ELP_ERR_DATA, "Invalid QUAL character (phred > 93) in a duplicate-marking candidate (reference: log.Panic, filters/mark-duplicates.go:64-66)");
}

// check_quals: report a quality > 93 in a duplicate-marking candidate (computePhredScore panics); the BQSR entry points, which
// only need the per-read low-quality-tail bounds, pass false and leave that error to a later elp_mark_duplicates
// the quality-error word of the score kernel, read when somebody needs it (check_quals) - or by elp_mark_duplicates together with its
// own first read-back (adapt_note): the adapt stage has no synchronisation of its own
static int adapt_resolve(elp_ctx *c) {
  if (!c->derived.adapt_pending) return 0;
  uint32_t w[ADAPT_WORDS];
  ELP_HIP(c, hipMemcpyAsync(w, c->adapt_err.p, sizeof w, hipMemcpyDeviceToHost, c->stream));
  ELP_HIP(c, elp::stream_wait(c->stream));
  adapt_note(c, w);
  return 0;
}
// words: [0] the score kernel's error word, [2 .. 5] the quality values its sampled groups saw (k_score_uniform only)
void adapt_note(elp_ctx *c, const uint32_t *words) {
  c->derived.adapt_word_read((words[0] & 1u) != 0);
  if (c->derived.adapt_sampled) {
    c->adapt_qmask[0] = (unsigned long long)words[2] | ((unsigned long long)words[3] << 32);
    c->adapt_qmask[1] = (unsigned long long)words[4] | ((unsigned long long)words[5] << 32);
  }
}
int adapt_begin(elp_ctx *c, int *pos_bits_out) {
  ELP_HIP(c, hipSetDevice(c->device));
  const uint64_t n = c->n;
  ELP_TRY(ensure_flat_index(c));
  ELP_TRY(ensure(c, c->upos, n + 1));
  ELP_TRY(ensure(c, c->score, n + 1));
  ELP_TRY(ensure(c, c->key, n + 1));
  ELP_TRY(ensure(c, c->qbounds, n + 1));
  ELP_TRY(ensure(c, c->adapt_err, ADAPT_WORDS + 2));
  ELP_HIP(c, hipMemsetAsync(c->adapt_err.p, 0, ADAPT_WORDS * sizeof(uint32_t), c->stream));
  c->derived.adapt_begins();
  const KeyWidth kw = key_width(c->max_pos, c->n_ref);
  c->key_bits = kw.key_bits;
  *pos_bits_out = kw.pos_bits;
  return 0;
}
// every record's score and low-quality-tail bounds (records without QUAL bytes: zero)
int adapt_scores(elp_ctx *c) {
  const uint64_t n = c->n;
  if (!n) return 0;
  if (!c->qual_bytes) {  // no QUAL bytes at all: no tile, no kernel
    ELP_HIP(c, hipMemsetAsync(c->qbounds.p, 0, n * sizeof(uint64_t), c->stream));
    ELP_HIP(c, hipMemsetAsync(c->score.p, 0, n * sizeof(int32_t), c->stream));
    return 0;
  }
  ELP_TRY(ensure_uniform_len(c));
  if (c->uniform_len && score_uniform_ok(c->uniform_len) && c->tune.score_kernel != 1) {
    ELP_TRY(score_uniform(c));  // (writes the score of every record)
  } else {
    ELP_HIP(c, hipMemsetAsync(c->score.p, 0, n * sizeof(int32_t), c->stream));  // (a read without bases belongs to no tile's group)
    const unsigned grid = (unsigned)std::min<uint64_t>(flat_steps<ScoreBody>(c->qual_bytes), (uint64_t)c->n_cu * 4);
    ELP_LAUNCH(c, "adapt_score_flat", k_score_flat, dim3(grid), dim3(FL_THREADS), 0, n, (const uint64_t *)c->qual_off.p, (const uint8_t *)c->qual.p,
               c->qual_bytes, (const uint32_t *)c->tile_first.p, (const uint16_t *)c->flag.p, c->score.p, c->qbounds.p, c->adapt_err.p);
  }
  c->derived.adapt_pending = true;
  return 0;
}
int ensure_adapted(elp_ctx *c, bool check_quals) {
  if (c->derived.adapted()) {
    if (check_quals) ELP_TRY(adapt_resolve(c));
    return (check_quals && c->derived.adapt_bad_qual) ? adapt_quality_error(c) : 0;
  }
  int pos_bits = 1;
  ELP_TRY(adapt_begin(c, &pos_bits));
  const uint64_t n = c->n;
  if (n) {
    ELP_LAUNCH(c, "adapt_fixed", k_adapt_fixed, dim3(blocks_for(n, 256)), dim3(256), 0, n, (const int32_t *)c->pos.p, (const int32_t *)c->refid.p,
               (const uint16_t *)c->flag.p, (const uint64_t *)c->cigar_off.p, (const uint32_t *)c->cigar.p, c->upos.p, c->score.p, c->key.p,
               (uint32_t)c->n_ref, pos_bits, (const uint8_t *)c->has_sr.p);
    ELP_TRY(adapt_scores(c));
  }
  c->derived.keys = c->derived.scores = true;
  if (check_quals) ELP_TRY(adapt_resolve(c));
  return (check_quals && c->derived.adapt_bad_qual) ? adapt_quality_error(c) : 0;
}
// all the coordinate sort asks for: it reads no score, so nothing elp_bqsr_apply spoils sends it back into the adapt stage
int ensure_keys(elp_ctx *c) { return c->derived.keys ? 0 : ensure_adapted(c, false); }

// c->qual_present = quality values seen in a sample of the QUAL column (a sizing hint, see k_qual_present_sample)
int ensure_qual_present(elp_ctx *c, bool exact) {
  if (c->derived.have_qual_present) return 0;
  c->qual_present[0] = c->qual_present[1] = 0;
  // elp_set_tuning "qual_hint" = 1: the hint stays empty, which forces the gather's report-and-retry path (tests)
  if (!exact && c->tune.qual_hint != 1 && c->derived.scores && c->derived.adapt_sampled) {
    // the score kernel sampled the column as it went (k_score_uniform): no pass, and no wait of its own if the error word is in already
    ELP_TRY(adapt_resolve(c));
    c->qual_present[0] = c->adapt_qmask[0];
    c->qual_present[1] = c->adapt_qmask[1];
  } else if (c->qual_bytes && (exact || c->tune.qual_hint != 1)) {
    unsigned long long *qm;
    ELP_TRY(scratch(c, 6, 4, &qm));
    ELP_HIP(c, hipMemsetAsync(qm, 0, 16, c->stream));
    const uint64_t ntiles = (c->qual_bytes + FL_TILE - 1) / FL_TILE;
    const uint64_t stride = exact ? 1 : std::min<uint64_t>(16, std::max<uint64_t>(1, ntiles / 2048));
    const unsigned grid = (unsigned)std::min<uint64_t>((ntiles + stride - 1) / stride, 2048);
    ELP_LAUNCH(c, "qual_present_sample", k_qual_present_sample, dim3(grid), dim3(256), 0, (const uint8_t *)c->qual.p, c->qual_bytes, stride,
               (exact || stride == 1) ? FL_TILE : (uint64_t)4096, qm);
    ELP_HIP(c, hipMemcpyAsync(c->qual_present, qm, 16, hipMemcpyDeviceToHost, c->stream));
    ELP_HIP(c, elp::stream_wait(c->stream));
  }
  // elp_set_tuning "qual_hint_drop" = q removes one quality from the hint (tests: the kernels' no-slot paths)
  if (!exact && c->tune.qual_hint_drop >= 0) {
    const int q = c->tune.qual_hint_drop;
    if (q < 64) c->qual_present[0] &= ~(1ull << q);
    else if (q < 128) c->qual_present[1] &= ~(1ull << (q - 64));
  }
  c->derived.have_qual_present = true;
  return 0;
}

}  // namespace elp
