// bgzf_inflate.hip — BGZF on the device, inflate (RFC 1951): the blocks of a BAM file inflated in HBM, in two phases.
// Reference: the reader inflates every block with compress/flate on a worker goroutine (utils/bgzf/bgzf-files.go:164-221) and checks
// its CRC-32.  A BAM file of a 30x genome is a few hundred thousand independent blocks of <= 64 KB.
#include "bgzf.hpp"
#include "bgzf_crc.hpp"

namespace elp {

// base values and extra-bit counts of the length codes 257.. and the distance codes (RFC 1951 3.2.5), by arithmetic (as tables in constant
// memory they cost every match four dependent memory round trips); checked against the RFC's tables at compile time
__host__ __device__ constexpr uint32_t inf_len_ext(uint32_t ls) { return ls < 8u || ls == 28u ? 0u : (ls - 4u) >> 2; }
__host__ __device__ constexpr uint32_t inf_len_base(uint32_t ls) { return ls < 8u ? 3u + ls : (ls == 28u ? 258u : 3u + ((4u + (ls & 3u)) << inf_len_ext(ls))); }
__host__ __device__ constexpr uint32_t inf_dist_ext(uint32_t ds) { return ds < 4u ? 0u : (ds - 2u) >> 1; }
__host__ __device__ constexpr uint32_t inf_dist_base(uint32_t ds) { return ds < 4u ? 1u + ds : 1u + ((2u + (ds & 1u)) << inf_dist_ext(ds)); }
namespace inf_check {
constexpr uint16_t LENS[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
constexpr uint8_t LEXT[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
constexpr uint16_t DISTS[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
constexpr uint8_t DEXT[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
constexpr bool ok() {
  for (uint32_t k = 0; k < 29; k++) if (inf_len_base(k) != LENS[k] || inf_len_ext(k) != LEXT[k]) return false;
  for (uint32_t k = 0; k < 30; k++) if (inf_dist_base(k) != DISTS[k] || inf_dist_ext(k) != DEXT[k]) return false;
  return true;
}
static_assert(ok(), "length / distance code arithmetic differs from RFC 1951 3.2.5");
}  // namespace inf_check
__constant__ uint8_t INF_ORDER[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// canonical decoding of the next code in `word` (LSB first), at most 15 bits: symbol, *len = its length; -1: no such code
__device__ inline int canon_decode(const uint16_t *count, const uint16_t *symbol, uint32_t word, int *len_out) {
  int code = 0, first = 0, index = 0;
  for (int len = 1; len <= 15; len++) {
    code |= (int)(word & 1u);
    word >>= 1;
    const int cnt = count[len];
    if (code - cnt < first) { *len_out = len; return symbol[index + (code - first)]; }
    index += cnt;
    first += cnt;
    first <<= 1;
    code <<= 1;
  }
  return -1;
}

// Two phases.  The serial part of DEFLATE is the bit stream, not the copies (on BAM records most symbols are matches of 5 - 7 bytes, literal
// runs are one or two symbols long, and a third of the matches reach further back than a few KB of the block's output), so a window of the
// output in LDS would bound the waves per CU - and with them the rate:
//   phase A  k_bgzf_tokens   a wave per block walks the Huffman stream and does NOTHING else: a literal goes straight to its place in the
//            block's output (HBM), a match becomes an 8-byte token {output position | length << 16, distance} appended to the block's token
//            list (the lanes that hold matches write theirs together).  No window, no drain: 5 KB of LDS per wave (1 KB input ring, u32
//            tables of 9 / 8 bits), 80 VGPRs: 24 waves per CU.
//   phase B  k_bgzf_resolve  a workgroup per block: every output byte gets a PARENT in LDS (u16 [65536]) - itself for a literal; for
//            byte i of a match: position - distance + (i mod distance), i.e. always a byte in front of the match -; pointer jumping
//            (parent = parent[parent], every thread over its unfinished bytes, no barrier between the rounds) leaves every byte pointing at
//            the literal it descends from; ONE pass then fills the matches in from the block's own output, which holds the literals
//            already, and takes the CRC-32.
// Stored blocks copy their bytes in phase A.  The tokens of a block: at most (bytes / 3) of 8 bytes each, 171 KB per block of scratch.
// Phase A is bound by issued instructions, not by latency (a wave that decodes symbol after symbol spends ~150 instructions on each, and the
// lanes beside lane 0 repeat them), so the lanes decode AT ONCE: lane k decodes the symbol that would start k bits behind the wave's place
// in the stream - all 64 candidates, one table look-up (two for a match) each, branch-free -; the wave then walks the true chain (start at
// 0, step by the bits the symbol there consumed: ~6 scalar steps per 64 bits, a hand-written loop), which also gives every true symbol its
// place in the output; the lanes on the chain store their literal or their token.  ~5 symbols per round of ~230 issued instructions
// (110 scalar, 76 vector, 34 branches, 7 LDS: profiles/round6_bgzf_pmc.csv and the run behind it) instead of one per ~150.
// A symbol whose code is longer than the tables' bits, the end of a block and an invalid symbol are decoded on the walk: for a long code
// lane L tests whether the first L bits are a code of length L, all lengths at once (tk_slow_entry).
constexpr int TK_RING = 1024, TK_HALF = TK_RING / 2, TK_LB = 9, TK_DB = 8;
// table entry: code length (4 bits; 0: the code is longer than the table's bits) | kind << 4 | extra bits << 6 | base value << 10
enum : uint32_t { TK_LIT = 0, TK_MATCH = 1, TK_EOB = 2, TK_BAD = 3 };
// what a lane found at its offset: bits consumed | output bytes << 7 | flag << 16
enum : uint32_t { TF_SLOW = 1, TF_EOB = 2, TF_BAD = 3 };
struct TokLds {
  uint32_t ring[TK_RING / 4 + 4];  // the last four words mirror the first four: a window is three consecutive words from anywhere in the ring
  uint32_t ltab[1 << TK_LB], dtab[1 << TK_DB];
  uint16_t lcount[16], dcount[16], lsym[288], dsym[32];
  uint16_t lfirst[16], loffs[16], dfirst[16], doffs[16];  // per code length: the first canonical code, the place of its symbol in lsym / dsym
  uint8_t lengths[320];
  int left;
};
__device__ __forceinline__ uint32_t tk_lit_entry(uint32_t sym, uint32_t len) {
  if (sym < 256u) return len | (TK_LIT << 4) | (sym << 10);
  if (sym == 256u) return len | (TK_EOB << 4);
  if (sym >= 286u) return len | (TK_BAD << 4);
  return len | (TK_MATCH << 4) | (inf_len_ext(sym - 257u) << 6) | (inf_len_base(sym - 257u) << 10);
}
__device__ __forceinline__ uint32_t tk_dist_entry(uint32_t sym, uint32_t len) {
  if (sym >= 30u) return len | (TK_BAD << 4);
  return len | (TK_MATCH << 4) | (inf_dist_ext(sym) << 6) | (inf_dist_base(sym) << 10);
}
// count / symbol arrays of the canonical code (lane 0), then the table, every lane its share of the bit patterns.  `kind`: 0 the code of
// the code lengths (entries: symbol << 10 | length), 1 literals / lengths, 2 distances.  > 0: incomplete, < 0: over-subscribed.
__device__ inline int tok_huff_build(TokLds *L, uint16_t *count, uint16_t *symbol, const uint8_t *length, int n, uint32_t *tab, int tbits, int kind) {
  if ((threadIdx.x & 63u) == 0) {
    uint16_t offs[16];
    for (int len = 0; len <= 15; len++) count[len] = 0;
    for (int sym = 0; sym < n; sym++) count[length[sym]]++;
    int left = 1;
    if (count[0] == n) left = 0;
    else {
      for (int len = 1; len <= 15 && left >= 0; len++) { left <<= 1; left -= count[len]; }
      if (left >= 0) {
        offs[1] = 0;
        for (int len = 1; len < 15; len++) offs[len + 1] = offs[len] + count[len];
        if (kind) {  // the walk's decoder of long codes (tk_slow_entry): first code and first symbol per length
          uint16_t *first = kind == 1 ? L->lfirst : L->dfirst, *ofs = kind == 1 ? L->loffs : L->doffs;
          uint32_t f = 0;
          first[0] = 0;
          ofs[0] = 0;
          for (int len = 1; len <= 15; len++) { first[len] = (uint16_t)f; ofs[len] = offs[len]; f = (f + count[len]) << 1; }
        }
        for (int sym = 0; sym < n; sym++)
          if (length[sym] != 0) symbol[offs[length[sym]]++] = (uint16_t)sym;
      }
    }
    L->left = left;
  }
  __syncthreads();  // (one wave per workgroup: orders its lanes' LDS writes before the reads that follow)
  const int left = L->left;
  if (left >= 0)
    for (uint32_t idx = threadIdx.x & 63u; idx < (1u << tbits); idx += 64u) {
      int len = 0;
      const int sym = canon_decode(count, symbol, idx, &len);
      uint32_t e = 0;
      if (sym >= 0 && len <= tbits) e = kind == 0 ? ((uint32_t)sym << 10) | (uint32_t)len : (kind == 1 ? tk_lit_entry((uint32_t)sym, (uint32_t)len) : tk_dist_entry((uint32_t)sym, (uint32_t)len));
      tab[idx] = e;
    }
  __syncthreads();
  return left;
}
struct TokInflater {
  TokLds *L;
  const uint8_t *in;
  uint32_t in_len, in_bits, loaded;
  uint32_t bp;  // the reader's place in the block's input, in bits
  uint32_t out_len, out_at;
  uint8_t *out;
  uint2 *tokens;  // the block's token array (HBM)
  uint32_t ntok;
  // the ring holds input [loaded - TK_RING, loaded): topped up whenever the reader enters its last half (16 bytes per lane)
  __device__ __forceinline__ void feed() {
    while (loaded < in_len && (bp >> 3) + TK_HALF > loaded) {
      const uint32_t lane16 = (threadIdx.x & 63u) * 16u, p = loaded + lane16;
      __syncthreads();
      if (lane16 < (uint32_t)TK_HALF && p < in_len) {  // (the compressed bytes are followed by the trailer and the buffer's padding: a 16-byte read is safe)
        uint4 v;
        __builtin_memcpy(&v, in + p, 16);
        const uint32_t at = (p & (TK_RING - 1)) >> 2;
        *reinterpret_cast<uint4 *>(&L->ring[at]) = v;
        if (at == 0) *reinterpret_cast<uint4 *>(&L->ring[TK_RING / 4]) = v;
      }
      __syncthreads();
      loaded = loaded + TK_HALF < in_len ? loaded + TK_HALF : in_len;
    }
  }
  // the 64 bits of the input from bit b on (what lies behind the input's end is garbage: the callers check their place against in_bits)
  __device__ __forceinline__ unsigned long long window(uint32_t b) const {
    const uint32_t *r = &L->ring[(b >> 5) & (TK_RING / 4 - 1)];
    const uint32_t w0 = r[0], w1 = r[1], w2 = r[2];
    // (v_alignbit: the low 32 bits of {hi, lo} >> (b & 31))
    return ((unsigned long long)__builtin_amdgcn_alignbit(w2, w1, b) << 32) | __builtin_amdgcn_alignbit(w1, w0, b);
  }
  __device__ __forceinline__ uint32_t bits(int n) {  // n <= 16; the header's fields
    feed();
    const uint32_t v = (uint32_t)window(bp) & ((1u << n) - 1u);
    bp += (uint32_t)n;
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
  }
  // a symbol of the code of the code lengths (table entries symbol << 10 | length, 7 bits: never a miss)
  __device__ __forceinline__ int cl_symbol() {
    feed();
    const uint32_t e = (uint32_t)__builtin_amdgcn_readfirstlane((int)L->ltab[(uint32_t)window(bp) & 127u]);
    if (!e) return -1;
    bp += e & 15u;
    return (int)(e >> 10);
  }
};
// one symbol at bit b by canonical decoding, for the walk: its entry in the table's form with the true code length (0: no such code)
// (every code length at once: lane L tests whether the first L bits are a code of length L - canonical codes of one length are consecutive
// numbers, first[L] .. first[L] + count[L] - 1, MSB first -; the bit-by-bit walk of canon_decode took fifteen dependent LDS reads)
__device__ __forceinline__ uint32_t tk_slow_entry(const TokInflater &s, uint32_t b, bool dist) {
  const uint32_t lane = threadIdx.x & 63u, ll = lane & 15u;
  const uint16_t *count = dist ? s.L->dcount : s.L->lcount, *first = dist ? s.L->dfirst : s.L->lfirst, *ofs = dist ? s.L->doffs : s.L->loffs;
  const uint32_t rev = __brev((uint32_t)s.window(b)) >> 17;  // the next fifteen bits, the first one on top
  const uint32_t c = rev >> (15u - ll), f = first[ll], cnt = count[ll];
  const bool hit = lane >= 1u && lane <= 15u && c - f < cnt;
  const unsigned long long m = __ballot(hit);
  if (!m) return 0;
  const int len = __builtin_ctzll(m);
  const uint32_t idx = (uint32_t)__builtin_amdgcn_readlane((int)(ofs[ll] + c - f), len);
  const uint32_t sym = (uint32_t)__builtin_amdgcn_readfirstlane((int)(dist ? s.L->dsym : s.L->lsym)[idx]);
  return dist ? tk_dist_entry(sym, (uint32_t)len) : tk_lit_entry(sym, (uint32_t)len);
}
__device__ inline int tok_codes(TokInflater &s) {
  TokLds *L = s.L;
  const uint32_t lane = threadIdx.x & 63u;
  for (;;) {
    s.feed();
    // every lane: the symbol that starts `lane` bits on.  Without branches: the distance part is computed for every lane (for a literal's
    // entry the extra-bit count is 0 and the look-up lands somewhere in the table: discarded)
    const unsigned long long w = s.window(s.bp + lane);
    const uint32_t e = L->ltab[(uint32_t)w & ((1u << TK_LB) - 1u)];
    const uint32_t cl = e & 15u, xb = (e >> 6) & 15u, t = cl + xb;
    uint32_t kind = (e >> 4) & 3u, val = e >> 10;
    const uint32_t e2 = L->dtab[(uint32_t)(w >> t) & ((1u << TK_DB) - 1u)];
    const uint32_t dl = e2 & 15u, db = (e2 >> 6) & 15u;
    uint32_t dist = (e2 >> 10) + ((uint32_t)(w >> (t + dl)) & ((1u << db) - 1u));
    const bool is_m = kind == TK_MATCH;
    uint32_t olen = is_m ? val + ((uint32_t)(w >> cl) & ((1u << xb) - 1u)) : 1u;
    const bool special = e == 0 || kind >= TK_EOB || (is_m && (e2 == 0 || ((e2 >> 4) & 3u) == TK_BAD));
    // bits consumed | output bytes << 7; a symbol for the walk's slow path: 64 bits "consumed" (the walk's loop ends there) | a mark
    constexpr uint32_t TK_SPECIAL = 64u | (1u << 30);
    const int info = special ? (int)TK_SPECIAL : (int)((is_m ? t + dl + db : cl) | (olen << 7));
    // the walk along the true chain (wave-uniform values throughout); a lane on the chain learns its place in the output
    uint32_t off = 0, outpos = s.out_at;
    int vpos = -1, rc = 0;
    bool eob = false;
    for (;;) {
      // the chain's fast steps, by hand (the compiler's loop: 9 scalar + 4 vector + 3 branch instructions a step, two of the branches
      // taken; this one: 5 + 2 + 1 - the kernel is bound by issued scalar instructions, profiles/round6_bgzf_pmc_final.csv).  The place in
      // the input and the place in the output advance in ONE register (acc = off | outpos << 7: a lane's `info` has the same layout and
      // off stays below 128); a special lane's info carries 64 as its bits: the loop's one test (off < 64) ends on it too, its mark says why
      //   while (off < 64) { inf = readlane(info, off); vpos[lane off] = outpos; acc += inf; }
      bool special_hit = false;
      if (off < 64u) {
        int inf, tmp, m0_was;
        uint32_t acc = off | (outpos << 7);
        asm volatile(
            "s_mov_b32 %[m0w], m0\n\t"
            "1:\n\t"
            "v_readlane_b32 %[inf], %[info], %[off]\n\t"
            "s_lshr_b32 %[tmp], %[acc], 7\n\t"
            "s_mov_b32 m0, %[off]\n\t"
            "v_writelane_b32 %[vpos], %[tmp], m0\n\t"
            "s_add_u32 %[acc], %[acc], %[inf]\n\t"
            "s_and_b32 %[off], %[acc], 0x7f\n\t"
            "s_bitcmp0_b32 %[acc], 6\n\t"
            "s_cbranch_scc1 1b\n\t"
            "s_mov_b32 m0, %[m0w]\n\t"
            : [inf] "=&s"(inf), [tmp] "=&s"(tmp), [m0w] "=&s"(m0_was), [off] "+s"(off), [acc] "+s"(acc), [vpos] "+v"(vpos)
            : [info] "v"(info)
            : "scc");
        if ((uint32_t)inf & (1u << 30)) {  // the loop ended on a special lane: take its step back (that lane's vpos is set below, or unset)
          acc -= (uint32_t)inf;
          special_hit = true;
        }
        off = acc & 127u;
        outpos = acc >> 7;
      }
      if (!special_hit) break;  // (off >= 64)
      // end of block, a code longer than a table's bits, an invalid symbol: this one symbol step by step
      asm volatile("" ::: "memory");  // (keeps the loads below in here)
      const uint32_t b = s.bp + off;
      uint32_t e1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)L->ltab[(uint32_t)s.window(b) & ((1u << TK_LB) - 1u)]);
      if (!e1) e1 = tk_slow_entry(s, b, false);
      if (!e1) { rc = 2; break; }
      uint32_t a = e1 & 15u, ol = 1, d = 0;
      const uint32_t k1 = (e1 >> 4) & 3u;
      if (k1 == TK_BAD) { rc = 4; break; }
      if (k1 == TK_EOB) {
        if (lane == off) vpos = -1;  // (the fast loop marked the lane: it holds no symbol that is stored)
        off += a;
        eob = true;
        break;
      }
      if (k1 == TK_MATCH) {
        const uint32_t x1 = (e1 >> 6) & 15u;
        ol = (e1 >> 10) + ((uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(s.window(b + a))) & ((1u << x1) - 1u));
        a += x1;
        uint32_t f2 = (uint32_t)__builtin_amdgcn_readfirstlane((int)L->dtab[(uint32_t)s.window(b + a) & ((1u << TK_DB) - 1u)]);
        if (!f2) f2 = tk_slow_entry(s, b + a, true);
        if (!f2 || ((f2 >> 4) & 3u) == TK_BAD) { rc = 5; break; }
        const uint32_t l2 = f2 & 15u, b2 = (f2 >> 6) & 15u;
        d = (f2 >> 10) + ((uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(s.window(b + a + l2))) & ((1u << b2) - 1u));
        a += l2 + b2;
      }
      if (lane == off) { kind = k1; val = e1 >> 10; olen = ol; dist = d; vpos = (int)outpos; }  // (the lane at this offset stores it with the others)
      outpos += ol;
      off += a;
    }
    if (rc) return rc;
    if (outpos > s.out_len) return 3;
    if (s.bp + off > s.in_bits) return 1;
    // the lanes on the chain: literal to its place, match to the token list
    const bool on = vpos >= 0;
    const bool mat = on && kind == TK_MATCH;
    if (on && kind == TK_LIT) s.out[(uint32_t)vpos] = (uint8_t)val;
    const unsigned long long mb = __ballot(mat);
    if (mat) {
      const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(mb >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mb, 0u));
      s.tokens[s.ntok + rank] = make_uint2((uint32_t)vpos | (olen << 16), dist);
    }
    if (__ballot(mat && dist > (uint32_t)vpos)) return 6;
    s.ntok += (uint32_t)__popcll(mb);
    s.out_at = outpos;
    s.bp += off;
    if (eob) return 0;
  }
}
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(6, 8))) void k_bgzf_tokens(const uint8_t *__restrict__ cdata, const BgzfBlk *__restrict__ blk, uint32_t n_blk, uint8_t *__restrict__ raw,
                                                    uint2 *__restrict__ tokens, uint32_t *__restrict__ ntok_out, uint32_t *err) {
  __shared__ __attribute__((aligned(16))) TokLds L;
  const uint32_t lane = threadIdx.x;
  const BgzfBlk B = blk[blockIdx.x];
  TokInflater s{&L, cdata + B.in_off, B.in_len, B.in_len * 8u, 0, 0, B.out_len, 0, raw + B.out_off, tokens + (size_t)blockIdx.x * TOK_STRIDE, 0};
  int rc = 0, last;
  do {
    last = (int)s.bits(1);
    const int type = (int)s.bits(2);
    if (s.bp > s.in_bits) { rc = 1; break; }
    if (type == 0) {  // stored: on to a byte boundary, LEN, NLEN, the bytes - from HBM straight to the output
      s.bp = (s.bp + 7u) & ~7u;
      const uint32_t len = s.bits(16), nlen = s.bits(16);
      if (s.bp > s.in_bits) { rc = 1; break; }
      if (len != (~nlen & 0xFFFFu)) { rc = 7; break; }
      if (s.out_at + len > s.out_len) { rc = 3; break; }
      const uint32_t pos = s.bp >> 3;
      if (pos + len > s.in_len) { rc = 1; break; }
      for (uint32_t k = lane; k < len; k += 64u) s.out[s.out_at + k] = s.in[pos + k];
      s.out_at += len;
      s.bp += len * 8u;
      // the ring starts over at the half the reader stands in (feed() brings it and the next one)
      if ((s.bp >> 3) + TK_HALF > s.loaded + TK_HALF) s.loaded = (s.bp >> 3) & ~(uint32_t)(TK_HALF - 1);
    } else if (type == 1) {  // fixed codes
      for (uint32_t sym = lane; sym < 288; sym += 64) L.lengths[sym] = sym < 144 ? 8 : (sym < 256 ? 9 : (sym < 280 ? 7 : 8));
      __syncthreads();
      tok_huff_build(&L, L.lcount, L.lsym, L.lengths, 288, L.ltab, TK_LB, 1);
      if (lane < 30) L.lengths[lane] = 5;
      __syncthreads();
      tok_huff_build(&L, L.dcount, L.dsym, L.lengths, 30, L.dtab, TK_DB, 2);
      rc = tok_codes(s);
    } else if (type == 2) {  // dynamic codes
      const int nlen = (int)s.bits(5) + 257, ndist = (int)s.bits(5) + 1, ncode = (int)s.bits(4) + 4;
      if (s.bp > s.in_bits) { rc = 1; break; }
      if (nlen > 286 || ndist > 30) { rc = 8; break; }
      if (lane < 19) L.lengths[lane] = 0;
      __syncthreads();
      for (int index = 0; index < ncode; index++) {
        const uint32_t v = s.bits(3);
        if (lane == 0) L.lengths[INF_ORDER[index]] = (uint8_t)v;
      }
      __syncthreads();
      if (tok_huff_build(&L, L.lcount, L.lsym, L.lengths, 19, L.ltab, 7, 0) != 0) { rc = 9; break; }
      int index = 0;
      uint32_t prev = 0;
      while (index < nlen + ndist) {
        const int symbol = s.cl_symbol();
        if (symbol < 0 || s.bp > s.in_bits) { rc = 2; break; }
        if (symbol < 16) {
          if (lane == 0) L.lengths[index] = (uint8_t)symbol;
          prev = (uint32_t)symbol;
          index++;
        } else {
          uint32_t len = 0;
          int rep;
          if (symbol == 16) {
            if (index == 0) { rc = 10; break; }
            len = prev;
            rep = 3 + (int)s.bits(2);
          } else if (symbol == 17) rep = 3 + (int)s.bits(3);
          else rep = 11 + (int)s.bits(7);
          if (index + rep > nlen + ndist) { rc = 11; break; }
          if ((int)lane < rep) L.lengths[index + lane] = (uint8_t)len;
          if ((int)lane + 64 < rep) L.lengths[index + lane + 64] = (uint8_t)len;
          if ((int)lane + 128 < rep) L.lengths[index + lane + 128] = (uint8_t)len;
          index += rep;
          prev = len;
        }
      }
      if (rc) break;
      if (s.bp > s.in_bits) { rc = 1; break; }
      __syncthreads();
      if (L.lengths[256] == 0) { rc = 12; break; }
      int e = tok_huff_build(&L, L.dcount, L.dsym, L.lengths + nlen, ndist, L.dtab, TK_DB, 2);
      if (e && (e < 0 || ndist != (int)L.dcount[0] + (int)L.dcount[1])) { rc = 14; break; }
      e = tok_huff_build(&L, L.lcount, L.lsym, L.lengths, nlen, L.ltab, TK_LB, 1);
      if (e && (e < 0 || nlen != (int)L.lcount[0] + (int)L.lcount[1])) { rc = 13; break; }
      rc = tok_codes(s);
    } else rc = 15;
  } while (!rc && !last);
  if (!rc && s.out_at != s.out_len) rc = 16;  // ISIZE promised another number of bytes
  if (lane == 0) {
    if (rc) atomicOr(&err[0], 1u);
    ntok_out[blockIdx.x] = rc ? 0u : s.ntok;
  }
  (void)n_blk;
}

// phase B: see above.  One workgroup of 1024 threads per block around the parents of its (at most 65536) output bytes; then the block's
// CRC-32 while its bytes are in the L2: 64 bytes per thread, four bytes per step (tables of the CRC of a byte 0..3 positions further on -
// four independent look-ups instead of four dependent ones), the partial CRCs shifted to their place by x^(8 * bytes behind) mod p.
__global__ __launch_bounds__(RES_THREADS) void k_bgzf_resolve(const BgzfBlk *__restrict__ blk, uint8_t *__restrict__ raw, const uint2 *__restrict__ tokens,
                                                            const uint32_t *__restrict__ ntok_in, CrcPow pw, uint32_t n_common, const uint32_t *__restrict__ pow_common, uint32_t *err) {
  extern __shared__ __attribute__((aligned(16))) uint16_t parent[];  // [65536]
  __shared__ uint32_t s_crc, T[4 * 256];  // the CRC's tables: of a byte 0 .. 3 positions further on
  const uint32_t nt = ntok_in[blockIdx.x];
  const BgzfBlk B = blk[blockIdx.x];
  uint8_t *out = raw + B.out_off;
  const uint32_t n = B.out_len, t = threadIdx.x;
  if (nt) {  // (0: nothing but literals and stored bytes - or the block did not inflate: reported by phase A)
    // every byte its own parent (eight entries per store; entries behind n are never read)
    for (uint32_t j = t * 8u; j < n; j += RES_THREADS * 8u) {
      const uint32_t a = j | ((j + 1u) << 16), two = 0x00020002u;
      *reinterpret_cast<uint4 *>(&parent[j]) = make_uint4(a, a + two, a + 2u * two, a + 3u * two);
    }
    __syncthreads();
    const uint2 *tk = tokens + (size_t)blockIdx.x * TOK_STRIDE;
    for (uint32_t k = t; k < nt; k += RES_THREADS) {
      const uint2 tok = tk[k];
      // (a match that overlaps itself repeats the `dist` bytes in front of it: every byte points into that first period, not at the byte
      // `dist` in front of it - a run of one byte is then one step deep instead of as deep as it is long)
      const uint32_t p = tok.x & 0xFFFFu, len = tok.x >> 16, dist = tok.y, src = p - dist;
      for (uint32_t i = 0, o = 0; i < len; i++) {
        parent[p + i] = (uint16_t)(src + o);
        o = o + 1u == dist ? 0u : o + 1u;
      }
    }
    __syncthreads();
    // pointer jumping: a byte of a match points at a byte in front of it; a byte is done when it points at a literal (a byte that points
    // at itself).  Each thread keeps the bytes it still has to move as a bit mask (byte t + 1024 k: bit k): after the first rounds few are
    // left, and a round costs what is left (round 6: all bytes in every round took 3/4 of this kernel's time).
    unsigned long long todo = 0;
    for (uint32_t k = 0, j = t; j < n; k++, j += RES_THREADS)
      if (parent[j] != (uint16_t)j) todo |= 1ull << k;
    // (no barrier between the rounds: a pointer only ever moves towards the literal - a match copies from in front of it -, so a wave
    // that reads another wave's half-finished pointers reads ancestors all the same and finishes its own bytes at its own pace)
    while (todo) {
      for (unsigned long long m = todo; m; m &= m - 1ull) {
        const uint32_t k = (uint32_t)__builtin_ctzll(m), j = t + k * RES_THREADS;
        const uint16_t q = parent[j], r = parent[q];
        if (r != q) parent[j] = r;
        else todo &= ~(1ull << k);
      }
    }
    __syncthreads();
  }
  // ONE pass fills the matches in and takes the CRC: a thread owns 64 consecutive bytes; per four of them the word as phase A left it
  // (literals in place), their four parents from LDS, the bytes of the matches from the literals they point at (a literal is never
  // written here: no order to keep), the word back if it changed, the word into the CRC.  (Rounds before: a gather over all bytes, then
  // the CRC's own pass over them.)
  if (t < 256) {
    uint32_t c = t;
    for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ BGZF_POLY : c >> 1;
    T[t] = c;
  }
  if (t == 0) s_crc = 0;
  __syncthreads();
  if (t < 256) {
    uint32_t c = T[t];
    for (int k = 1; k < 4; k++) { c = (c >> 8) ^ T[c & 0xFFu]; T[k * 256 + t] = c; }
  }
  __syncthreads();
  const uint32_t lo = t * 64u < n ? t * 64u : n, hi = lo + 64u < n ? lo + 64u : n;
  if (hi > lo) {
    uint32_t c = 0xFFFFFFFFu, k = lo;
    for (; k + 4u <= hi; k += 4u) {
      uint32_t w;
      __builtin_memcpy(&w, out + k, 4);
      if (nt) {
        const uint2 p4 = *reinterpret_cast<const uint2 *>(&parent[k]);  // (k is a multiple of 4: aligned)
        const uint32_t q0 = p4.x & 0xFFFFu, q1 = p4.x >> 16, q2 = p4.y & 0xFFFFu, q3 = p4.y >> 16;
        const uint32_t b0 = q0 != k ? out[q0] : w & 0xFFu, b1 = q1 != k + 1u ? out[q1] : (w >> 8) & 0xFFu, b2 = q2 != k + 2u ? out[q2] : (w >> 16) & 0xFFu,
                       b3 = q3 != k + 3u ? out[q3] : w >> 24;
        const uint32_t v = b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
        if (v != w) { __builtin_memcpy(out + k, &v, 4); w = v; }
      }
      c ^= w;
      c = T[768 + (c & 0xFFu)] ^ T[512 + ((c >> 8) & 0xFFu)] ^ T[256 + ((c >> 16) & 0xFFu)] ^ T[c >> 24];
    }
    for (; k < hi; k++) {
      uint32_t byte = out[k];
      if (nt) { const uint32_t q = parent[k]; if (q != k) { byte = out[q]; out[k] = (uint8_t)byte; } }
      c = T[(c ^ byte) & 0xFFu] ^ (c >> 8);
    }
    c ^= 0xFFFFFFFFu;
    atomicXor(&s_crc, crc_mulmod(n == n_common ? pow_common[t] : crc_x8n(pw, n - hi), c));
  }
  __syncthreads();
  if (t == 0 && s_crc != B.crc) atomicOr(&err[0], 2u);
}
// x^(8 * bytes behind thread t's 64 bytes) mod p for a block of n bytes: the same for every block of that length (nearly all of a file)
__global__ __launch_bounds__(RES_THREADS) void k_crc_pow_common(uint32_t n, CrcPow pw, uint32_t *__restrict__ out) {
  const uint32_t t = threadIdx.x, lo = t * 64u < n ? t * 64u : n, hi = lo + 64u < n ? lo + 64u : n;
  out[t] = crc_x8n(pw, n - hi);
}

// One inflate piece: as many of the n blocks from `blocks` on (places as bgzf_parse left them) as the token scratch holds are inflated
// to c->raw + raw0 + out_off.  Everything is queued; what the decoder found is in piece->res->inflate for the first scan piece's
// read-back.  Every size and offset is bgzf_plan.hpp's.
int bgzf_inflate_piece(elp_ctx *c, const uint8_t *bgzf, const BgzfBlk *blocks, size_t n, uint64_t raw0, CopyEvents &copied, BgzfPiece *piece) {
  hipStream_t st = c->stream;
  // (a failed allocation leaves its text in c->err: the text that was there comes back when a smaller launch finds its scratch)
  uint2 *tok = nullptr;
  const std::string err_before = c->err;
  const BgzfTokFit fit = bgzf_tok_fit(n, c->tune.bgzf_tok_fail_above, [&](size_t nt) { return scratch(c, 7, BgzfScratch7(nt).elems, &tok) == 0; });
  if (!fit.nt) return fit.pretended ? set_error(c, ELP_ERR_HIP, "elp_stage_bgzf: no device memory for the decoder's token scratch") : ELP_ERR_HIP;
  if (fit.nt != n) (void)hipGetLastError();  // (a smaller launch found its scratch: the failed allocations are no error)
  c->err = err_before;
  const uint32_t na = (uint32_t)fit.nt;
  const uint64_t in_lo = blocks[0].in_off, in_hi = blocks[na - 1].in_off + blocks[na - 1].in_len;
  uint8_t *d_in;
  ELP_TRY(scratch(c, 5, (size_t)(in_hi - in_lo) + 64, &d_in));
  if (!c->copy_stream) ELP_HIP(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
  ELP_TRY(copied.fence(c, st, c->copy_stream));  // (what is queued on the stream may still read the buffer the copies are about to overwrite)
  std::vector<BgzfBlk> &tb = piece->tb;
  tb.assign(blocks, blocks + na);
  for (auto &t : tb) { t.in_off -= in_lo; t.out_off += raw0; }
  const BgzfScratch6 L6(na);
  uint64_t *wk;
  ELP_TRY(scratch(c, 6, L6.words64, &wk));
  uint32_t *wk32 = reinterpret_cast<uint32_t *>(wk);
  BgzfBlk *d_blk = reinterpret_cast<BgzfBlk *>(wk);
  piece->na = na;
  piece->blk = d_blk;
  piece->entry = wk + L6.entry;
  piece->exit = wk + L6.exit;
  piece->res = reinterpret_cast<BgzfRes *>(wk + L6.res);
  piece->cnt = wk32 + L6.cnt;
  piece->base = wk32 + L6.base;
  piece->bad_list = wk32 + L6.bad_list;
  piece->inflate_checked = false;
  ELP_HIP(c, hipMemcpyAsync(d_blk, tb.data(), (size_t)na * sizeof(BgzfBlk), hipMemcpyHostToDevice, st));
  ELP_HIP(c, hipMemsetAsync(piece->res, 0, BgzfRes::CLEAR_PIECE, st));
  uint32_t *ierr = &piece->res->inflate;
  // the bit stream first (literals placed, matches as tokens), then the matches and the CRC, a workgroup per block
  const BgzfScratch7 L7(na);
  uint32_t *ntok = reinterpret_cast<uint32_t *>(tok + L7.ntok), *pow_common = ntok + L7.pow_common;
  const uint32_t n_common = bgzf_common_len(tb.data(), na);
  const CrcPow &pw = crc_pow();
  ELP_LAUNCH(c, "stage_bgzf_crc_pow", k_crc_pow_common, dim3(1), dim3(RES_THREADS), 0, n_common, pw, pow_common);
  ELP_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void *>(&k_bgzf_resolve), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(65536 * sizeof(uint16_t))));
  const BgzfChunks chunks(na, c->tune.bgzf_copy_chunk, c->tune.bgzf_first_chunk_div, c->n_cu);
  elp_ctx *lane = nullptr;
  if (chunks.lane) ELP_TRY(side_lane(c, 1, &lane));
  for (const BgzfChunks::Turn &q : chunks.turns) {
    const uint64_t lo = tb[q.q0].in_off, hi = tb[q.q1 - 1].in_off + tb[q.q1 - 1].in_len;
    ELP_HIP(c, hipMemcpyAsync(d_in + lo, bgzf + in_lo + lo, (size_t)(hi - lo), hipMemcpyHostToDevice, c->copy_stream));
    elp_ctx *on = q.side ? lane : c;
    ELP_TRY(copied.arrived(c, c->copy_stream, on->stream));
    ELP_LAUNCH(on, "stage_bgzf_tokens", k_bgzf_tokens, dim3(q.q1 - q.q0), dim3(64), (size_t)c->tune.bgzf_tok_lds, (const uint8_t *)d_in, (const BgzfBlk *)d_blk + q.q0, q.q1 - q.q0,
               c->raw.p, tok + (size_t)q.q0 * TOK_STRIDE, ntok + q.q0, ierr);
  }
  if (lane) ELP_TRY(side_join(c, 1));
  ELP_LAUNCH(c, "stage_bgzf_resolve", k_bgzf_resolve, dim3(na), dim3(RES_THREADS), 65536 * sizeof(uint16_t), (const BgzfBlk *)d_blk, c->raw.p, (const uint2 *)tok,
             (const uint32_t *)ntok, pw, n_common, (const uint32_t *)pow_common, ierr);
  return 0;
}

}  // namespace elp
