// bgzf.hip — BGZF on the device: the blocks of a BAM file written from HBM, and inflated in HBM.
//
// Reference: utils/bgzf/bgzf-files.go.  Writer (:324-383): every block is a gzip member with the 6-byte "BC" extra field that holds
// the block's size, a raw DEFLATE stream, the CRC-32 of the uncompressed bytes and their number; the file ends with the 28-byte empty
// block (:53-62); a block carries at most 65280 bytes so that its size fits the BC field.  What is written here is DEFLATE with each
// block's own (dynamic) Huffman codes (k_bgzf_deflate); `elp_set_tuning` forces fixed codes only ("bgzf_fixed") or DEFLATE *stored*
// blocks (BTYPE 00, RFC 1951 3.2.4: "bgzf_stored", k_bgzf_frame).  Every form is valid BGZF that every reader inflates, byte-identical
// after inflation to what the reference writes (parity of a BAM file is defined on the inflated stream).
// The CRC-32 (IEEE, reflected 0xEDB88320) of a block is computed by the workgroup that writes it: every thread its part of the bytes by
// table, the parts combined by multiplication with x^(8 * bytes behind the part) modulo the polynomial (the algebra of zlib's
// crc32_combine).
#include "common.hpp"
#include "deflate_core.hpp"
#include <atomic>

namespace elp {

constexpr uint32_t BGZF_PAYLOAD = 65280, BGZF_OVERHEAD = 31, BGZF_POLY = 0xEDB88320u;
static_assert(BGZF_PAYLOAD == dfl::PAYLOAD && dfl::NT * dfl::PART == dfl::PAYLOAD, "one BGZF block = 256 parts of 255 bytes");

// a(x) * b(x) mod p(x), reflected bit order (bit 31 = x^0)
__host__ __device__ inline uint32_t crc_mulmod(uint32_t a, uint32_t b) {
  uint32_t m = 1u << 31, p = 0;
  for (;;) {
    if (a & m) {
      p ^= b;
      if ((a & (m - 1)) == 0) break;
    }
    m >>= 1;
    b = (b & 1u) ? (b >> 1) ^ BGZF_POLY : b >> 1;
  }
  return p;
}
struct CrcPow { uint32_t x2n[32]; };  // x^(2^k) mod p
static CrcPow crc_pow_table() {
  CrcPow t;
  uint32_t p = 1u << 30;  // x^1
  t.x2n[0] = p;
  for (int k = 1; k < 32; k++) t.x2n[k] = p = crc_mulmod(p, p);
  return t;
}
// x^(8 n) mod p
__device__ inline uint32_t crc_x8n(const CrcPow &t, uint32_t n) {
  uint32_t p = 1u << 31;
  for (int k = 3; n; n >>= 1, k++)
    if (n & 1u) p = crc_mulmod(t.x2n[k & 31], p);
  return p;
}

// one workgroup per block: out[blk * (PAYLOAD + OVERHEAD) ...] = header | stored-block header | payload | CRC-32 | ISIZE
__global__ __launch_bounds__(256) void k_bgzf_frame(const uint8_t *__restrict__ raw, uint64_t n_bytes, uint8_t *__restrict__ out, CrcPow pw) {
  __shared__ uint32_t tbl[256];
  __shared__ uint32_t s_crc;
  __shared__ __attribute__((aligned(16))) uint8_t buf[BGZF_PAYLOAD];
  const uint32_t t = threadIdx.x;
  {
    uint32_t c = t;
    for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ BGZF_POLY : c >> 1;
    tbl[t] = c;
  }
  if (t == 0) s_crc = 0;
  const uint64_t at = (uint64_t)blockIdx.x * BGZF_PAYLOAD;
  const uint32_t len = (uint32_t)((n_bytes - at) < (uint64_t)BGZF_PAYLOAD ? (n_bytes - at) : (uint64_t)BGZF_PAYLOAD);
  uint8_t *o = out + (uint64_t)blockIdx.x * (BGZF_PAYLOAD + BGZF_OVERHEAD);
  // payload: through LDS (the CRC reads it from there), 16 bytes per thread and step; `raw` is 16-byte aligned and PAYLOAD a multiple of 16
  for (uint32_t k = t * 16u; k < len; k += 256u * 16u) {
    uint4 v;
    if (k + 16u <= len) v = *reinterpret_cast<const uint4 *>(raw + at + k);
    else {
      uint8_t tmp[16];
      for (uint32_t j = 0; j < 16; j++) tmp[j] = k + j < len ? raw[at + k + j] : (uint8_t)0;
      __builtin_memcpy(&v, tmp, 16);
    }
    *reinterpret_cast<uint4 *>(buf + k) = v;
    if (k + 16u <= len) __builtin_memcpy(o + 23 + k, &v, 16);
    else
      for (uint32_t j = 0; k + j < len; j++) o[23 + k + j] = buf[k + j];
  }
  __syncthreads();
  // CRC-32 of the thread's part [lo, hi), then its place in the block's polynomial
  const uint32_t lo = t * 255u < len ? t * 255u : len, hi = lo + 255u < len ? lo + 255u : len;
  if (hi > lo) {
    uint32_t c = 0xFFFFFFFFu;
    for (uint32_t k = lo; k < hi; k++) c = tbl[(c ^ buf[k]) & 0xFFu] ^ (c >> 8);
    c ^= 0xFFFFFFFFu;
    atomicXor(&s_crc, crc_mulmod(crc_x8n(pw, len - hi), c));
  }
  __syncthreads();
  if (t == 0) {
    const uint32_t total = len + BGZF_OVERHEAD, crc = s_crc;
    const uint8_t head[23] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, (uint8_t)((total - 1) & 0xFF), (uint8_t)((total - 1) >> 8),
                              0x01, (uint8_t)(len & 0xFF), (uint8_t)(len >> 8), (uint8_t)(~len & 0xFF), (uint8_t)((~len >> 8) & 0xFF)};
    for (int k = 0; k < 23; k++) o[k] = head[k];
    uint8_t *tail = o + 23 + len;
    for (int k = 0; k < 4; k++) { tail[k] = (uint8_t)(crc >> (8 * k)); tail[4 + k] = (uint8_t)(len >> (8 * k)); }
  }
}

uint64_t bgzf_framed_size(uint64_t n_bytes) { return n_bytes + (uint64_t)BGZF_OVERHEAD * ((n_bytes + BGZF_PAYLOAD - 1) / BGZF_PAYLOAD); }

// frames n_bytes of `raw` (device, 16-byte aligned) into `out` (device, bgzf_framed_size(n_bytes) bytes): full blocks are PAYLOAD +
// OVERHEAD bytes apart, the last one is short
int bgzf_frame(elp_ctx *c, const uint8_t *raw, uint64_t n_bytes, uint8_t *out) {
  if (!n_bytes) return 0;
  static const CrcPow pw = crc_pow_table();
  const uint64_t nblk = (n_bytes + BGZF_PAYLOAD - 1) / BGZF_PAYLOAD;
  ELP_LAUNCH(c, "emit_bgzf_frame", k_bgzf_frame, dim3((unsigned)nblk), dim3(256), 0, raw, n_bytes, out, pw);
  return 0;
}


// ------------------------------------------------------------------ the compressing writer
// Reference: utils/bgzf/bgzf-files.go:324-383 compresses every block with compress/flate.  Here: a workgroup per block, DEFLATE with the
// block's own Huffman codes (fixed codes where those are not longer, and everywhere under the tuning key "bgzf_fixed")
// over a parallel LZ77 parse (deflate_core.hpp has the algorithm and every function that decides a bit; this kernel is its
// phases with barriers between them).  A block's member (18-byte header | DEFLATE data | CRC-32 | ISIZE) lands in a slot of fixed stride;
// the members' sizes differ, so a second kernel moves them together behind a scan of the sizes.  A block that would not shrink is stored.
constexpr uint32_t BGZF_SLOT = 65344;  // bytes between two slots (>= PAYLOAD + OVERHEAD, a multiple of 64)
constexpr uint32_t DFL_LD = dfl::PAYLOAD + 256;  // words of match notes / tokens per workgroup
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_bgzf_deflate(const uint8_t *__restrict__ raw, uint64_t n_bytes, uint32_t nblk, uint8_t *__restrict__ slots,
                                                      uint32_t *__restrict__ sizes, uint32_t *__restrict__ ld_all, CrcPow pw, int fixed_only) {
  using namespace dfl;
  __shared__ uint32_t s_crc, s_wsum[4];
  __shared__ __attribute__((aligned(16))) uint16_t table[(size_t)WAYS << HBITS];
  __shared__ __attribute__((aligned(16))) uint8_t buf[PAYLOAD + IN_PAD];  // the block's payload; behind the parse: its DEFLATE data
  // (81.7 KB: two workgroups per CU.  The CRC's byte table lives in the hash table's place: the CRC is taken before the table is cleared)
  static_assert(sizeof(table) + sizeof(buf) + 64 <= 81920, "two workgroups per CU");
  uint32_t *tbl = reinterpret_cast<uint32_t *>(table);
  const uint32_t t = threadIdx.x;
  uint32_t *ld = ld_all + (size_t)blockIdx.x * DFL_LD;
  uint32_t *words = reinterpret_cast<uint32_t *>(buf);
  for (uint32_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const uint64_t at = (uint64_t)blk * PAYLOAD;
    const uint32_t len = (uint32_t)((n_bytes - at) < (uint64_t)PAYLOAD ? (n_bytes - at) : (uint64_t)PAYLOAD);
    // ---- the payload into LDS (`raw` is 16-byte aligned and PAYLOAD a multiple of 16), zeros behind it; an empty table
    for (uint32_t k = t * 16u; k < PAYLOAD + IN_PAD; k += 256u * 16u) {
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (k + 16u <= len) v = *reinterpret_cast<const uint4 *>(raw + at + k);
      else if (k < len) {
        uint8_t tmp[16];
        for (uint32_t j = 0; j < 16; j++) tmp[j] = k + j < len ? raw[at + k + j] : (uint8_t)0;
        __builtin_memcpy(&v, tmp, 16);
      }
      *reinterpret_cast<uint4 *>(buf + k) = v;
    }
    {
      uint32_t c = t;
      for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ BGZF_POLY : c >> 1;
      tbl[t] = c;
    }
    if (t == 0) s_crc = 0;
    __syncthreads();
    // ---- CRC-32 of the thread's part [lo, hi), then its place in the block's polynomial (as k_bgzf_frame)
    const uint32_t lo = t * PART < len ? t * PART : len, hi = lo + PART < len ? lo + PART : len;
    if (hi > lo) {
      uint32_t c = 0xFFFFFFFFu;
      for (uint32_t k = lo; k < hi; k++) c = tbl[(c ^ buf[k]) & 0xFFu] ^ (c >> 8);
      c ^= 0xFFFFFFFFu;
      atomicXor(&s_crc, crc_mulmod(crc_x8n(pw, len - hi), c));
    }
    __syncthreads();
    for (uint32_t k = t; k < ((uint32_t)WAYS << HBITS); k += 256u) table[k] = NOPOS;
    __syncthreads();
    // ---- 1. match finding, a strip of 256 positions at a time: look-ups against everything in front of the strip, then its inserts
    for (uint32_t base = 0; base < len; base += 256u) {
      const uint32_t i = base + t;
      const uint32_t w = i < len ? load4(buf + i) : 0u;
      if (i < len) ld[i] = find_match(buf, len, i, table, w);
      __syncthreads();
      if (i < len) table_insert(table, len, i, w);
      __syncthreads();
    }
    // ---- 2. the parse of the thread's part: tokens in place of the notes, their bits
    DynCodes &D = *reinterpret_cast<DynCodes *>(table);  // (the hash table's LDS is free from here on: deflate_core.hpp, dynamic codes)
    static_assert(sizeof(DynCodes) <= sizeof(table), "the codes' tables live where the hash table was");
    for (uint32_t k = t; k < 320u; k += 256u) { D.freq[k] = 0u; D.len[k] = 0; }
    if (t < 2u) { D.m[t] = 0u; D.over[t] = 0u; }
    if (t < 34u) D.cnt[t / 17u][t % 17u] = 0u;
    __syncthreads();
    uint32_t my_bits = 0;
    uint32_t *freq = D.freq;
    const uint32_t my_tok = parse_part(buf, ld, lo, hi, &my_bits, [freq](uint32_t sy) { atomicAdd(&freq[sy], 1u); });
    // ---- 3. bit offsets: exclusive scan over the 256 parts
    uint32_t incl = my_bits;
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t v = __shfl_up(incl, d, 64);
      if ((int)(t & 63u) >= d) incl += v;
    }
    if ((t & 63u) == 63u) s_wsum[t >> 6] = incl;
    __syncthreads();  // (also: every thread is through with the payload in `buf`, the CRC is complete)
    uint32_t off = 0;
    for (uint32_t w = 0; w < (t >> 6); w++) off += s_wsum[w];
    uint32_t my_off = off + incl - my_bits;
    uint32_t total_bits = s_wsum[0] + s_wsum[1] + s_wsum[2] + s_wsum[3];
    uint32_t cbytes = deflate_bytes(total_bits);
    // ---- 3b. dynamic codes (deflate_core.hpp: count | rank | build | codes | header | bits); the hash table's LDS is free by now
    bool dynamic = false;
    if (!fixed_only) {
      if (t == 0) atomicAdd(&D.freq[256], 1u);
      __syncthreads();
      for (uint32_t sy = t; sy < (uint32_t)NLL; sy += 256u) {
        const int r = symbol_rank(D.freq, NLL, (int)sy);
        if (r >= 0) { D.order[r] = (uint16_t)sy; atomicAdd(&D.m[0], 1u); }
      }
      if (t < (uint32_t)NDIST) {
        const int r = symbol_rank(D.freq + DOFF, NDIST, (int)t);
        if (r >= 0) { D.order[DOFF + r] = (uint16_t)t; atomicAdd(&D.m[1], 1u); }
      }
      __syncthreads();
      const int m0 = (int)D.m[0], m1 = (int)D.m[1];
      if (t == 0 && m0 >= 2) huffman_merge(D.freq, D.order, m0, D.w, D.up);
      if (t == 64 && m1 >= 2) huffman_merge(D.freq + DOFF, D.order + DOFF, m1, D.w + 2 * DOFF, D.up + 2 * DOFF);
      __syncthreads();
      for (int leaf = (int)t; leaf < m0 && m0 >= 2; leaf += 256) {
        uint32_t d = leaf_depth(D.up, leaf, m0);
        if (d > 15u) { d = 15u; atomicAdd(&D.over[0], 1u); }
        atomicAdd(&D.cnt[0][d], 1u);
      }
      if ((int)t < m1 && m1 >= 2) {
        uint32_t d = leaf_depth(D.up + 2 * DOFF, (int)t, m1);
        if (d > 15u) { d = 15u; atomicAdd(&D.over[1], 1u); }
        atomicAdd(&D.cnt[1][d], 1u);
      }
      __syncthreads();
      if (t == 0) {
        if (m0 >= 2) limit_counts(D.cnt[0], 15, (int)D.over[0], D.base[0]);
        else trivial_lengths(D.order, m0, NLL, D.len, D.cnt[0], D.base[0]);
      } else if (t == 64) {
        if (m1 >= 2) limit_counts(D.cnt[1], 15, (int)D.over[1], D.base[1]);
        else trivial_lengths(D.order + DOFF, m1, NDIST, D.len + DOFF, D.cnt[1], D.base[1]);
      }
      __syncthreads();
      for (int leaf = (int)t; leaf < m0 && m0 >= 2; leaf += 256) D.len[D.order[leaf]] = (uint8_t)length_of_rank(D.cnt[0], 15, leaf);
      if ((int)t < m1 && m1 >= 2) D.len[DOFF + D.order[DOFF + t]] = (uint8_t)length_of_rank(D.cnt[1], 15, (int)t);
      __syncthreads();
      for (uint32_t sy = t; sy < (uint32_t)NLL; sy += 256u) D.code[sy] = canonical_code(D.len, (int)sy, D.base[0]);
      if (t < (uint32_t)NDIST) D.code[DOFF + t] = canonical_code(D.len + DOFF, (int)t, D.base[1]);
      if (t == 128) build_header(D);  // (reads the lengths only; the other threads count their bits meanwhile)
      uint32_t dyn_bits = 0;
      for (uint32_t j = 0; j < my_tok; j++) dyn_bits += token_bits_dyn(ld[lo + j], D);
      uint32_t dincl = dyn_bits;
      for (int d = 1; d < 64; d <<= 1) {
        const uint32_t v = __shfl_up(dincl, d, 64);
        if ((int)(t & 63u) >= d) dincl += v;
      }
      __syncthreads();  // (s_wsum's readers above are through)
      if ((t & 63u) == 63u) s_wsum[t >> 6] = dincl;
      __syncthreads();
      uint32_t doff = 0;
      for (uint32_t w = 0; w < (t >> 6); w++) doff += s_wsum[w];
      const uint32_t dtotal = s_wsum[0] + s_wsum[1] + s_wsum[2] + s_wsum[3];
      const uint32_t dyn_bytes = deflate_bytes_dyn(D, dtotal);
      if (dyn_bytes < cbytes) {
        dynamic = true;
        cbytes = dyn_bytes;
        total_bits = dtotal;
        my_off = doff + dincl - dyn_bits;
      }
    }
    const bool stored = cbytes >= len + 5u;
    const uint32_t dbytes = stored ? len + 5u : cbytes;  // the member's DEFLATE data
    if (!stored && dynamic) {
      for (uint32_t k = t; k < (cbytes + 3u) / 4u + 1u; k += 256u) words[k] = 0u;
      __syncthreads();
      auto orw = [words](uint32_t w, uint32_t v) { atomicOr(&words[w], v); };
      if (t == 0) {
        BitWriter<decltype(orw)> hw(orw, 0u);
        emit_dyn_header(hw, D);
        hw.finish();
      }
      if (t == 255) {  // the end-of-block code behind the last part's tokens
        BitWriter<decltype(orw)> ew(orw, D.header_bits + total_bits);
        ew.put(D.code[256], D.len[256]);
        ew.finish();
      }
      BitWriter<decltype(orw)> bw(orw, D.header_bits + my_off);
      for (uint32_t j = 0; j < my_tok; j++) emit_token_dyn(bw, ld[lo + j], D);
      bw.finish();
      __syncthreads();
    } else if (!stored) {
      // ---- 4. the codes at their bit offsets, OR-ed into the zeroed words (neighbouring parts share words)
      for (uint32_t k = t; k < (cbytes + 3u) / 4u + 1u; k += 256u) words[k] = 0u;
      __syncthreads();
      auto orw = [words](uint32_t w, uint32_t v) { atomicOr(&words[w], v); };
      if (t == 0) {  // BFINAL = 1, BTYPE = 01
        BitWriter<decltype(orw)> hw(orw, 0u);
        hw.put(3u, 3u);
        hw.finish();
      }
      BitWriter<decltype(orw)> bw(orw, 3u + my_off);
      for (uint32_t j = 0; j < my_tok; j++) emit_token(bw, ld[lo + j]);
      bw.finish();
      // (the end-of-block code is seven zero bits: counted in cbytes, nothing to set)
      __syncthreads();
    }
    // ---- 5. the member into its slot: header | DEFLATE data | CRC-32 | ISIZE
    uint8_t *o = slots + (uint64_t)blk * BGZF_SLOT;
    const uint32_t total = 18u + dbytes + 8u;
    if (t == 0) {
      const uint8_t head[18] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, (uint8_t)((total - 1) & 0xFF), (uint8_t)((total - 1) >> 8)};
      for (int k = 0; k < 18; k++) o[k] = head[k];
      const uint32_t crc = s_crc;
      uint8_t *tail = o + 18 + dbytes;
      for (int k = 0; k < 4; k++) { tail[k] = (uint8_t)(crc >> (8 * k)); tail[4 + k] = (uint8_t)(len >> (8 * k)); }
      sizes[blk] = total;
      if (stored) { o[18] = 0x01; o[19] = (uint8_t)(len & 0xFF); o[20] = (uint8_t)(len >> 8); o[21] = (uint8_t)(~len & 0xFF); o[22] = (uint8_t)((~len >> 8) & 0xFF); }
    }
    if (stored) {
      for (uint32_t k = t; k < len; k += 256u) o[23 + k] = raw[at + k];
    } else {  // (the slot's byte 18 is 2 mod 4: two bytes per store; an odd last byte by itself - the trailer's first byte follows it)
      const uint16_t *src = reinterpret_cast<const uint16_t *>(buf);
      uint16_t *dst = reinterpret_cast<uint16_t *>(o + 18);
      for (uint32_t k = t; k < cbytes / 2u; k += 256u) dst[k] = src[k];
      if ((cbytes & 1u) && t == 255u) o[18 + cbytes - 1u] = buf[cbytes - 1u];
    }
    __syncthreads();  // (the next block's payload overwrites `buf`)
  }
}
// the members of the slots moved together: member b to out + offs[b]
__global__ __launch_bounds__(256) void k_bgzf_compact(const uint8_t *__restrict__ slots, const uint32_t *__restrict__ sizes, const uint32_t *__restrict__ offs,
                                                      uint8_t *__restrict__ out) {
  const uint8_t *s = slots + (uint64_t)blockIdx.x * BGZF_SLOT;
  uint8_t *d = out + offs[blockIdx.x];
  const uint32_t n = sizes[blockIdx.x];
  for (uint32_t k = threadIdx.x; k < n; k += 256u) d[k] = s[k];
}
// compresses n_bytes of `raw` (device, 16-byte aligned) into `out` (device, room for bgzf_framed_size(n_bytes) bytes): BGZF members of
// <= 65280 payload bytes each, behind each other; *out_bytes = their total size
int bgzf_deflate(elp_ctx *c, const uint8_t *raw, uint64_t n_bytes, uint8_t *out, uint64_t *out_bytes) {
  *out_bytes = 0;
  if (!n_bytes) return 0;
  static const CrcPow pw = crc_pow_table();
  const uint64_t nblk = (n_bytes + BGZF_PAYLOAD - 1) / BGZF_PAYLOAD;
  if (nblk >= 0x7FFFFFFFull) return set_error(c, ELP_ERR_UNSUPPORTED, "bgzf_deflate: too many blocks in one pass");
  const unsigned grid = (unsigned)std::min<uint64_t>(nblk, 2ull * (uint64_t)c->n_cu);  // two workgroups per CU (82 KB of LDS each), looping over the blocks
  uint32_t *wk;
  ELP_TRY(scratch(c, 0, (size_t)grid * DFL_LD + 2 * (nblk + 8) + 16, &wk));
  uint32_t *ld_all = wk, *sizes = wk + (size_t)grid * DFL_LD, *offs = sizes + nblk + 8;
  uint8_t *slots;
  ELP_TRY(scratch(c, 1, nblk * BGZF_SLOT + 64, &slots));
  ELP_LAUNCH(c, "emit_bgzf_deflate", k_bgzf_deflate, dim3(grid), dim3(256), 0, raw, n_bytes, (uint32_t)nblk, slots, sizes, ld_all, pw, c->tune.bgzf_fixed);
  uint32_t total = 0;
  ELP_TRY(exclusive_scan_u32(c, sizes, offs, nblk, &total));  // (a pass is below 4 GiB: emit_stream's chunks)
  ELP_LAUNCH(c, "emit_bgzf_compact", k_bgzf_compact, dim3((unsigned)nblk), dim3(256), 0, (const uint8_t *)slots, (const uint32_t *)sizes, (const uint32_t *)offs, out);
  *out_bytes = total;
  return 0;
}


// ------------------------------------------------------------------ inflate (RFC 1951)
// Reference: the reader inflates every block with compress/flate on a worker goroutine (utils/bgzf/bgzf-files.go:164-221) and checks
// its CRC-32.  A BAM file of a 30x genome is a few hundred thousand independent blocks of <= 64 KB.
struct BgzfBlk { uint64_t in_off; uint32_t in_len, out_len; uint64_t out_off; uint32_t crc; uint32_t pad; };  // CDATA in the piece; ISIZE; place in c->raw

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
constexpr uint32_t TOK_STRIDE = 21888;  // tokens per block: >= 65536 / 3 + 1, a multiple of 64
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
constexpr int RES_THREADS = 1024;
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

// ------------------------------------------------------------------ where the alignment records start in the inflated stream
// A reader walks the block_size chain record by record (sam/bam-files.go: one record after the other from the stream); that is one
// dependent load per record - 50 M of them.  Here every inflated block GUESSES its first record start (the first offset at which a
// well-formed record header stands and whose block_size chain stays well-formed for a few records), walks its own records from there
// and reports where its chain leaves the block; the guesses are then PROVEN: the chain that starts at the known first record of the
// stream enters every block exactly at that block's guess iff every block's exit equals the next block's guess - checked for all
// blocks at once.  Where a guess was wrong (a byte pattern that happened to look like a record), one thread repairs the entries in
// order.  The result is exact; the guessing only decides how much runs in parallel.
struct RecScan {
  const uint8_t *raw;
  uint64_t begin, end;  // the stream's bytes in c->raw: the first record of the piece starts at `begin`
  int32_t n_ref;
};
constexpr uint64_t REC_NONE = ~0ull;
__device__ __forceinline__ uint32_t ld32(const uint8_t *p) { uint32_t v; __builtin_memcpy(&v, p, 4); return v; }
// could a record start at p?  (fields of the fixed part, sam/bam-files.go:parseBamAlignment; everything that is checkable inside the data)
__device__ inline bool rec_plausible(const RecScan &r, uint64_t p) {
  if (p + 36 > r.end) return false;
  const uint8_t *q = r.raw + p;
  const uint32_t bs = ld32(q);
  if (bs < 32 || bs > (1u << 28)) return false;
  const int32_t refid = (int32_t)ld32(q + 4), pos = (int32_t)ld32(q + 8), next_refid = (int32_t)ld32(q + 24), next_pos = (int32_t)ld32(q + 28);
  if (refid < -1 || refid >= r.n_ref || next_refid < -1 || next_refid >= r.n_ref || pos < -1 || next_pos < -1) return false;
  const uint32_t l_name = q[12], n_cig = q[16] | ((uint32_t)q[17] << 8), l_seq = ld32(q + 20);
  if (l_name < 1 || l_seq > (1u << 28)) return false;
  const uint64_t need = 32ull + l_name + 4ull * n_cig + (l_seq + 1) / 2 + l_seq;
  if (need > bs) return false;
  const uint64_t nul = p + 36 + l_name - 1;
  if (nul < r.end && r.raw[nul] != 0) return false;
  return true;
}
// per inflated block: first / one-past-last byte in c->raw
__global__ __launch_bounds__(256) void k_rec_guess(RecScan r, const BgzfBlk *__restrict__ blk, uint64_t *__restrict__ guess, int weak) {
  __shared__ unsigned long long s_best;
  const BgzfBlk B = blk[blockIdx.x];
  // (the first block of a piece also owns the bytes in front of it: the record that was pending when the previous piece ended starts there)
  const uint64_t lo = (blockIdx.x == 0 || B.out_off < r.begin) ? r.begin : B.out_off, hi = B.out_off + B.out_len;
  if (threadIdx.x == 0) s_best = (weak && lo < hi) ? lo + (blockIdx.x % 3u) : REC_NONE;  // weak: a guess without a look at the bytes
  __syncthreads();
  for (uint64_t base = lo; !weak && base < hi; base += 256) {
    const uint64_t p = base + threadIdx.x;
    if (p < hi && rec_plausible(r, p)) {
      // the chain must stay plausible for up to three more records (as far as the data at hand goes)
      uint64_t q = p + 4ull + ld32(r.raw + p);
      bool ok = true;
      for (int k = 0; ok && k < 3 && q + 36 <= r.end; k++) {
        ok = rec_plausible(r, q);
        q += 4ull + ld32(r.raw + q);
      }
      if (ok) atomicMin(&s_best, (unsigned long long)p);
    }
    __syncthreads();
    if (s_best != REC_NONE) break;  // (uniform: read behind the barrier)
    __syncthreads();
  }
  if (threadIdx.x == 0) guess[blockIdx.x] = s_best;
}
// the record at p is not complete in the data at hand: it stays pending (the next piece brings the rest)
__device__ __forceinline__ bool rec_incomplete(const RecScan &r, uint64_t p) { return p + 4 > r.end || p + 4ull + ld32(r.raw + p) > r.end; }
// thread per block: the complete records that START in the block, from its entry; exit = where the chain leaves the block, or the first
// record that is not complete in the data.  fill: also writes the starts (second pass)
__device__ inline void rec_walk(const RecScan &r, uint64_t entry, uint64_t hi, uint64_t *exit_out, uint32_t *cnt_out, uint64_t *starts, uint32_t *max_rec) {
  uint64_t p = entry;
  uint32_t cnt = 0, mx = 0;
  while (p < hi) {
    if (rec_incomplete(r, p)) break;
    const uint64_t nx = p + 4ull + ld32(r.raw + p);
    if (starts) starts[cnt] = p;
    cnt++;
    const uint32_t sz = (uint32_t)(nx - p);
    mx = sz > mx ? sz : mx;
    p = nx;
  }
  *exit_out = p;
  *cnt_out = cnt;
  if (max_rec && mx) atomicMax(max_rec, mx);
}
__global__ __launch_bounds__(64) void k_rec_walk(RecScan r, const BgzfBlk *__restrict__ blk, uint32_t n_blk, const uint64_t *__restrict__ entry, uint64_t *__restrict__ exit_,
                                                 uint32_t *__restrict__ cnt) {
  const uint32_t b = blockIdx.x * 64 + threadIdx.x;
  if (b >= n_blk) return;
  const uint64_t hi = blk[b].out_off + blk[b].out_len;
  if (entry[b] == REC_NONE) { exit_[b] = REC_NONE; cnt[b] = 0; return; }
  rec_walk(r, entry[b], hi, &exit_[b], &cnt[b], nullptr, nullptr);
}
constexpr uint32_t REC_BAD_CAP = 1024;  // rejected guesses that are listed (more: the repair goes through all blocks)
// the proof: block b's guess is the true entry iff the nearest block in front of it that has an entry leaves its records exactly there
// (blocks in between hold no record start: the chain jumps over them); the first entry must be the stream's known first record
__global__ __launch_bounds__(256) void k_rec_check(RecScan r, const BgzfBlk *__restrict__ blk, uint32_t n_blk, const uint64_t *__restrict__ entry,
                                                   const uint64_t *__restrict__ exit_, uint32_t *bad, uint32_t *__restrict__ bad_list) {
  const uint32_t b = blockIdx.x * 256 + threadIdx.x;
  if (b >= n_blk) return;
  const uint64_t lo = blk[b].out_off, hi = lo + blk[b].out_len;
  int64_t a = (int64_t)b - 1;
  while (a >= 0 && entry[a] == REC_NONE) a--;
  const uint64_t came = a >= 0 ? exit_[a] : r.begin;  // where the true chain stands when it reaches this block (if everything in front is right)
  bool ok;
  if (entry[b] == REC_NONE) ok = came >= hi || rec_incomplete(r, came);  // no complete record starts here: the chain jumps over the block, or stands at the pending record
  else ok = came == entry[b];
  if (hi <= r.begin) ok = true;  // a block of the header prefix
  (void)lo;
  if (!ok) {
    const uint32_t k = atomicAdd(bad, 1u);
    if (k < REC_BAD_CAP) bad_list[k] = b;
  }
}
// one thread, in order: entries that the proof rejected are replaced by where the chain really arrives.  Only the rejected blocks are
// visited (round 6: the loop over all blocks - a dependent load each - took 15 ms for 19 k blocks because of one wrong guess), each followed
// by the blocks behind it for as long as the repaired chain arrives somewhere else than they assumed.
__device__ inline uint64_t rec_repair_block(const RecScan &r, const BgzfBlk *blk, uint32_t b, uint64_t came, uint64_t *entry, uint64_t *exit_, uint32_t *cnt) {
  const uint64_t hi = blk[b].out_off + blk[b].out_len;
  if (hi <= r.begin) return came;
  const uint64_t want = (came < hi && !rec_incomplete(r, came)) ? came : REC_NONE;
  if (entry[b] != want && !(want == REC_NONE && entry[b] == came)) {  // (an entry at the pending record itself is as good as none)
    entry[b] = want;
    if (want == REC_NONE) { exit_[b] = REC_NONE; cnt[b] = 0; }
    else rec_walk(r, want, hi, &exit_[b], &cnt[b], nullptr, nullptr);
  }
  return entry[b] != REC_NONE ? exit_[b] : came;
}
__global__ void k_rec_repair(RecScan r, const BgzfBlk *__restrict__ blk, uint32_t n_blk, uint64_t *entry, uint64_t *exit_, uint32_t *cnt, const uint32_t *bad,
                             uint32_t *bad_list) {
  const uint32_t n_bad = bad[0];
  if (n_bad > REC_BAD_CAP) {
    uint64_t came = r.begin;
    for (uint32_t b = 0; b < n_blk; b++) came = rec_repair_block(r, blk, b, came, entry, exit_, cnt);
    return;
  }
  for (uint32_t i = 1; i < n_bad; i++) {  // (the list is in the order of the atomics: sort it, it is short)
    const uint32_t v = bad_list[i];
    uint32_t j = i;
    for (; j > 0 && bad_list[j - 1] > v; j--) bad_list[j] = bad_list[j - 1];
    bad_list[j] = v;
  }
  uint32_t done = 0;  // blocks below are consistent with the repaired chain
  for (uint32_t i = 0; i < n_bad; i++) {
    uint32_t b = bad_list[i];
    if (b < done) continue;
    int64_t a = (int64_t)b - 1;
    while (a >= 0 && entry[a] == REC_NONE) a--;
    uint64_t came = a >= 0 ? exit_[a] : r.begin;
    for (;;) {
      came = rec_repair_block(r, blk, b, came, entry, exit_, cnt);
      if (++b >= n_blk) break;
      // does the next block stand as it is?  (k_rec_check's condition, with the chain as it is now)
      const uint64_t hi = blk[b].out_off + blk[b].out_len;
      const bool ok = hi <= r.begin || (entry[b] == REC_NONE ? (came >= hi || rec_incomplete(r, came)) : came == entry[b]);
      if (ok) break;
    }
    done = b;
  }
}
__global__ __launch_bounds__(64) void k_rec_fill(RecScan r, const BgzfBlk *__restrict__ blk, uint32_t n_blk, const uint64_t *__restrict__ entry,
                                                 const uint32_t *__restrict__ base, uint64_t *__restrict__ rec_off, uint32_t *max_rec) {
  const uint32_t b = blockIdx.x * 64 + threadIdx.x;
  if (b >= n_blk || entry[b] == REC_NONE) return;
  uint64_t ex;
  uint32_t cn;
  rec_walk(r, entry[b], blk[b].out_off + blk[b].out_len, &ex, &cn, rec_off + base[b], max_rec);
}
__global__ void k_rec_tail(const uint64_t *__restrict__ entry, const uint64_t *__restrict__ exit_, uint32_t n_blk, uint64_t begin, uint64_t *__restrict__ out /* [0] = end of the last complete record */) {
  uint64_t e = begin;
  for (int64_t b = (int64_t)n_blk - 1; b >= 0; b--)
    if (entry[b] != REC_NONE) { e = exit_[b]; break; }
  out[0] = e;
}


}  // namespace elp

using namespace elp;

// events between the context's stream and its copy stream, destroyed when the call returns (also on an error path)
struct CopyEvents {
  std::vector<hipEvent_t> ev;
  ~CopyEvents() { for (auto e : ev) (void)hipEventDestroy(e); }
  int next(elp_ctx *c, hipEvent_t *out) {
    hipEvent_t e;
    ELP_HIP(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    ev.push_back(e);
    *out = e;
    return 0;
  }
  // `to` waits for everything queued on `from` so far
  int fence(elp_ctx *c, hipStream_t from, hipStream_t to) {
    hipEvent_t e;
    ELP_TRY(next(c, &e));
    ELP_HIP(c, hipEventRecord(e, from));
    ELP_HIP(c, hipStreamWaitEvent(to, e, 0));
    return 0;
  }
  int arrived(elp_ctx *c, hipStream_t copy, hipStream_t st) { return fence(c, copy, st); }
};

// elp_stage_bgzf: see include/elprep_hip.h
extern "C" int elp_stage_bgzf(elp_ctx *c, const uint8_t *bgzf, uint64_t n_bytes, uint64_t first_record, uint16_t split_id) {
  if (!c || (!bgzf && n_bytes)) return ELP_ERR_ARG;
  std::lock_guard<std::mutex> g(c->stage_mu);
  ELP_HIP(c, hipSetDevice(c->device));
  if (!c->have_header) return set_error(c, ELP_ERR_ARG, "elp_stage_bgzf: call elp_set_header first");
  if (c->dict_replaced) return staging_refused_after_replace(c, "elp_stage_bgzf");
  if (c->n_rg && !c->have_rg_ids && !c->replace_rg) return set_error(c, ELP_ERR_ARG, "elp_stage_bgzf: call elp_set_read_group_ids first");
  if (c->n != c->raw_n) return set_error(c, ELP_ERR_ARG, "elp_stage_bgzf: the context already holds records staged with elp_stage");
  // ---- the blocks (host: a few fields per 64 KB; utils/bgzf/bgzf-files.go:95-123)
  std::vector<BgzfBlk> blocks;
  uint64_t p = 0, inflated = 0;
  bool saw_eof = false;
  while (p < n_bytes) {
    if (p + 18 > n_bytes) return set_error(c, ELP_ERR_DATA, "elp_stage_bgzf: truncated block header at byte %llu", (unsigned long long)p);
    const uint8_t *h = bgzf + p;
    if (h[0] != 0x1f || h[1] != 0x8b || h[2] != 8 || !(h[3] & 4)) return set_error(c, ELP_ERR_DATA, "elp_stage_bgzf: not a BGZF block at byte %llu", (unsigned long long)p);
    const uint32_t xlen = h[10] | ((uint32_t)h[11] << 8);
    if (p + 12 + xlen > n_bytes) return set_error(c, ELP_ERR_DATA, "elp_stage_bgzf: truncated extra field at byte %llu", (unsigned long long)p);
    uint32_t bsize = 0;
    for (uint32_t i = 0; i + 4 <= xlen;) {
      const uint32_t slen = h[12 + i + 2] | ((uint32_t)h[12 + i + 3] << 8);
      if (h[12 + i] == 66 && h[12 + i + 1] == 67 && slen == 2 && i + 6 <= xlen) { bsize = (h[12 + i + 4] | ((uint32_t)h[12 + i + 5] << 8)) + 1u; break; }
      i += 4 + slen;
    }
    if (!bsize) return set_error(c, ELP_ERR_DATA, "missing BC extra subfield in BGZF header (block at byte %llu)", (unsigned long long)p);
    if (bsize < 12 + xlen + 8 || p + bsize > n_bytes) return set_error(c, ELP_ERR_DATA, "elp_stage_bgzf: bad block size at byte %llu", (unsigned long long)p);
    uint32_t crc, isize;
    memcpy(&crc, bgzf + p + bsize - 8, 4);
    memcpy(&isize, bgzf + p + bsize - 4, 4);
    if (isize > 65536) return set_error(c, ELP_ERR_DATA, "elp_stage_bgzf: block at byte %llu claims %u inflated bytes", (unsigned long long)p, isize);
    saw_eof = isize == 0;
    if (isize) blocks.push_back(BgzfBlk{p + 12 + xlen, bsize - 12 - xlen - 8, isize, inflated, crc, 0});
    inflated += isize;
    p += bsize;
  }
  (void)saw_eof;  // (the end-of-file block is the host's to insist on: a caller may hand over a file in several calls)
  if (first_record > inflated) return set_error(c, ELP_ERR_ARG, "elp_stage_bgzf: first_record lies behind the inflated data");
  c->derived.records_changed();
  if (blocks.empty()) return 0;
  hipStream_t st = c->stream;
  static const CrcPow pw = crc_pow_table();
  // the inflated stream goes to c->raw behind what is there; the records of the header prefix are never referenced
  const uint64_t raw0 = c->raw_bytes;
  ELP_TRY(ensure(c, c->raw, raw0 + inflated + 64, true, raw0));
  // Two sizes of pieces.  INFLATE pieces (<= 2 GiB inflated: ~33 k blocks) - the decoder wants every block of the file in flight at once (a
  // wave per block, 24 of them per CU: 6.1 k blocks fill the chip once; round 6: 192 MiB pieces left it half empty and cost 1.7x) and pays
  // 171 KB of token scratch per block for it.  Inside one, SCAN pieces (<= 1 GiB: u32 scans and bounded scratch in stage_bam_columns; round 6: 192 MiB pieces cost 7 x 2 host
  // waits and launches of 3 k threads)
  // find the records and stage the columns as before.
  const uint64_t PIECE = (uint64_t)c->tune.bgzf_piece, IPIECE = (uint64_t)c->tune.bgzf_inflate_piece;
  uint64_t begin = raw0 + first_record;  // where the next record starts in c->raw
  size_t b0 = 0, a1 = 0;
  BgzfBlk *d_blk_all = nullptr;
  uint64_t *entry_all = nullptr, *exit_all = nullptr, *res = nullptr;
  uint32_t *cnt_all = nullptr, *base_all = nullptr, *bad_list = nullptr;
  std::vector<BgzfBlk> tb_all;
  CopyEvents copied;
  const uint32_t chunk = c->tune.bgzf_copy_chunk > 0 ? (uint32_t)c->tune.bgzf_copy_chunk : std::max(1024u, (uint32_t)c->n_cu * 24u);
  size_t a0 = 0;
  bool inflate_checked = true;
  while (b0 < blocks.size()) {
    if (b0 == a1) {  // the next inflate piece: compressed bytes + block table to the device, every block inflated
      a0 = a1;
      uint64_t in_lo = blocks[a0].in_off, in_hi = in_lo, out_bytes = 0;
      while (a1 < blocks.size() && (a1 == a0 || out_bytes + blocks[a1].out_len <= IPIECE)) {
        in_hi = blocks[a1].in_off + blocks[a1].in_len;
        out_bytes += blocks[a1].out_len;
        a1++;
      }
      // the decoder's token scratch is 171 KB per block in flight: where the device's free memory does not hold it for the whole piece
      // the launch takes half the blocks, and half of that ... (a part of 2 GiB wants 5.7 GB)
      // (a failed allocation leaves its text in c->err: the text that was there comes back when a smaller launch finds its scratch)
      uint2 *tok = nullptr;
      const std::string err_before = c->err;
      for (;;) {
        const size_t nt = a1 - a0;
        const bool pretend = c->tune.bgzf_tok_fail_above > 0 && nt > (size_t)c->tune.bgzf_tok_fail_above;  // (tests: this path without a full device)
        if (!pretend && scratch(c, 7, nt * TOK_STRIDE + (nt + 2) / 2 + RES_THREADS / 2 + 8, &tok) == 0) break;
        if (nt <= 1) return pretend ? set_error(c, ELP_ERR_HIP, "elp_stage_bgzf: no device memory for the decoder's token scratch") : ELP_ERR_HIP;
        (void)hipGetLastError();
        a1 = a0 + nt / 2;
      }
      c->err = err_before;
      in_hi = blocks[a1 - 1].in_off + blocks[a1 - 1].in_len;
      const uint32_t na = (uint32_t)(a1 - a0);
      uint8_t *d_in;
      ELP_TRY(scratch(c, 5, (size_t)(in_hi - in_lo) + 64, &d_in));
      // the compressed bytes cross PCIe in chunks of blocks on the copy stream, each chunk's decoder launch waits for its own chunk only:
      // the decoder works on chunk k while chunk k + 1 arrives.  A chunk = the blocks that fill the chip once (24 waves per CU).
      if (!c->copy_stream) ELP_HIP(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
      ELP_TRY(copied.fence(c, st, c->copy_stream));  // (what is queued on the stream may still read the buffer the copies are about to overwrite)
      tb_all.assign(blocks.begin() + a0, blocks.begin() + a1);
      for (auto &t : tb_all) { t.in_off -= in_lo; t.out_off += raw0; }
      // block table | entry | exit (u64 each) | result words | cnt | base (u32 each) | list of rejected guesses
      static_assert(sizeof(BgzfBlk) == 32, "BgzfBlk is four 64-bit words");
      uint64_t *wk;
      ELP_TRY(scratch(c, 6, (size_t)na * 6 + 8 + (size_t)(na + 8) + 16 + REC_BAD_CAP / 2, &wk));
      d_blk_all = reinterpret_cast<BgzfBlk *>(wk);
      entry_all = wk + (size_t)na * 4;
      exit_all = entry_all + na;
      res = exit_all + na;
      cnt_all = reinterpret_cast<uint32_t *>(res + 8);
      base_all = cnt_all + na + 8;
      bad_list = base_all + na + 8;
      ELP_HIP(c, hipMemcpyAsync(d_blk_all, tb_all.data(), (size_t)na * sizeof(BgzfBlk), hipMemcpyHostToDevice, st));
      ELP_HIP(c, hipMemsetAsync(res, 0, 64, st));
      uint32_t *ierr = reinterpret_cast<uint32_t *>(res + 4);  // (its own word: the scan pieces clear theirs)
      // the bit stream first (literals placed, matches as tokens), then the matches and the CRC, a workgroup per block
      uint32_t *ntok = reinterpret_cast<uint32_t *>(tok + (size_t)na * TOK_STRIDE), *pow_common = ntok + ((na + 1u) & ~1u);
      uint32_t n_common = tb_all[0].out_len;  // the inflated length most blocks have (majority vote; any value is correct, the common one is fast)
      {
        uint32_t votes = 0;
        for (const auto &t : tb_all) {
          if (votes == 0) { n_common = t.out_len; votes = 1; }
          else if (t.out_len == n_common) votes++;
          else votes--;
        }
      }
      ELP_LAUNCH(c, "stage_bgzf_crc_pow", k_crc_pow_common, dim3(1), dim3(RES_THREADS), 0, n_common, pw, pow_common);
      ELP_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void *>(&k_bgzf_resolve), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(65536 * sizeof(uint16_t))));
      // the chunks' launches alternate between the context's stream and a lane of its own (the sort lane: idle while records are staged):
      // a launch behind another on ONE stream starts when the last wave of the one in front has finished - a block takes 4.5 ms, the chip
      // drains for half of that per launch -; on two streams the next chunk's waves take the slots as they come free
      elp_ctx *lane = nullptr;
      if (na > chunk) ELP_TRY(side_lane(c, 1, &lane));
      uint32_t turn = 0;
      for (uint32_t q0 = 0, q1 = 0; q0 < na; q0 = q1, turn++) {
        q1 = std::min(na, q0 + (turn == 0 ? std::max(1u, chunk / (uint32_t)std::max(1, c->tune.bgzf_first_chunk_div)) : chunk));  // (a small first chunk: the decoder starts early)
        const uint64_t lo = tb_all[q0].in_off, hi = tb_all[q1 - 1].in_off + tb_all[q1 - 1].in_len;
        ELP_HIP(c, hipMemcpyAsync(d_in + lo, bgzf + in_lo + lo, (size_t)(hi - lo), hipMemcpyHostToDevice, c->copy_stream));
        elp_ctx *on = (lane && (turn & 1u)) ? lane : c;
        ELP_TRY(copied.arrived(c, c->copy_stream, on->stream));
        ELP_LAUNCH(on, "stage_bgzf_tokens", k_bgzf_tokens, dim3(q1 - q0), dim3(64), (size_t)c->tune.bgzf_tok_lds, (const uint8_t *)d_in, (const BgzfBlk *)d_blk_all + q0, q1 - q0,
                   c->raw.p, tok + (size_t)q0 * TOK_STRIDE, ntok + q0, ierr);
      }
      if (lane) ELP_TRY(side_join(c, 1));
      ELP_LAUNCH(c, "stage_bgzf_resolve", k_bgzf_resolve, dim3(na), dim3(RES_THREADS), 65536 * sizeof(uint16_t), (const BgzfBlk *)d_blk_all, c->raw.p, (const uint2 *)tok,
                 (const uint32_t *)ntok, pw, n_common, (const uint32_t *)pow_common, ierr);
      inflate_checked = false;
    }
    // the next scan piece, inside the inflate piece
    size_t b1 = b0;
    {
      uint64_t out_bytes = 0;
      while (b1 < a1 && (b1 == b0 || out_bytes + blocks[b1].out_len <= PIECE)) {
        out_bytes += blocks[b1].out_len;
        b1++;
      }
    }
    const uint32_t nb = (uint32_t)(b1 - b0);
    const size_t rel = b0 - a0;
    const BgzfBlk *d_blk = d_blk_all + rel;
    uint64_t *entry = entry_all + rel, *exit_ = exit_all + rel;
    uint32_t *cnt = cnt_all + rel, *base = base_all + rel;
    ELP_HIP(c, hipMemsetAsync(res, 0, 16, st));
    uint32_t *err = reinterpret_cast<uint32_t *>(res), *bad = err + 1, *max_rec = err + 2;
    (void)err;
    const BgzfBlk &last = tb_all[b1 - 1 - a0];
    const uint64_t end = last.out_off + last.out_len;
    const RecScan rs{c->raw.p, begin, end, c->n_ref};
    ELP_LAUNCH(c, "stage_bgzf_guess", k_rec_guess, dim3(nb), dim3(256), 0, rs, (const BgzfBlk *)d_blk, entry, c->tune.bgzf_weak_guess);
    ELP_LAUNCH(c, "stage_bgzf_walk", k_rec_walk, dim3(blocks_for(nb, 64)), dim3(64), 0, rs, (const BgzfBlk *)d_blk, nb, (const uint64_t *)entry, exit_, cnt);
    ELP_LAUNCH(c, "stage_bgzf_check", k_rec_check, dim3(blocks_for(nb, 256)), dim3(256), 0, rs, (const BgzfBlk *)d_blk, nb, (const uint64_t *)entry, (const uint64_t *)exit_, bad, bad_list);
    uint32_t hr[10];
    ELP_HIP(c, hipMemcpyAsync(hr, res, sizeof hr, hipMemcpyDeviceToHost, st));
    ELP_HIP(c, elp::stream_wait(st));
    if (!inflate_checked) {
      if (hr[8] & 1u) return set_error(c, ELP_ERR_DATA, "elp_stage_bgzf: a block does not inflate (corrupt DEFLATE data or wrong ISIZE)");
      if (hr[8] & 2u) return set_error(c, ELP_ERR_DATA, "invalid CRC-32 value for a data block in a BGZF file");
      inflate_checked = true;
    }
    if (hr[1]) ELP_LAUNCH(c, "stage_bgzf_repair", k_rec_repair, dim3(1), dim3(1), 0, rs, d_blk, nb, entry, exit_, cnt, (const uint32_t *)bad, bad_list);
    uint32_t n_rec = 0;
    ELP_TRY(exclusive_scan_u32(c, cnt, base, nb, &n_rec));
    if (c->n + n_rec > 0xFFFFFFF0ull) return set_error(c, ELP_ERR_UNSUPPORTED, "more than 2^32-16 records per context");
    ELP_TRY(ensure(c, c->raw_off, c->n + n_rec + 2, true, c->n + 1));
    ELP_LAUNCH(c, "stage_bgzf_fill", k_rec_fill, dim3(blocks_for(nb, 64)), dim3(64), 0, rs, (const BgzfBlk *)d_blk, nb, (const uint64_t *)entry, (const uint32_t *)base,
               c->raw_off.p + c->n, max_rec);
    ELP_LAUNCH(c, "stage_bgzf_tail", k_rec_tail, dim3(1), dim3(1), 0, (const uint64_t *)entry, (const uint64_t *)exit_, nb, begin, c->raw_off.p + c->n + n_rec);
    uint64_t rec_end = 0;
    ELP_HIP(c, hipMemcpyAsync(&rec_end, c->raw_off.p + c->n + n_rec, 8, hipMemcpyDeviceToHost, st));
    ELP_HIP(c, hipMemcpyAsync(hr, res, sizeof hr, hipMemcpyDeviceToHost, st));
    ELP_HIP(c, elp::stream_wait(st));
    if (rec_end < begin || rec_end > end) return set_error(c, ELP_ERR_DATA, "elp_stage_bgzf: the alignment records do not chain (block_size fields)");
    if (n_rec) ELP_TRY(stage_bam_columns(c, n_rec, rec_end - begin, rec_end, hr[2], split_id));
    begin = rec_end;
    b0 = b1;
  }
  if (begin != raw0 + inflated) return set_error(c, ELP_ERR_DATA, "elp_stage_bgzf: the data ends inside an alignment record (%llu bytes left over)", (unsigned long long)(raw0 + inflated - begin));
  c->raw_bytes = raw0 + inflated;
  return 0;
}

namespace elp {
}  // namespace elp
