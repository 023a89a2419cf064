// bgzf_out.hip — BGZF on the device, the writer: the blocks of a BAM file written from HBM.
//
// Reference: utils/bgzf/bgzf-files.go.  Writer (:324-383): every block is a gzip member with the 6-byte "BC" extra field that holds
// the block's size, a raw DEFLATE stream, the CRC-32 of the uncompressed bytes and their number; the file ends with the 28-byte empty
// block (:53-62); a block carries at most 65280 bytes so that its size fits the BC field.  What is written here is DEFLATE with each
// block's own (dynamic) Huffman codes (k_bgzf_deflate); `elp_set_tuning` forces fixed codes only ("bgzf_fixed") or DEFLATE *stored*
// blocks (BTYPE 00, RFC 1951 3.2.4: "bgzf_stored", k_bgzf_frame).  Every form is valid BGZF that every reader inflates, byte-identical
// after inflation to what the reference writes (parity of a BAM file is defined on the inflated stream).
// The CRC-32 of a block is computed by the workgroup that writes it (bgzf_crc.hpp).
#include "common.hpp"
#include "bgzf_crc.hpp"
#include "bgzf_plan.hpp"
#include "deflate_core.hpp"

namespace elp {

static_assert(BGZF_PAYLOAD == dfl::PAYLOAD && dfl::NT * dfl::PART == dfl::PAYLOAD, "one BGZF block = 256 parts of 255 bytes");

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

// frames n_bytes of `raw` (device, 16-byte aligned) into `out` (device, bgzf_framed_size(n_bytes) bytes, bgzf_plan.hpp): full blocks are PAYLOAD +
// OVERHEAD bytes apart, the last one is short
int bgzf_frame(elp_ctx *c, const uint8_t *raw, uint64_t n_bytes, uint8_t *out) {
  if (!n_bytes) return 0;
  const CrcPow &pw = crc_pow();
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
  const CrcPow &pw = crc_pow();
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

}  // namespace elp
