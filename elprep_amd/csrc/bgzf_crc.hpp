// bgzf_crc.hpp — the CRC-32 (IEEE, reflected 0xEDB88320) algebra both halves of BGZF use: a block's CRC is computed by the workgroup
// that writes (bgzf_out.hip) or inflates (bgzf_inflate.hip) it, every thread its part of the bytes by table, the parts combined by
// multiplication with x^(8 * bytes behind the part) modulo the polynomial (the algebra of zlib's crc32_combine).
#pragma once
#include <cstdint>

namespace elp {

constexpr uint32_t BGZF_POLY = 0xEDB88320u;

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
inline CrcPow crc_pow_table() {
  CrcPow t;
  uint32_t p = 1u << 30;  // x^1
  t.x2n[0] = p;
  for (int k = 1; k < 32; k++) t.x2n[k] = p = crc_mulmod(p, p);
  return t;
}
inline const CrcPow &crc_pow() {  // the table, computed once (the kernels take it by value)
  static const CrcPow t = crc_pow_table();
  return t;
}
// x^(8 n) mod p
__device__ inline uint32_t crc_x8n(const CrcPow &t, uint32_t n) {
  uint32_t p = 1u << 31;
  for (int k = 3; n; n >>= 1, k++)
    if (n & 1u) p = crc_mulmod(t.x2n[k & 31], p);
  return p;
}

}  // namespace elp
