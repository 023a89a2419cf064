// bamtag_read.hpp — the pure readers of a BAM record's bytes: little-endian loads and the optional fields' sizes and integer values
// (parseBamAlignment's tag loop, sam/bam-files.go:373-396), as host-and-device code in the manner of samparse.hpp.  bamtag.hpp includes
// it for the kernels; filter_rules.hpp for the strict filter's rule, which the CPU tests compile with the host compiler.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define ELP_TAG_HD __host__ __device__ __forceinline__
#define ELP_TAG_HD_NOFORCE __host__ __device__ inline
#else
#define ELP_TAG_HD inline
#define ELP_TAG_HD_NOFORCE inline
#endif

namespace elp {

ELP_TAG_HD uint32_t ld_u16(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
ELP_TAG_HD uint32_t ld_u32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

// bytes of the value of one optional field of type `t` at p (end = end of the record); 0 = malformed
ELP_TAG_HD_NOFORCE uint32_t tag_value_size(uint8_t t, const uint8_t *p, const uint8_t *end) {
  switch (t) {
    case 'A': case 'c': case 'C': return 1;
    case 's': case 'S': return 2;
    case 'i': case 'I': case 'f': return 4;
    case 'Z': case 'H': {
      uint32_t k = 0;
      while (p + k < end && p[k] != 0) k++;
      return p + k < end ? k + 1 : 0;
    }
    case 'B': {
      if (p + 5 > end) return 0;
      const uint8_t st = p[0];
      const uint32_t cnt = ld_u32(p + 1);
      const uint32_t es = (st == 'c' || st == 'C') ? 1 : ((st == 's' || st == 'S') ? 2 : ((st == 'i' || st == 'I' || st == 'f') ? 4 : 0));
      if (!es) return 0;
      const uint64_t sz = 5ull + (uint64_t)cnt * es;  // 64-bit: a malformed count must not wrap into a small size
      return sz > (uint64_t)(end - p) ? 0u : (uint32_t)sz;
    }
    default: return 0;
  }
}
ELP_TAG_HD bool tag_is_int(uint8_t t) { return t == 'c' || t == 'C' || t == 's' || t == 'S' || t == 'i' || t == 'I'; }
ELP_TAG_HD_NOFORCE long long tag_int_value(uint8_t t, const uint8_t *p) {
  switch (t) {
    case 'c': return (long long)(int8_t)p[0];
    case 'C': return (long long)p[0];
    case 's': return (long long)(int16_t)ld_u16(p);
    case 'S': return (long long)ld_u16(p);
    case 'i': return (long long)(int32_t)ld_u32(p);
    default: return (long long)ld_u32(p);
  }
}

}  // namespace elp
