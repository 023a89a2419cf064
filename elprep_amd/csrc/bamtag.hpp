// bamtag.hpp — reading a BAM record's bytes on the device: little-endian loads / stores and the optional fields' sizes and integer
// values (parseBamAlignment, sam/bam-files.go:138-221, 373-396; formatBamTag's integer rule :492-525).  Shared by bam_in.hip (staging),
// bam_out.hip and sam.hip (the emitters) and filter.hip (the predicate that reads optional fields).
#pragma once

#include "common.hpp"
#include "samparse.hpp"

namespace elp {

__device__ __forceinline__ uint32_t ld_u16(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
__device__ __forceinline__ uint32_t ld_u32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
__device__ __forceinline__ void st_u16(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); }
__device__ __forceinline__ void st_u32(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }

// bytes of the value of one optional field of type `t` at p (end = end of the record); 0 = malformed
__device__ inline uint32_t tag_value_size(uint8_t t, const uint8_t *p, const uint8_t *end) {
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
__device__ __forceinline__ bool tag_is_int(uint8_t t) { return t == 'c' || t == 'C' || t == 's' || t == 'S' || t == 'i' || t == 'I'; }
__device__ inline long long tag_int_value(uint8_t t, const uint8_t *p) {
  switch (t) {
    case 'c': return (long long)(int8_t)p[0];
    case 'C': return (long long)p[0];
    case 's': return (long long)(int16_t)ld_u16(p);
    case 'S': return (long long)ld_u16(p);
    case 'i': return (long long)(int32_t)ld_u32(p);
    default: return (long long)ld_u32(p);
  }
}
// formatBamTag's integer rule (:492-525): type and size of the re-encoded value (samparse.hpp's, which SAM text in stores by)
__device__ __forceinline__ uint32_t int_out(long long v, uint8_t *type) { return samparse::int_store((int64_t)v, type); }

// a two-byte key as the 16-bit number the tag filter's bit table is indexed by
__device__ __forceinline__ uint32_t tag_key(const uint8_t *t) { return (uint32_t)t[0] | ((uint32_t)t[1] << 8); }
constexpr uint32_t tag_key_of(char a, char b) { return (uint32_t)(uint8_t)a | ((uint32_t)(uint8_t)b << 8); }

}  // namespace elp
