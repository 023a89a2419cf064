// bamtag.hpp — reading a BAM record's bytes on the device: little-endian loads / stores and the optional fields' sizes and integer
// values (parseBamAlignment, sam/bam-files.go:138-221, 373-396; formatBamTag's integer rule :492-525).  Shared by bam_in.hip (staging),
// bam_out.hip and sam.hip (the emitters) and filter.hip (the predicate that reads optional fields, whose rule - filter_rules.hpp - takes
// the pure readers from bamtag_read.hpp).
#pragma once

#include "common.hpp"
#include "bamtag_read.hpp"  // ld_u16, ld_u32, tag_value_size, tag_is_int, tag_int_value: host-and-device
#include "samparse.hpp"

namespace elp {

__device__ __forceinline__ void st_u16(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); }
__device__ __forceinline__ void st_u32(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }

// formatBamTag's integer rule (:492-525): type and size of the re-encoded value (samparse.hpp's, which SAM text in stores by)
__device__ __forceinline__ uint32_t int_out(long long v, uint8_t *type) { return samparse::int_store((int64_t)v, type); }

// a two-byte key as the 16-bit number the tag filter's bit table is indexed by
__device__ __forceinline__ uint32_t tag_key(const uint8_t *t) { return (uint32_t)t[0] | ((uint32_t)t[1] << 8); }
constexpr uint32_t tag_key_of(char a, char b) { return (uint32_t)(uint8_t)a | ((uint32_t)(uint8_t)b << 8); }

}  // namespace elp
