// samtext_host.cpp — elprep_amd/csrc/samtext.hpp behind C functions, for tests/test_samtext_cpu.py.  The header is host-and-device code:
// this file is built by the host compiler alone.  Every function returns the number of bytes and writes them if out is not NULL.
#include "../elprep_amd/csrc/samtext.hpp"

using namespace elp::samtext;

extern "C" {

uint32_t samtext_i64(uint8_t *out, int64_t v) { return put_i64(out, v); }
uint32_t samtext_i64_width(int64_t v) { return i64_width(v); }
uint32_t samtext_f32(uint8_t *out, uint32_t bits) { return put_f32(out, bits); }
uint8_t samtext_base(uint32_t nibble) { return base_of(nibble); }
uint8_t samtext_cigar_op(uint32_t op) { return cigar_op_char(op); }
uint32_t samtext_field(uint8_t *out, const uint8_t *key, uint8_t type, const uint8_t *value, uint32_t value_bytes) { return put_field(out, key, type, value, value_bytes); }

// n floats at once: text k at out + 16 k, its length in len[k]; the width-only pass must agree (returns the number of disagreements)
uint64_t samtext_f32_many(const uint32_t *bits, uint64_t n, uint8_t *out, uint8_t *len) {
  uint64_t bad = 0;
  for (uint64_t k = 0; k < n; k++) {
    const uint32_t l = put_f32(out + 16 * k, bits[k]);
    len[k] = (uint8_t)l;
    bad += l != put_f32(nullptr, bits[k]) || l > FLOAT_MAX_TEXT;
  }
  return bad;
}

}  // extern "C"
