// optical_name_host.cpp — elprep_amd/csrc/optical_name.hpp behind C functions, for tests/test_optical_name_host_cpu.py: the host build
// of the name parser and the distance test that the kernels of metrics.hip run.  Built by the host compiler alone.
#include "../elprep_amd/csrc/optical_name.hpp"

#include <cstring>
#include <vector>

using namespace elp;

static uint64_t load8(const uint8_t *p) {
  uint64_t w;
  memcpy(&w, p, 8);
  return w;
}

extern "C" {

// tile_parse over the name, fetched as metrics.hip's tile_info fetches it: up to 48 bytes with six words loaded in front of the parse
// (a word the name does not reach is 0), longer names with a load per eight parsed bytes.  The name is copied into a buffer padded as
// the QNAME column is.  out: tile, x, y, bad
void on_tile_info(const uint8_t *name, uint32_t len, long long *out) {
  std::vector<uint8_t> buf((size_t)len + 64, 0xAA);  // (the padding is not zero: no byte behind the name may be parsed)
  if (len) memcpy(buf.data(), name, len);
  const uint8_t *q = buf.data();
  bool bad = false;
  Tile t;
  if (len <= 48) {
    const uint64_t w0 = len > 0 ? load8(q) : 0ull, w1 = len > 8 ? load8(q + 8) : 0ull, w2 = len > 16 ? load8(q + 16) : 0ull,
                   w3 = len > 24 ? load8(q + 24) : 0ull, w4 = len > 32 ? load8(q + 32) : 0ull, w5 = len > 40 ? load8(q + 40) : 0ull;
    t = tile_parse(len, &bad, [&](uint32_t k) { return k == 0 ? w0 : k == 1 ? w1 : k == 2 ? w2 : k == 3 ? w3 : k == 4 ? w4 : w5; });
  } else {
    t = tile_parse(len, &bad, [&](uint32_t k) { return load8(q + 8 * k); });
  }
  out[0] = t.t; out[1] = t.x; out[2] = t.y; out[3] = bad;
}

long long on_abs_diff(long long a, long long b) { return go_abs_diff(a, b); }

// a, b: tile, x, y; rg_rev: rgid << 1 | reversed
int on_close(const long long *a, uint32_t rg_rev_a, const long long *b, uint32_t rg_rev_b, long long dist) {
  return optical_close(Member{a[0], a[1], a[2], rg_rev_a, 0}, Member{b[0], b[1], b[2], rg_rev_b, 0}, dist);
}

}  // extern "C"
