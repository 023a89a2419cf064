// optical_name.hpp — what the optical-duplicate count reads out of a QNAME and how it compares two of them (computeTileInfo,
// filters/mark-optical-duplicates.go:50-71; isOpticalDuplicate :82-93; isOpticalDuplicateShort, filters/unpedantic.go:32-34; absInt,
// filters/utils.go:62), as host-and-device code in the manner of samparse.hpp: the kernels of metrics.hip and the host build the CPU
// tests compile (tests/optical_name_host.cpp) run the same functions.  How a name's bytes are fetched stays with the caller (`word`).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define ELP_OPTNAME_HD __host__ __device__ __forceinline__
#else
#define ELP_OPTNAME_HD inline
#endif

namespace elp {

struct Tile { long long t, x, y; };

// computeTileInfo :50-71; *bad is set where internal.ParseInt would panic (strconv.ParseInt(s, 10, 64): one optional sign, one or
// more ASCII digits - leading zeros of any length -, the value in [-2^63, 2^63 - 1]).  One pass over the name, eight bytes per load: the
// integer value (and parse status) of fields 2..6 is kept in scalars, the field count decides at the end which three are used
// (7 fields -> 4,5,6; 5 fields -> 2,3,4).
// `word(k)` = bytes 8 k .. 8 k + 7 of the name
template <class W>
ELP_OPTNAME_HD Tile tile_parse(uint32_t len, bool *bad, W word) {
  long long v2 = 0, v3 = 0, v4 = 0, v5 = 0, v6 = 0;
  uint32_t badmask = 0;       // bit k: field k does not parse
  int col = 0;
  unsigned long long x = 0;   // magnitude of the current field
  uint32_t ndig = 0;          // digits seen in the current field
  bool neg = false, fbad = false, first = true;
  uint64_t w = 0;
  for (uint32_t i = 0;; i++) {
    const bool end = i == len;
    if (!end && (i & 7u) == 0) w = word(i >> 3);
    const uint32_t ch = end ? (uint32_t)':' : (uint32_t)(w >> (8 * (i & 7u))) & 0xFFu;
    if (ch == ':') {
      const bool fb = fbad || ndig == 0 || x > (neg ? 0x8000000000000000ull : 0x7FFFFFFFFFFFFFFFull);
      const long long val = (long long)(neg ? 0ull - x : x);
      if (col == 2) v2 = val; else if (col == 3) v3 = val; else if (col == 4) v4 = val; else if (col == 5) v5 = val; else if (col == 6) v6 = val;
      if (col >= 2 && col <= 6 && fb) badmask |= 1u << col;
      col++;
      x = 0; ndig = 0; neg = false; fbad = false; first = true;
    } else {
      if (first && (ch == '+' || ch == '-')) {
        neg = ch == '-';
      } else {
        const uint32_t d = ch - (uint32_t)'0';
        if (d > 9) fbad = true;
        else if (x > 922337203685477580ull) fbad = true;  // over 2^63 already (x * 10 >= 9223372036854775810); stays bad
        else x = x * 10 + d;
        ndig++;
      }
      first = false;
    }
    if (end) break;
  }
  int a;
  if (col == 7) a = 4;
  else if (col == 5) a = 2;
  else return Tile{-1, -1, -1};
  if (badmask & (7u << a)) { *bad = true; return Tile{-1, -1, -1}; }
  return a == 4 ? Tile{v4, v5, v6} : Tile{v2, v3, v4};
}

// a listed read of a duplicate set.  rg_rev = rgid << 1 | reversed; bad: the name does not parse (the reference panics if it parses it:
// a member of a strand list of 2..OPT_LIST_CAP entries, :327-368; k_opt_eval decides)
struct Member { long long t, x, y; uint32_t rg_rev, bad; };

// absInt (filters/utils.go:62) of a - b on Go's int: the difference wraps, and absInt(MinInt64) stays MinInt64 (so it is "close")
ELP_OPTNAME_HD long long go_abs_diff(long long a, long long b) {
  const unsigned long long d = (unsigned long long)a - (unsigned long long)b;
  return (long long)((long long)d < 0 ? 0ull - d : d);
}
ELP_OPTNAME_HD bool optical_close(const Member &a, const Member &b, long long dist) {  // isOpticalDuplicate + same RG / strand list / tile
  if (a.t == -1 || b.rg_rev != a.rg_rev || b.t != a.t) return false;
  return go_abs_diff(a.x, b.x) <= dist && go_abs_diff(a.y, b.y) <= dist;
}

}  // namespace elp
