// samtext.hpp — the scalar pieces of SAM text (FormatAlignment / formatSamTag, sam/sam-files.go:485-598), as host-and-device code: the
// decimal form of an int64, the nibble -> base table, the text of a float32 and the text size of one optional field.  The emit kernels
// (sam.hip) and the host build the CPU tests compile (tests/samtext_host.cpp) run the same functions.
//
// Every writer takes `out` = where the text goes, or nullptr to count only, and returns the number of bytes: the size pass and the emit
// pass cannot disagree.  Nothing here buffers: digits go straight to `out`, from the last to the first.
//
// The float form is Go's strconv.AppendFloat(float64(v), 'g', -1, 32): the SHORTEST decimal that reads back as the float32, and of the
// decimals of that length the one nearest the value; exponent form (d[.ddd]e+XX, sign always, two exponent digits at least) if the decimal
// exponent X is < -4 or >= 6 (with the shortest form %g's precision counts as 6, strconv/ftoa.go), else positional.
//   The digits are generated exactly, in the manner of Steele & White's free-format algorithm: the value is R / S, the half gaps to the
// neighbouring float32 values are Mp / S (up) and Mm / S (down), all four unsigned integers of 192 bits.  x = m * 2^e with m < 2^24 and
// -149 <= e <= 104, so with R = 2m * 2^e (4m at a power of two, where the lower gap is half the upper) S is 2 or 4 times a power of ten
// below 10^39 (e >= 0: S < 2^130) or a power of two up to 2^151 times a power of ten that is at most x < 2^24 (e < 0: S < 2^175); R stays
// below 10 S and the gaps below S, so nothing exceeds 2^179.  After scaling to S <= R < 10 S a digit is floor(R / S) - at most nine
// subtractions -, and the generation stops at the first length n for which the n-digit decimal just below the value (distance rem / S)
// or just above it ((S - rem) / S) lies in the rounding interval - bounds included iff the mantissa is even -: any n-digit decimal in the
// interval implies that one of these two is.  Both inside: the nearer (they are never equally near: then the value would have n + 1
// digits, which takes more factors of two than a float32 that far from its neighbours has).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define ELP_SAM_HD __host__ __device__ inline
#else
#define ELP_SAM_HD inline
#endif

namespace elp {
namespace samtext {

// Sequence.Base (sam/sam-types.go): BAM's nibble codes
ELP_SAM_HD uint8_t base_of(uint32_t nibble) {
  // "=ACMGRSVTWYHKDBN" packed as two 64-bit words (no table in memory: a constant array would be a load per base on the device)
  const uint64_t lo = 0x565352474D43413Dull, hi = 0x4E42444B48595754ull;  // "=ACMGRSV", "TWYHKDBN", first character in the low byte
  return (uint8_t)(((nibble & 8u) ? hi : lo) >> (8u * (nibble & 7u)));
}
// "MIDNSHP=X" (cigarOps, sam/bam-files.go:289); codes above 8 index past the reference's table (it panics): '?' here
ELP_SAM_HD uint8_t cigar_op_char(uint32_t op) {
  const uint64_t lo = 0x3D5048534E44494Dull;  // "MIDNSHP="
  return op < 8 ? (uint8_t)(lo >> (8u * op)) : (op == 8 ? (uint8_t)'X' : (uint8_t)'?');
}

ELP_SAM_HD uint32_t u64_width(uint64_t v) {
  uint32_t w = 1;
  while (v >= 10) { v /= 10; w++; }
  return w;
}
// strconv.AppendUint(v, 10)
ELP_SAM_HD uint32_t put_u64(uint8_t *out, uint64_t v) {
  const uint32_t w = u64_width(v);
  if (out)
    for (uint32_t k = w; k-- > 0; v /= 10) out[k] = (uint8_t)('0' + (uint32_t)(v % 10));
  return w;
}
// the narrow case the emitters meet most (FLAG, MAPQ, POS, CIGAR lengths, B elements): 32-bit division only
ELP_SAM_HD uint32_t u32_width(uint32_t v) {
  return v < 10u ? 1u : v < 100u ? 2u : v < 1000u ? 3u : v < 10000u ? 4u : v < 100000u ? 5u : v < 1000000u ? 6u : v < 10000000u ? 7u : v < 100000000u ? 8u : v < 1000000000u ? 9u : 10u;
}
ELP_SAM_HD uint32_t put_u32(uint8_t *out, uint32_t v) {
  const uint32_t w = u32_width(v);
  if (out)
    for (uint32_t k = w; k-- > 0; v /= 10) out[k] = (uint8_t)('0' + v % 10);
  return w;
}
// strconv.AppendInt(v, 10); every integer of a SAM line is an int64 whose magnitude fits 32 bits, INT64_MIN included for completeness
ELP_SAM_HD uint32_t i64_width(int64_t v) {
  const uint64_t mag = v < 0 ? 0ull - (uint64_t)v : (uint64_t)v;
  return (v < 0 ? 1u : 0u) + (mag <= 0xFFFFFFFFull ? u32_width((uint32_t)mag) : u64_width(mag));
}
ELP_SAM_HD uint32_t put_i64(uint8_t *out, int64_t v) {
  const uint64_t mag = v < 0 ? 0ull - (uint64_t)v : (uint64_t)v;
  const uint32_t s = v < 0 ? 1u : 0u;
  if (out && s) out[0] = '-';
  uint8_t *o = out ? out + s : nullptr;
  return s + (mag <= 0xFFFFFFFFull ? put_u32(o, (uint32_t)mag) : put_u64(o, mag));
}

// ---- float32: shortest digits
constexpr int BIG_LIMBS = 6;  // 192 bits, 32 a limb
struct Big {
  uint32_t w[BIG_LIMBS];
};
ELP_SAM_HD void big_set(Big &a, uint32_t v) {
  a.w[0] = v;
  for (int k = 1; k < BIG_LIMBS; k++) a.w[k] = 0;
}
ELP_SAM_HD void big_mul(Big &a, uint32_t f) {
  uint64_t carry = 0;
  for (int k = 0; k < BIG_LIMBS; k++) {
    const uint64_t p = (uint64_t)a.w[k] * f + carry;
    a.w[k] = (uint32_t)p;
    carry = p >> 32;
  }
}
ELP_SAM_HD void big_shl(Big &a, uint32_t bits) {  // bits < 192
  const uint32_t limbs = bits >> 5, sh = bits & 31u;
  for (int k = BIG_LIMBS - 1; k >= 0; k--) {
    const int from = k - (int)limbs;
    uint32_t v = 0;
    if (from >= 0) {
      v = a.w[from] << sh;
      if (sh && from >= 1) v |= a.w[from - 1] >> (32u - sh);
    }
    a.w[k] = v;
  }
}
ELP_SAM_HD void big_pow10(Big &a, uint32_t p) {  // a *= 10^p
  for (; p >= 9; p -= 9) big_mul(a, 1000000000u);
  uint32_t f = 1;
  for (; p > 0; p--) f *= 10u;
  if (f > 1) big_mul(a, f);
}
ELP_SAM_HD int big_cmp(const Big &a, const Big &b) {
  for (int k = BIG_LIMBS - 1; k >= 0; k--)
    if (a.w[k] != b.w[k]) return a.w[k] < b.w[k] ? -1 : 1;
  return 0;
}
ELP_SAM_HD void big_sub(Big &a, const Big &b) {  // a -= b, a >= b
  uint32_t borrow = 0;
  for (int k = 0; k < BIG_LIMBS; k++) {
    const uint64_t d = (uint64_t)a.w[k] - b.w[k] - borrow;
    a.w[k] = (uint32_t)d;
    borrow = (uint32_t)(d >> 63);
  }
}
ELP_SAM_HD void big_add(Big &a, const Big &b) {
  uint64_t carry = 0;
  for (int k = 0; k < BIG_LIMBS; k++) {
    const uint64_t s = (uint64_t)a.w[k] + b.w[k] + carry;
    a.w[k] = (uint32_t)s;
    carry = s >> 32;
  }
}

// the shortest decimal of a finite, non-zero float32 (its bits without the sign): *digits (n decimal digits, no trailing zero unless n == 1)
// and the decimal exponent X of its first digit; returns n
ELP_SAM_HD uint32_t shortest_digits(uint32_t bits, uint32_t *digits, int32_t *exp10) {
  const uint32_t frac = bits & 0x7FFFFFu, ef = (bits >> 23) & 0xFFu;
  const uint32_t m = ef ? (frac | 0x800000u) : frac;
  const int32_t e = (ef ? (int32_t)ef : 1) - 150;
  const bool even = (m & 1u) == 0;
  const bool narrow = frac == 0 && ef > 1;  // a power of two above the smallest normal exponent: the float below is half a gap away
  Big R, S, Mp, Mm;
  big_set(R, narrow ? 4u * m : 2u * m);
  big_set(S, narrow ? 4u : 2u);
  big_set(Mp, narrow ? 2u : 1u);
  big_set(Mm, 1u);
  if (e >= 0) { big_shl(R, (uint32_t)e); big_shl(Mp, (uint32_t)e); big_shl(Mm, (uint32_t)e); }
  else big_shl(S, (uint32_t)-e);
  // X = floor(log10 x): estimated from the position of the top bit (floor(t * log10 2) as t * 78913 >> 18), then made exact
  const int32_t t = e + 31 - (int32_t)__builtin_clz(m);
  int32_t X = (int32_t)(((int64_t)t * 78913) >> 18);
  if (X >= 0) big_pow10(S, (uint32_t)X);
  else { big_pow10(R, (uint32_t)-X); big_pow10(Mp, (uint32_t)-X); big_pow10(Mm, (uint32_t)-X); }
  while (big_cmp(R, S) < 0) { big_mul(R, 10u); big_mul(Mp, 10u); big_mul(Mm, 10u); X--; }
  for (;;) {
    Big S10 = S;
    big_mul(S10, 10u);
    if (big_cmp(R, S10) < 0) break;
    S = S10;
    X++;
  }
  uint32_t D = 0, n = 0;
  for (;;) {
    uint32_t d = 0;
    while (big_cmp(R, S) >= 0) { big_sub(R, S); d++; }
    D = D * 10u + d;
    n++;
    // R = value - D (in units of this digit, times S): D is in the interval if R <= Mm, D + 1 if S - R <= Mp
    const int cl = big_cmp(R, Mm);
    const bool low = even ? cl <= 0 : cl < 0;
    Big up = R;
    big_add(up, Mp);
    const int ch = big_cmp(up, S);
    const bool high = even ? ch >= 0 : ch > 0;
    if (low || high) {
      bool take_up = high;
      if (low && high) {
        Big twice = R;
        big_add(twice, R);
        const int c2 = big_cmp(twice, S);
        take_up = c2 > 0 || (c2 == 0 && (D & 1u));
      }
      if (take_up) D++;
      break;
    }
    big_mul(R, 10u); big_mul(Mp, 10u); big_mul(Mm, 10u);
  }
  // D + 1 may end in zeros: 9 -> 10 at the first digit (the next decade), never later (a shorter decimal would have been taken)
  while (n > 1 && D % 10u == 0) { D /= 10u; n--; }
  if (n == 1 && D == 10u) { D = 1; X++; }
  *digits = D;
  *exp10 = X;
  return n;
}

// strconv.AppendFloat(float64(v), 'g', -1, 32) of the float32 with these bits; at most FLOAT_MAX_TEXT bytes
constexpr uint32_t FLOAT_MAX_TEXT = 15;  // "-0.00012345678", "-1.2345678e-38"
ELP_SAM_HD uint32_t put_lit(uint8_t *out, const char *s, uint32_t n) {
  if (out)
    for (uint32_t k = 0; k < n; k++) out[k] = (uint8_t)s[k];
  return n;
}
ELP_SAM_HD uint32_t put_f32(uint8_t *out, uint32_t bits) {
  const uint32_t mag = bits & 0x7FFFFFFFu;
  const bool neg = (bits >> 31) != 0;
  if (mag > 0x7F800000u) return put_lit(out, "NaN", 3);
  if (mag == 0x7F800000u) return put_lit(out, neg ? "-Inf" : "+Inf", 4);
  uint32_t at = 0;
  if (neg) { if (out) out[0] = '-'; at = 1; }
  if (mag == 0) { if (out) out[at] = '0'; return at + 1; }
  uint32_t D;
  int32_t X;
  const uint32_t n = shortest_digits(mag, &D, &X);
  uint8_t *o = out ? out + at : nullptr;
  uint32_t len;
  if (X < -4 || X >= 6) {  // %e: d[.ddd]e+XX
    const uint32_t ax = (uint32_t)(X < 0 ? -X : X);
    len = n + (n > 1 ? 1u : 0u) + 2u + (ax < 10 ? 2u : u32_width(ax));
    if (o) {
      uint32_t v = D;
      for (uint32_t k = n; k-- > 1; v /= 10u) o[1 + k] = (uint8_t)('0' + v % 10u);
      o[0] = (uint8_t)('0' + v);
      if (n > 1) o[1] = '.';
      uint8_t *x = o + n + (n > 1 ? 1u : 0u);
      x[0] = 'e';
      x[1] = X < 0 ? '-' : '+';
      x[2] = (uint8_t)('0' + ax / 10u);
      x[3] = (uint8_t)('0' + ax % 10u);  // (|X| <= 45)
    }
  } else if (X >= 0) {  // %f: X + 1 integer digits (zeros behind the n digits if they are fewer), then the rest behind a point
    const uint32_t ip = (uint32_t)X + 1u;
    len = n <= ip ? ip : n + 1u;
    if (o) {
      uint32_t v = D;
      for (uint32_t k = len; k-- > 0;) {
        if (n > ip && k == ip) { o[k] = '.'; continue; }
        const uint32_t digit_at = k > ip ? k - 1 : k;  // index among the digits
        if (digit_at >= n) o[k] = '0';
        else { o[k] = (uint8_t)('0' + v % 10u); v /= 10u; }
      }
    }
  } else {  // 0.000ddd: -X - 1 zeros behind the point
    const uint32_t z = (uint32_t)(-X) - 1u;
    len = 2u + z + n;
    if (o) {
      o[0] = '0'; o[1] = '.';
      for (uint32_t k = 0; k < z; k++) o[2 + k] = '0';
      uint32_t v = D;
      for (uint32_t k = n; k-- > 0; v /= 10u) o[2 + z + k] = (uint8_t)('0' + v % 10u);
    }
  }
  return at + len;
}

// ---- optional fields
ELP_SAM_HD uint32_t rd_u16(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
ELP_SAM_HD uint32_t rd_u32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
ELP_SAM_HD uint32_t elem_size(uint8_t st) { return (st == 'c' || st == 'C') ? 1u : ((st == 's' || st == 'S') ? 2u : ((st == 'i' || st == 'I' || st == 'f') ? 4u : 0u)); }
// one element of a B array (or the value of a c C s S i I f field) of type st at p: its text, without a separator
ELP_SAM_HD uint32_t put_number(uint8_t *out, uint8_t st, const uint8_t *p) {
  switch (st) {
    case 'c': return put_i64(out, (int64_t)(int8_t)p[0]);
    case 'C': return put_u32(out, p[0]);
    case 's': return put_i64(out, (int64_t)(int16_t)rd_u16(p));
    case 'S': return put_u32(out, rd_u16(p));
    case 'i': return put_i64(out, (int64_t)(int32_t)rd_u32(p));
    case 'I': return put_u32(out, rd_u32(p));
    default: return put_f32(out, rd_u32(p));
  }
}
// formatSamTag: the text of one well-formed field - '\t', key, ':', type, ':', value - whose BAM value at v has `sz` bytes (bamtag.hpp's
// tag_value_size); type H (which the emitters refuse) counts as its bytes
ELP_SAM_HD uint32_t put_field(uint8_t *out, const uint8_t *key, uint8_t ty, const uint8_t *v, uint32_t sz) {
  const bool is_int = ty == 'c' || ty == 'C' || ty == 's' || ty == 'S' || ty == 'i' || ty == 'I';
  if (out) { out[0] = '\t'; out[1] = key[0]; out[2] = key[1]; out[3] = ':'; out[4] = is_int ? (uint8_t)'i' : ty; out[5] = ':'; }
  uint8_t *o = out ? out + 6 : nullptr;
  if (is_int || ty == 'f') return 6 + put_number(o, ty, v);
  if (ty == 'A') { if (o) o[0] = v[0]; return 7; }
  if (ty == 'B') {
    const uint8_t st = v[0];
    const uint32_t cnt = rd_u32(v + 1), es = elem_size(st);
    if (o) o[0] = st;
    uint32_t at = 1;
    for (uint32_t k = 0; k < cnt; k++) {
      if (o) o[at] = ',';
      at += 1 + put_number(o ? o + at + 1 : nullptr, st, v + 5 + (uint64_t)k * es);
    }
    return 6 + at;
  }
  // Z (H): the bytes in front of the NUL
  if (o)
    for (uint32_t k = 0; k + 1 < sz; k++) o[k] = v[k];
  return 6 + sz - 1;
}

}  // namespace samtext
}  // namespace elp
