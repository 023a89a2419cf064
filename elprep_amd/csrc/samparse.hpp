// samparse.hpp — the token parsers of SAM text IN (parseSamAlignment, sam/sam-files.go:186-410; ScanCigarString, sam/sam-types.go:680-740),
// as host-and-device code in the manner of samtext.hpp: the integers of strconv.ParseInt / ParseUint, one CIGAR token and the merge of a
// run of equal operations, the base -> nibble table, formatBamTag's integer rule and the float32 of strconv.ParseFloat(s, 32).  The
// kernels of samin.hip and the host build the CPU tests compile (tests/samparse_host.cpp) run the same functions.
//
// Every parser takes the token as (pointer, length) and returns a Reason: 0, or why the line is refused.  Reasons below R_UNSUPPORTED
// are what the reference panics on (ELP_ERR_DATA); the others are inputs the reference accepts and this library does not
// (ELP_ERR_UNSUPPORTED).
//
// strconv is restated from its documentation - no Go toolchain was at hand to run it against:
//   ParseInt(s, 10, b):  [+-]digits, no underscores (they need base 0), out of range for b bits = an error; ParseUint: no sign.
//   ParseFloat(s, 32):   [+-](digits[.digits] | .digits)[(e|E)[+-]digits], or [+-]inf / [+-]infinity / nan (no sign) in either case; the
//                        result is the float32 NEAREST the decimal, ties to even, rounded once (not via a float64); a decimal that
//                        rounds beyond the largest float32 is a range error, one below half the smallest denormal is +-0.
//                        Hexadecimal floats and digit-separating underscores, which ParseFloat reads, are refused (R_FLOAT_FORM), as is
//                        a token of more than FLOAT_MAX_TOKEN bytes.
// The float: with D the decimal's significant digits (at most 64, an integer below 2^213) and the value D * 10^e,
//   fast path  D < 2^24 and |e| <= 10: both exact as float32, ONE float32 multiplication or division rounds correctly (Clinger);
//   the rest   value = A / B with A = D * 10^max(e, 0), B = 10^max(-e, 0) as integers of WIDE_LIMBS * 32 bits (B <= 10^109 < 2^363: a
//              decimal whose first digit stands at 10^-47 or below is 0, at 10^39 or above a range error); both shifted to the same bit
//              length, the mantissa's bits come from a restoring division one at a time, then the guard bit and whether anything is left
//              (sticky): round half to even on exact integers.  Denormals take as many bits as they have.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define ELP_SAMIN_HD __host__ __device__ inline
#else
#define ELP_SAMIN_HD inline
#endif

namespace elp {
namespace samparse {

enum Reason : uint32_t {
  R_OK = 0,
  R_MISSING_TAB,      // fewer than eleven fields ("missing tabulator in SAM alignment line"); an empty line
  R_LINE_LONG,        // bufio.Scanner: token too long (maxTokenSize, sam/sam-files.go:614)
  R_FLAG, R_MAPQ, R_POS, R_PNEXT, R_TLEN,   // strconv errors of the mandatory numbers
  R_CIGAR,            // empty length, unknown operation, length beyond int32, digits without an operation
  R_FIELD,            // an optional field that is not KK:T:...
  R_FIELD_TYPE,       // unknown type byte
  R_FIELD_A,          // A: not exactly one byte
  R_FIELD_INT,        // i: strconv error at 64 bits
  R_FIELD_FLOAT,      // f / B:f: syntax or range
  R_FIELD_B,          // B: no subtype + comma ("missing entry in numeric array"), unknown subtype
  R_FIELD_B_ENTRY,    // B: strconv error of an entry
  R_UNSUPPORTED = 32,
  R_NAME_UNKNOWN = 32,  // RNAME / RNEXT neither * / = nor in the dictionary
  R_CIGAR_LENGTH,     // a merged length above 2^28 - 1
  R_CIGAR_OPS,        // more than 65535 operations
  R_QUAL_LENGTH,      // len(QUAL) != len(SEQ)
  R_QNAME_LONG,       // above 254 bytes
  R_QNAME_NUL,
  R_FIELD_TWICE,      // two fields of one key
  R_FIELD_INT_RANGE,  // i outside [-2^31, 2^32 - 1]
  R_FIELD_Z_NUL,
  R_FIELD_H,
  R_FLOAT_FORM,       // hex float, underscore, token above FLOAT_MAX_TOKEN bytes
  R_FIELDS_MANY,      // more optional fields in a line than MAX_FIELDS
  R_COUNT
};
constexpr uint32_t MAX_LINE = 1u << 20;       // maxTokenSize
constexpr uint32_t MAX_TABS = 256;            // tab positions a wave keeps per line
constexpr uint32_t MAX_FIELDS = MAX_TABS - 11;  // optional fields per line (a trailing tab included)
constexpr uint32_t FLOAT_MAX_TOKEN = 64;

// (host code: the text elp_last_error gives)
inline const char *reason_text(uint32_t r) {
  switch (r) {
    case R_MISSING_TAB: return "missing tabulator in SAM alignment line";
    case R_LINE_LONG: return "line longer than 1 MiB";
    case R_FLAG: return "FLAG is not a 16-bit unsigned number";
    case R_MAPQ: return "MAPQ is not an 8-bit unsigned number";
    case R_POS: return "POS is not a 32-bit number";
    case R_PNEXT: return "PNEXT is not a 32-bit number";
    case R_TLEN: return "TLEN is not a 32-bit number";
    case R_CIGAR: return "invalid CIGAR string";
    case R_FIELD: return "invalid field tag in SAM alignment line";
    case R_FIELD_TYPE: return "invalid field type in SAM alignment line";
    case R_FIELD_A: return "an A field that is not one byte";
    case R_FIELD_INT: return "an i field that is not a 64-bit number";
    case R_FIELD_FLOAT: return "a float that does not parse or is out of range";
    case R_FIELD_B: return "missing entry in numeric array, or invalid numeric array type";
    case R_FIELD_B_ENTRY: return "an entry of a numeric array does not parse as its type";
    case R_NAME_UNKNOWN: return "RNAME or RNEXT is not in the reference dictionary";
    case R_CIGAR_LENGTH: return "a CIGAR operation longer than 268435455";
    case R_CIGAR_OPS: return "more than 65535 CIGAR operations";
    case R_QUAL_LENGTH: return "QUAL and SEQ differ in length";
    case R_QNAME_LONG: return "QNAME longer than 254 bytes";
    case R_QNAME_NUL: return "NUL byte in QNAME";
    case R_FIELD_TWICE: return "two optional fields of one key";
    case R_FIELD_INT_RANGE: return "an i field outside [-2^31, 2^32-1]";
    case R_FIELD_Z_NUL: return "NUL byte in a Z field";
    case R_FIELD_H: return "H-typed optional field";
    case R_FLOAT_FORM: return "a float in hexadecimal form, with an underscore or longer than 64 bytes";
    case R_FIELDS_MANY: return "more than 245 optional fields in a line";
    default: return "unknown reason";
  }
}

ELP_SAMIN_HD bool is_digit(uint8_t c) { return c >= '0' && c <= '9'; }

// strconv.ParseInt(s, 10, bits) (is_signed) / strconv.ParseUint(s, 10, bits): false = an error (syntax or range)
ELP_SAMIN_HD bool parse_int(const uint8_t *s, uint32_t n, uint32_t bits, bool is_signed, int64_t *out) {
  uint32_t i = 0;
  bool neg = false;
  if (is_signed && n && (s[0] == '+' || s[0] == '-')) { neg = s[0] == '-'; i = 1; }
  if (i >= n) return false;
  const uint64_t limit = is_signed ? (1ull << (bits - 1)) - (neg ? 0ull : 1ull) : (bits == 64 ? ~0ull : (1ull << bits) - 1ull);
  const uint64_t l10 = limit / 10u, lr = limit % 10u;
  uint64_t v = 0;
  for (; i < n; i++) {
    if (!is_digit(s[i])) return false;
    const uint32_t d = s[i] - '0';
    if (v > l10 || (v == l10 && d > lr)) return false;
    v = v * 10u + d;
  }
  *out = neg ? (int64_t)(0ull - v) : (int64_t)v;
  return true;
}

// formatBamTag's integer rule (sam/bam-files.go:492-525): type and bytes of the stored value
ELP_SAMIN_HD uint32_t int_store(int64_t v, uint8_t *type) {
  if (v < 0) {
    if (v >= -128) { *type = 'c'; return 1; }
    if (v >= -32768) { *type = 's'; return 2; }
    *type = 'i';
    return 4;
  }
  if (v <= 255) { *type = 'C'; return 1; }
  if (v <= 65535) { *type = 'S'; return 2; }
  *type = 'I';
  return 4;
}

// baseToNibble (sam/sam-types.go): "=ACMGRSVTWYHKDBN", every other byte 15
constexpr uint64_t nibble_word(int half) {
  const char order[] = "=ACMGRSVTWYHKDBN";
  uint64_t w = ~0ull;
  for (int nb = 1; nb < 16; nb++) {
    const int i = order[nb] - 'A';
    if (i / 16 == half) w = (w & ~(0xFull << (4 * (i % 16)))) | ((uint64_t)nb << (4 * (i % 16)));
  }
  return w;
}
ELP_SAMIN_HD uint32_t base_nibble(uint8_t c) {
  constexpr uint64_t lo = nibble_word(0), hi = nibble_word(1);  // 'A' .. 'P', 'Q' .. (no table in memory, as samtext::base_of)
  if (c == '=') return 0;
  const uint32_t i = (uint32_t)c - 'A';
  if (i >= 32) return 15;
  return (uint32_t)(((i & 16u) ? hi : lo) >> (4u * (i & 15u))) & 15u;
}

// ---- CIGAR
// cigarOperationsTable: "MmIiDdNnSsHhPpXx=", lower case reads as upper case; 0xFF = not an operation
ELP_SAMIN_HD uint32_t cigar_op_code(uint8_t c) {
  switch (c | 0x20) {
    case 'm': return 0;
    case 'i': return 1;
    case 'd': return 2;
    case 'n': return 3;
    case 's': return 4;
    case 'h': return 5;
    case 'p': return 6;
    case 'x': return 8;
    default: return c == '=' ? 7u : 0xFFu;
  }
}
constexpr uint32_t CIGAR_MAX_LEN = (1u << 28) - 1u;
// newCigarOperation: the token whose digits are s[q .. p) and whose operation is s[p]
ELP_SAMIN_HD uint32_t cigar_token(const uint8_t *s, uint32_t q, uint32_t p, uint32_t *len, uint32_t *op) {
  int64_t v = 0;
  *op = cigar_op_code(s[p]);
  if (*op == 0xFFu || !parse_int(s + q, p - q, 32, true, &v)) return R_CIGAR;  // (digits only: the sign never comes into play)
  *len = (uint32_t)v;
  return R_OK;
}
// slowScanCigarString's merge: the length of the operation that BEGINS with the token (len, op) ending at p - the tokens behind it are
// added while they are of the same operation.  A malformed token behind it ends the walk (whoever looks at that token reports it).
ELP_SAMIN_HD uint32_t cigar_run(const uint8_t *s, uint32_t p, uint32_t end, uint32_t op, uint32_t len, uint32_t *merged) {
  uint64_t total = len;
  uint32_t q = p + 1;
  while (q < end && total <= CIGAR_MAX_LEN) {
    uint32_t e = q;
    while (e < end && is_digit(s[e])) e++;
    uint32_t l2, op2;
    if (e >= end || cigar_token(s, q, e, &l2, &op2) != R_OK || op2 != op) break;
    total += l2;
    q = e + 1;
  }
  if (total > CIGAR_MAX_LEN) return R_CIGAR_LENGTH;
  *merged = (uint32_t)total;
  return R_OK;
}
// the whole string, one token after the other (what the lanes of a wave do side by side in samin.hip): ops may be nullptr
ELP_SAMIN_HD uint32_t parse_cigar(const uint8_t *s, uint32_t n, uint32_t *ops, uint32_t *n_ops) {
  *n_ops = 0;
  if (n == 0 || (n == 1 && s[0] == '*')) return R_OK;
  uint32_t q = 0, prev = 0xFFu, cnt = 0;
  for (uint32_t p = 0; p < n; p++) {
    if (is_digit(s[p])) continue;
    uint32_t len, op, merged;
    if (const uint32_t r = cigar_token(s, q, p, &len, &op)) return r;
    if (op != prev) {
      if (const uint32_t r = cigar_run(s, p, n, op, len, &merged)) return r;
      if (ops && cnt < 65535u) ops[cnt] = (merged << 4) | op;
      cnt++;
    }
    prev = op;
    q = p + 1;
  }
  if (q != n) return R_CIGAR;  // digits without an operation (the reference indexes past the string)
  if (cnt > 65535u) return R_CIGAR_OPS;
  *n_ops = cnt;
  return R_OK;
}

// ---- float32
constexpr int WIDE_LIMBS = 12;  // 384 bits
struct Wide {
  uint32_t w[WIDE_LIMBS];
};
ELP_SAMIN_HD void wide_set(Wide &a, uint32_t v) {
  a.w[0] = v;
  for (int k = 1; k < WIDE_LIMBS; k++) a.w[k] = 0;
}
ELP_SAMIN_HD void wide_mul_add(Wide &a, uint32_t f, uint32_t add) {  // a = a * f + add
  uint64_t carry = add;
  for (int k = 0; k < WIDE_LIMBS; k++) {
    const uint64_t p = (uint64_t)a.w[k] * f + carry;
    a.w[k] = (uint32_t)p;
    carry = p >> 32;
  }
}
ELP_SAMIN_HD void wide_pow10(Wide &a, uint32_t p) {  // a *= 10^p
  for (; p >= 9; p -= 9) wide_mul_add(a, 1000000000u, 0);
  uint32_t f = 1;
  for (; p > 0; p--) f *= 10u;
  if (f > 1) wide_mul_add(a, f, 0);
}
ELP_SAMIN_HD int32_t wide_bits(const Wide &a) {  // position of the top bit + 1; 0 for 0
  for (int k = WIDE_LIMBS - 1; k >= 0; k--)
    if (a.w[k]) return 32 * k + 32 - (int32_t)__builtin_clz(a.w[k]);
  return 0;
}
ELP_SAMIN_HD void wide_shl(Wide &a, uint32_t bits) {  // bits < 384
  const uint32_t limbs = bits >> 5, sh = bits & 31u;
  for (int k = WIDE_LIMBS - 1; k >= 0; k--) {
    const int from = k - (int)limbs;
    uint32_t v = 0;
    if (from >= 0) {
      v = a.w[from] << sh;
      if (sh && from >= 1) v |= a.w[from - 1] >> (32u - sh);
    }
    a.w[k] = v;
  }
}
ELP_SAMIN_HD void wide_shl1(Wide &a) {
  uint32_t carry = 0;
  for (int k = 0; k < WIDE_LIMBS; k++) {
    const uint32_t v = a.w[k];
    a.w[k] = (v << 1) | carry;
    carry = v >> 31;
  }
}
ELP_SAMIN_HD bool wide_ge(const Wide &a, const Wide &b) {
  for (int k = WIDE_LIMBS - 1; k >= 0; k--)
    if (a.w[k] != b.w[k]) return a.w[k] > b.w[k];
  return true;
}
ELP_SAMIN_HD void wide_sub(Wide &a, const Wide &b) {  // a -= b, a >= b
  uint32_t borrow = 0;
  for (int k = 0; k < WIDE_LIMBS; k++) {
    const uint64_t d = (uint64_t)a.w[k] - b.w[k] - borrow;
    a.w[k] = (uint32_t)d;
    borrow = (uint32_t)(d >> 63);
  }
}
ELP_SAMIN_HD bool wide_zero(const Wide &a) {
  uint32_t any = 0;
  for (int k = 0; k < WIDE_LIMBS; k++) any |= a.w[k];
  return any == 0;
}
ELP_SAMIN_HD uint8_t lower(uint8_t c) { return (c >= 'A' && c <= 'Z') ? (uint8_t)(c | 0x20) : c; }
ELP_SAMIN_HD bool same_word(const uint8_t *s, uint32_t n, const char *word, uint32_t wn) {
  if (n != wn) return false;
  for (uint32_t k = 0; k < n; k++)
    if (lower(s[k]) != (uint8_t)word[k]) return false;
  return true;
}
// the float32 nearest D * 10^e10, D > 0 held in `A`; magnitude bits, or false = beyond the largest float32
ELP_SAMIN_HD bool wide_to_f32(Wide &A, int32_t e10, uint32_t *bits) {
  Wide B;
  wide_set(B, 1u);
  if (e10 > 0) wide_pow10(A, (uint32_t)e10);
  else wide_pow10(B, (uint32_t)-e10);
  int32_t t = wide_bits(A) - wide_bits(B);
  if (t >= 0) wide_shl(B, (uint32_t)t);
  else wide_shl(A, (uint32_t)-t);
  if (!wide_ge(A, B)) { wide_shl1(A); t--; }
  // value = (A / B) * 2^t with 1 <= A / B < 2
  if (t > 127) return false;
  if (t < -150) { *bits = 0; return true; }
  const int32_t nbits = t >= -126 ? 24 : t + 150;
  uint32_t M = 0;
  for (int32_t k = 0; k < nbits; k++) {
    M <<= 1;
    if (wide_ge(A, B)) { wide_sub(A, B); M |= 1u; }
    wide_shl1(A);
  }
  const bool guard = wide_ge(A, B);
  if (guard) wide_sub(A, B);
  if (guard && (!wide_zero(A) || (M & 1u))) M++;
  if (t < -126) { *bits = M; return true; }  // (a denormal that rounds up to 2^23 IS the smallest normal number's bit pattern)
  const uint32_t r = ((uint32_t)(t + 127) << 23) + (M - 0x800000u);
  if (r >= 0x7F800000u) return false;
  *bits = r;
  return true;
}
ELP_SAMIN_HD float pow10_f32(uint32_t k) {  // k <= 10: exact
  float p = 1.0f;
  for (uint32_t j = 0; j < k; j++) p *= 10.0f;  // (every partial product is exact: 10^10 = 2^10 * 5^10, 5^10 < 2^24)
  return p;
}
ELP_SAMIN_HD uint32_t f32_bits(float f) {
  uint32_t b;
  __builtin_memcpy(&b, &f, 4);
  return b;
}
// float32(strconv.ParseFloat(s, 32)) as its bits
ELP_SAMIN_HD uint32_t parse_f32(const uint8_t *s, uint32_t n, uint32_t *bits) {
  if (n == 0) return R_FIELD_FLOAT;
  if (n > FLOAT_MAX_TOKEN) return R_FLOAT_FORM;
  for (uint32_t k = 0; k < n; k++)
    if (s[k] == '_') return R_FLOAT_FORM;
  uint32_t i = 0;
  bool neg = false;
  if (s[0] == '+' || s[0] == '-') { neg = s[0] == '-'; i = 1; }
  const uint32_t sign = neg ? 0x80000000u : 0u;
  if (same_word(s + i, n - i, "inf", 3) || same_word(s + i, n - i, "infinity", 8)) { *bits = sign | 0x7F800000u; return R_OK; }
  if (i == 0 && same_word(s, n, "nan", 3)) { *bits = 0x7FC00000u; return R_OK; }
  if (n - i >= 2 && s[i] == '0' && lower(s[i + 1]) == 'x') return R_FLOAT_FORM;
  // readFloat: the significant digits as an integer, dp = where the point stands among them
  Wide A;
  wide_set(A, 0u);
  int32_t nd = 0, dp = 0;
  bool sawdot = false, sawdigits = false;
  uint32_t small = 0;  // the digits' value while it fits 32 bits
  for (; i < n; i++) {
    const uint8_t ch = s[i];
    if (ch == '.') {
      if (sawdot) return R_FIELD_FLOAT;
      sawdot = true;
      dp = nd;
      continue;
    }
    if (!is_digit(ch)) break;
    sawdigits = true;
    if (ch == '0' && nd == 0) { dp--; continue; }  // leading zeros
    nd++;
    if (nd <= 9) small = small * 10u + (uint32_t)(ch - '0');
    wide_mul_add(A, 10u, (uint32_t)(ch - '0'));
  }
  if (!sawdigits) return R_FIELD_FLOAT;
  if (!sawdot) dp = nd;
  if (i < n && lower(s[i]) == 'e') {
    i++;
    int32_t esign = 1, e = 0;
    if (i < n && (s[i] == '+' || s[i] == '-')) { esign = s[i] == '-' ? -1 : 1; i++; }
    if (i >= n || !is_digit(s[i])) return R_FIELD_FLOAT;
    for (; i < n && is_digit(s[i]); i++)
      if (e < 10000) e = e * 10 + (int32_t)(s[i] - '0');
    dp += e * esign;
  }
  if (i != n) return R_FIELD_FLOAT;
  if (nd == 0) { *bits = sign; return R_OK; }
  // the value lies in [10^(dp - 1), 10^dp)
  if (dp > 39) return R_FIELD_FLOAT;        // >= 10^39: beyond the largest float32 (3.4e38)
  if (dp < -45) { *bits = sign; return R_OK; }  // < 10^-46, below half the smallest denormal (7.0e-46)
  const int32_t e10 = dp - nd;
  uint32_t mag;
  if (nd <= 9 && small < (1u << 24) && e10 >= -10 && e10 <= 10) {
    const float d = (float)small;
    mag = f32_bits(e10 >= 0 ? d * pow10_f32((uint32_t)e10) : d / pow10_f32((uint32_t)-e10));
  } else if (!wide_to_f32(A, e10, &mag)) {
    return R_FIELD_FLOAT;
  }
  *bits = sign | mag;
  return R_OK;
}

// one entry of a B array of subtype st (parseSamNumericArray, sam/sam-files.go:237-317) as the bytes BAM stores: c and i through ParseInt
// at 8 / 32 bits, C S I through ParseUint at 8 / 16 / 32 - and s through ParseUint(.., 16) cast to int16, as the reference has it: "-1"
// is refused, "40000" stored as -25536 (the same two bytes)
ELP_SAMIN_HD uint32_t elem_size(uint8_t st) { return (st == 'c' || st == 'C') ? 1u : ((st == 's' || st == 'S') ? 2u : ((st == 'i' || st == 'I' || st == 'f') ? 4u : 0u)); }
ELP_SAMIN_HD uint32_t parse_entry(uint8_t st, const uint8_t *s, uint32_t n, uint32_t *value) {
  if (st == 'f') return parse_f32(s, n, value);
  int64_t v = 0;
  const bool is_signed = st == 'c' || st == 'i';
  const uint32_t bits = (st == 'c' || st == 'C') ? 8u : ((st == 's' || st == 'S') ? 16u : 32u);
  if (!parse_int(s, n, bits, is_signed, &v)) return R_FIELD_B_ENTRY;
  *value = (uint32_t)v;
  return R_OK;
}

}  // namespace samparse
}  // namespace elp
