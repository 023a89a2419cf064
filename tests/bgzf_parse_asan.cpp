// bgzf_parse_asan.cpp — bgzf_parse (elprep_amd/csrc/bgzf_plan.hpp), the one place where the library reads bytes it has no reason to
// trust, on its own under the sanitizers: build with  g++ -fsanitize=address,undefined -fno-sanitize-recover=all  and run.
// A valid file of three members and the end-of-file block is parsed from a heap buffer of EXACTLY n bytes for every truncation n in
// [0, size], then with every single byte of the first member's 18 header bytes set to 0x00, to 0xFF and to its complement (once more with
// that header's XLEN at 0xFFFF) - a read one byte behind the buffer trips the sanitizer.  Every call must succeed or return one of the error kinds, and what it lists must lie
// inside the buffer.  Exit status 0 and no report: passed (tests/test_bgzf_plan_cpu.py runs it).
#include "../elprep_amd/csrc/bgzf_plan.hpp"

#include <cstdio>
#include <memory>

using namespace elp;

// a member around a stored DEFLATE block of `len` bytes (the parser reads neither the data nor the CRC's value)
static void member(std::vector<uint8_t> &f, uint32_t len) {
  const uint32_t total = 18 + 5 + len + 8;
  const uint8_t head[18] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, (uint8_t)((total - 1) & 0xFF), (uint8_t)((total - 1) >> 8)};
  f.insert(f.end(), head, head + 18);
  const uint8_t stored[5] = {0x01, (uint8_t)(len & 0xFF), (uint8_t)(len >> 8), (uint8_t)(~len & 0xFF), (uint8_t)((~len >> 8) & 0xFF)};
  f.insert(f.end(), stored, stored + 5);
  for (uint32_t k = 0; k < len; k++) f.push_back((uint8_t)(k * 7 + len));
  const uint32_t crc = 0x12345678u + len;
  for (int k = 0; k < 4; k++) f.push_back((uint8_t)(crc >> (8 * k)));
  for (int k = 0; k < 4; k++) f.push_back((uint8_t)(len >> (8 * k)));
}

static int failures = 0;
static void expect(bool ok, const char *what, size_t n, int at, int value) {
  if (ok) return;
  failures++;
  fprintf(stderr, "bgzf_parse_asan: %s (buffer of %zu bytes, byte %d set to 0x%02x)\n", what, n, at, value);
}

// parses the first n bytes of `f` from a buffer of exactly n bytes, byte `at` replaced by `value` if at >= 0
static BgzfParse parse_exact(const std::vector<uint8_t> &f, size_t n, int at = -1, int value = 0) {
  std::unique_ptr<uint8_t[]> buf(new uint8_t[n]);
  if (n) memcpy(buf.get(), f.data(), n);
  if (at >= 0) buf[at] = (uint8_t)value;
  BgzfParse r = bgzf_parse(buf.get(), n);
  expect(r.error >= BGZF_PARSE_OK && r.error <= BGZF_ISIZE_TOO_BIG, "an error value that is none of the kinds", n, at, value);
  expect(r.error == BGZF_PARSE_OK || r.at < n || (r.error == BGZF_TRUNCATED_HEADER && r.at <= n), "an error behind the buffer", n, at, value);
  if (r.error == BGZF_PARSE_OK) {
    uint64_t inflated = 0;
    for (const BgzfBlk &b : r.blocks) {
      expect(b.in_off + b.in_len + 8 <= n, "a block that reaches behind the buffer", n, at, value);
      expect(b.out_len >= 1 && b.out_len <= 65536 && b.out_off == inflated, "a block out of place in the inflated stream", n, at, value);
      inflated += b.out_len;
    }
    expect(inflated == r.inflated, "a wrong inflated total", n, at, value);
  }
  return r;
}

int main() {
  std::vector<uint8_t> f;
  const uint32_t lens[3] = {10, 20, 5};
  size_t ends[4];
  for (int k = 0; k < 3; k++) { member(f, lens[k]); ends[k] = f.size(); }
  const uint8_t eof[28] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, 0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  f.insert(f.end(), eof, eof + 28);
  ends[3] = f.size();
  // every truncation: whole members parse, anything else is an error at the member that is cut
  for (size_t n = 0; n <= f.size(); n++) {
    const BgzfParse r = parse_exact(f, n);
    size_t whole = 0, start = 0;
    while (whole < 4 && ends[whole] <= n) start = ends[whole++];
    if (n == start) {
      expect(r.error == BGZF_PARSE_OK && r.blocks.size() == std::min<size_t>(whole, 3), "whole members that do not parse", n, -1, 0);
    } else {
      expect(r.error != BGZF_PARSE_OK && r.at == start, "a cut member that parses, or an error at another member", n, -1, 0);
      expect((n - start < 18) == (r.error == BGZF_TRUNCATED_HEADER), "a cut header that is not reported as one", n, -1, 0);
    }
  }
  const BgzfParse whole = parse_exact(f, f.size());
  expect(whole.blocks.size() == 3 && whole.inflated == 35, "the whole file", f.size(), -1, 0);
  // every byte of the first header, three values each, in the whole file and in a file that ends with the first member
  // (and the same again with an XLEN of 0xFFFF in that header: the walk over the subfields must stop at the buffer's end by itself)
  std::vector<uint8_t> wide = f;
  wide[10] = wide[11] = 0xFF;
  for (const std::vector<uint8_t> *file : {&f, &wide})
    for (int at = 0; at < 18; at++) {
      const int values[3] = {0x00, 0xFF, (uint8_t)~(*file)[at]};
      for (int value : values) {
        parse_exact(*file, file->size(), at, value);
        parse_exact(*file, ends[0], at, value);
      }
    }
  if (failures) return 1;
  printf("bgzf_parse_asan: ok\n");
  return 0;
}
