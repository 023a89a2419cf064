// bai_plan_asan.cpp — bai_members (elprep_amd/csrc/bai_plan.hpp), the index calls' walk over BGZF members it has no reason to trust, on
// its own under the sanitizers: build with  g++ -fsanitize=address,undefined -fno-sanitize-recover=all  and run.
// A stream of three members (payloads of 65280, 65280 and 100 bytes in stored blocks: 65311 + 65311 + 131 bytes) is walked from a heap
// buffer of EXACTLY n bytes for every truncation n, then whole with every single byte of the three 18-byte headers and of the three
// ISIZE fields set to 0x00, to 0xFF and to its complement - a read one byte behind the buffer trips the sanitizer.  Every call must
// give the table or one of the refusals with a byte inside the buffer and a text; what a sound answer lists must lie inside the buffer.
// Exit status 0 and no report: passed (tests/test_bai_plan_cpu.py runs it).
#include "../elprep_amd/csrc/bai_plan.hpp"

#include <cstdio>
#include <memory>

using namespace elp;

static int failures = 0;
static void expect(bool ok, const char *what, uint64_t a = 0, uint64_t b = 0, uint64_t c = 0) {
  if (ok) return;
  failures++;
  fprintf(stderr, "bai_plan_asan: %s (%llu, %llu, %llu)\n", what, (unsigned long long)a, (unsigned long long)b, (unsigned long long)c);
}

static void member(std::vector<uint8_t> &f, uint32_t payload) {
  const uint32_t total = 18 + 5 + payload + 8;
  const uint8_t head[18] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, (uint8_t)((total - 1) & 0xFF), (uint8_t)((total - 1) >> 8)};
  f.insert(f.end(), head, head + 18);
  const uint8_t stored[5] = {1, (uint8_t)(payload & 0xFF), (uint8_t)(payload >> 8), (uint8_t)(~payload & 0xFF), (uint8_t)((~payload >> 8) & 0xFF)};
  f.insert(f.end(), stored, stored + 5);
  for (uint32_t k = 0; k < payload; k++) f.push_back((uint8_t)(k * 7 + payload));
  for (int k = 0; k < 4; k++) f.push_back((uint8_t)(0xC0 + k));  // (the walk does not read the CRC-32)
  for (int k = 0; k < 4; k++) f.push_back((uint8_t)(payload >> (8 * k)));
}

// the walk over the first n bytes of `f` from a buffer of exactly n bytes, byte `at` replaced by `value` if at >= 0
static BaiMembers walk(const std::vector<uint8_t> &f, size_t n, long at, int value) {
  std::unique_ptr<uint8_t[]> buf(new uint8_t[n]);
  if (n) memcpy(buf.get(), f.data(), n);
  if (at >= 0) buf[at] = (uint8_t)value;
  BaiMembers r = bai_members(buf.get(), n);
  expect(r.error >= BAI_MEMBERS_OK && r.error <= BAI_BAD_LAST_ISIZE, "an error value that is none of the kinds", n, (uint64_t)at, r.error);
  if (r.error) {
    expect(r.at < n, "a refusal that names a byte behind the buffer", n, (uint64_t)at, r.at);
    expect(r.coff.empty() && r.inflated == 0, "a refusal that leaves a table", n, (uint64_t)at, r.coff.size());
    expect(r.text("who").size() > 10, "a refusal without a text", n, (uint64_t)at, r.error);
    expect(!bai_is_the_stream(r, 0), "refused bytes that pass for a stream", n, (uint64_t)at);
  } else {
    expect(!r.coff.empty() && r.coff.front() == 0 && r.coff.back() == n, "a table that does not span the bytes", n, (uint64_t)at, r.coff.back());
    uint64_t bound = 0;
    for (size_t k = 0; k + 1 < r.coff.size(); k++) {
      expect(r.coff[k + 1] >= r.coff[k] + BAI_MEMBER_MIN, "a member below the smallest", n, (uint64_t)at, k);
      bound += BGZF_PAYLOAD;
    }
    expect(r.inflated <= bound && (r.n_members() == 0 || r.inflated > bound - BGZF_PAYLOAD), "ISIZE that do not fit the members", n, (uint64_t)at, r.inflated);
    // every position of the stream has a member in the table
    for (uint64_t p : {(uint64_t)0, r.inflated / 2, r.inflated})
      expect(p / BGZF_PAYLOAD < r.coff.size(), "a position without a member", n, (uint64_t)at, p);
  }
  return r;
}

int main() {
  std::vector<uint8_t> f;
  const uint32_t payload[3] = {BGZF_PAYLOAD, BGZF_PAYLOAD, 100};
  size_t starts[4] = {0, 0, 0, 0};
  for (int k = 0; k < 3; k++) { member(f, payload[k]); starts[k + 1] = f.size(); }
  expect(f.size() == 65311 + 65311 + 131, "the stream's size", f.size());
  // every truncation: sound exactly at the members' ends (and with no bytes at all), refused everywhere else
  for (size_t n = 0; n <= f.size(); n++) {
    const BaiMembers r = walk(f, n, -1, 0);
    int whole = -1;
    for (int k = 0; k < 4; k++) if (starts[k] == n) whole = k;
    if (whole >= 0) {
      expect(r.error == BAI_MEMBERS_OK && r.n_members() == (size_t)whole, "whole members that are refused", n, r.error, r.n_members());
      expect(r.inflated == (whole == 3 ? 2ull * BGZF_PAYLOAD + 100 : (uint64_t)whole * BGZF_PAYLOAD), "a wrong sum of ISIZE", n, r.inflated);
    } else {
      size_t start = 0;
      for (int k = 0; k < 3; k++) if (starts[k] < n) start = starts[k];
      expect(r.error == (n - start < 18 ? BAI_TRUNCATED_MEMBER : BAI_BAD_BSIZE), "a cut member that is not refused as such", n, r.error, r.at);
      expect(r.at == (n - start < 18 ? start : start + 16), "a refusal at another byte", n, r.error, r.at);
    }
  }
  // every byte of the three headers and of the three ISIZE fields, three values each
  for (int k = 0; k < 3; k++)
    for (int part = 0; part < 2; part++)
      for (size_t b = 0; b < (part ? 4u : 18u); b++) {
        const size_t at = part ? starts[k + 1] - 4 + b : starts[k] + b;
        const int values[3] = {0x00, 0xFF, (uint8_t)~f[at]};
        for (int value : values) {
          const BaiMembers r = walk(f, f.size(), (long)at, value);
          const bool read = part || b < 4 || b >= 10;  // (MTIME, XFL and OS are not looked at)
          bool sound = value == f[at] || !read;
          if (k == 2 && part) {  // the last member's ISIZE: any value from 1 to 65280 is a member (the calls then compare the sum with the stream)
            uint32_t isize = 0;
            for (size_t q = 0; q < 4; q++) isize |= (uint32_t)(q == b ? (uint8_t)value : f[starts[3] - 4 + q]) << (8 * q);
            sound = isize >= 1 && isize <= BGZF_PAYLOAD;
            expect(!sound || value == f[at] || !bai_is_the_stream(r, 2ull * BGZF_PAYLOAD + 100), "another ISIZE that passes for the stream", at, (uint64_t)value);
          }
          if (sound) expect(r.error == BAI_MEMBERS_OK && r.n_members() == 3, "sound members that are refused", at, (uint64_t)value, r.error);
          else expect(r.error != BAI_MEMBERS_OK, "a damaged member that passes", at, (uint64_t)value);
          if (k < 2) (void)walk(f, starts[2], (long)at, value);
        }
      }
  // virtual offsets at the edges of the table
  {
    const BaiMembers r = walk(f, f.size(), -1, 0);
    expect(bai_voff(0, r.coff.data(), 0) == 0 && bai_voff(5, r.coff.data(), r.inflated) == (((uint64_t)5 + starts[2]) << 16 | 100), "the stream's ends as virtual offsets");
    const BaiMembers full = walk(f, starts[2], -1, 0);
    expect(bai_voff(5, full.coff.data(), full.inflated) == ((uint64_t)5 + starts[2]) << 16, "the end of a full last member");
  }
  if (failures) return 1;
  printf("bai_plan_asan: ok\n");
  return 0;
}
