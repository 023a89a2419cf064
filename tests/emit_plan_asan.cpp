// emit_plan_asan.cpp — bam_cut_piece (elprep_amd/csrc/emit_plan.hpp), elp_stage_bam's walk over bytes and offsets it has no reason to
// trust, and the emitters' pass functions at their edges, on their own under the sanitizers: build with
// g++ -fsanitize=address,undefined -fno-sanitize-recover=all  and run.
// A stream of three records (block_size 40, 50 and 36: 44, 54 and 40 bytes, 138 in all) is cut from a heap buffer of EXACTLY n bytes
// for every truncation n in [0, 138], with the 256 MiB limit and with limits of a few bytes, then with every single byte of the three
// block_size fields set to 0x00, to 0xFF and to its complement; the same records are cut by offsets from heap arrays of EXACTLY
// records + 1 entries, sound and with every single entry damaged - a read one byte or one entry behind a buffer trips the sanitizer.
// Every call must succeed or return one of the error kinds, and what it lists must lie inside the buffer.  Exit status 0 and no
// report: passed (tests/test_emit_plan_cpu.py runs it).
#include "../elprep_amd/csrc/emit_plan.hpp"

#include <cstdio>
#include <memory>

using namespace elp;

static int failures = 0;
static void expect(bool ok, const char *what, uint64_t a = 0, uint64_t b = 0, uint64_t c = 0) {
  if (ok) return;
  failures++;
  fprintf(stderr, "emit_plan_asan: %s (%llu, %llu, %llu)\n", what, (unsigned long long)a, (unsigned long long)b, (unsigned long long)c);
}

static void record(std::vector<uint8_t> &f, uint32_t block_size) {
  for (int k = 0; k < 4; k++) f.push_back((uint8_t)(block_size >> (8 * k)));
  for (uint32_t k = 0; k < block_size; k++) f.push_back((uint8_t)(k * 5 + block_size));
}

// all pieces of the first n bytes of `f`, from a buffer of exactly n bytes (byte `at` replaced by `value` if at >= 0) or, with `ro`,
// from an offset array of exactly ro->size() entries.  Returns the records found, or -1 - the error kind
static long cut_all(const std::vector<uint8_t> &f, size_t n, uint64_t limit, int at, int value, const std::vector<uint64_t> *ro, BamCut *last) {
  std::unique_ptr<uint8_t[]> buf(new uint8_t[n]);
  if (n) memcpy(buf.get(), f.data(), n);
  if (at >= 0) buf[at] = (uint8_t)value;
  std::unique_ptr<uint64_t[]> offs;
  uint64_t n_records = 0;
  if (ro) {
    offs.reset(new uint64_t[ro->size()]);
    memcpy(offs.get(), ro->data(), ro->size() * 8);
    n_records = ro->size() - 1;
  }
  // (elp_stage_bam refuses offsets that do not run from 0 to n before it cuts; without that a piece may be empty: no progress to insist on)
  const bool ends_sound = !ro || (ro->front() == 0 && ro->back() == n);
  uint64_t at_byte = 0, at_rec = 0, records = 0;
  while (at_byte < n) {
    BamCut r = bam_cut_piece(buf.get(), n, offs.get(), n_records, at_byte, at_rec, limit);
    *last = r;
    expect(r.error >= BAM_CUT_OK && r.error <= BAM_CUT_BAD_BLOCK_SIZE, "an error value that is none of the kinds", n, limit, r.error);
    if (r.error) {
      expect(r.error == BAM_CUT_BAD_OFFSETS ? r.at < n_records : r.at < n, "an error behind the buffer", n, limit, r.at);
      expect(!r.text().empty(), "an error without a text", n, limit, r.error);
      return -(long)r.error;
    }
    if (!ends_sound) {  // only: no read outside the arrays, and an end to it
      if (r.off.size() < 2 || r.end <= at_byte || r.end > n) return (long)records;
      records += r.off.size() - 1;
      at_byte = r.end;
      at_rec = r.next_rec;
      continue;
    }
    expect(r.off.size() >= 2 && r.off[0] == 0 && r.end > at_byte && r.end <= n && r.off.back() == r.end - at_byte, "a piece out of place", n, limit, r.end);
    uint64_t longest = 0;
    for (size_t k = 0; k + 1 < r.off.size(); k++) {
      expect(r.off[k + 1] >= r.off[k] + 36, "a record shorter than 36 bytes", n, limit, k);
      expect(k == 0 || r.off[k] < limit, "a record that starts behind the limit", n, limit, k);
      longest = std::max(longest, r.off[k + 1] - r.off[k]);
    }
    expect(longest == r.max_raw_rec, "a wrong longest record", n, limit, r.max_raw_rec);
    expect(!ro || r.next_rec == at_rec + r.off.size() - 1, "a wrong next record", n, limit, r.next_rec);
    records += r.off.size() - 1;
    at_byte = r.end;
    at_rec = r.next_rec;
  }
  return (long)records;
}

int main() {
  std::vector<uint8_t> f;
  const uint32_t bs[3] = {40, 50, 36};
  size_t ends[3];
  std::vector<uint64_t> starts(1, 0);
  for (int k = 0; k < 3; k++) { record(f, bs[k]); ends[k] = f.size(); starts.push_back(f.size()); }
  expect(f.size() == 138, "the stream's size", f.size());
  const uint64_t limits[5] = {BAM_PIECE_BYTES, 1, 44, 45, 300};
  BamCut last;
  // every truncation: whole records are found, anything else is an error at the record that is cut - fewer than 4 bytes of it are a
  // truncated record, more a block_size that reaches behind the bytes
  for (uint64_t limit : limits)
    for (size_t n = 0; n <= f.size(); n++) {
      const long got = cut_all(f, n, limit, -1, 0, nullptr, &last);
      size_t whole = 0, start = 0;
      while (whole < 3 && ends[whole] <= n) start = ends[whole++];
      if (n == start) {
        expect(got == (long)whole, "whole records that are not found", n, limit, (uint64_t)got);
      } else {
        expect(got == (n - start < 4 ? -(long)BAM_CUT_TRUNCATED : -(long)BAM_CUT_BAD_BLOCK_SIZE) && last.at == start, "a cut record that is found, or an error elsewhere", n, limit, last.at);
        expect(n - start < 4 || last.block_size == bs[whole], "a wrong block_size in the error", n, limit, last.block_size);
      }
    }
  // every byte of the three block_size fields, three values each, in the whole stream and in one that ends with the second record
  for (uint64_t limit : limits)
    for (int r = 0; r < 3; r++)
      for (int b = 0; b < 4; b++) {
        const int at = (int)starts[r] + b;
        const int values[3] = {0x00, 0xFF, (uint8_t)~f[at]};
        for (int value : values) {
          const long got = cut_all(f, f.size(), limit, at, value, nullptr, &last);
          expect(value != f[at] || got == 3, "the stream as it is that is refused", limit, (uint64_t)at, (uint64_t)value);
          if (r < 2) cut_all(f, ends[1], limit, at, value, nullptr, &last);
        }
      }
  // the caller's offsets: sound, then every entry damaged (the first and the last too: elp_stage_bam checks those two before it cuts,
  // the function must hold without that)
  for (uint64_t limit : limits) {
    expect(cut_all(f, f.size(), limit, -1, 0, &starts, &last) == 3, "sound offsets that are refused", limit);
    for (size_t e = 0; e < starts.size(); e++) {
      const uint64_t values[6] = {e ? 0 : 36, starts[e] - 1, starts[e] + 1, (e ? starts[e - 1] : 0) + 35, f.size() + 1, ~0ull};
      for (uint64_t value : values) {
        std::vector<uint64_t> ro = starts;
        ro[e] = value;
        const long got = cut_all(f, f.size(), limit, -1, 0, &ro, &last);
        expect(got >= -(long)BAM_CUT_BAD_OFFSETS, "damaged offsets with an error of the walk", limit, e, value);
      }
    }
  }
  // the pass functions at their edges
  for (OutFormat fmt : {OutFormat::BAM, OutFormat::BGZF, OutFormat::SAM})
    for (uint64_t held : {0ull, 1ull, 65279ull})
      for (uint64_t chunk : {0ull, 1ull, 65279ull, 65280ull, 65281ull, 0xFC000000ull, 0xFFFFFFFFull})
        for (bool is_last : {false, true}) {
          const uint64_t h = fmt == OutFormat::BGZF ? held : 0;
          const EmitPass p = emit_pass(fmt, h, chunk, is_last);
          expect(p.pass_bytes == h + chunk && p.frame_bytes + p.carry_bytes == p.pass_bytes, "a pass that loses bytes", h, chunk, is_last);
          expect(p.carry_bytes < BGZF_PAYLOAD && (!is_last || p.carry_bytes == 0), "a carry of a member or more, or behind the last pass", h, chunk, is_last);
          expect(p.out_bound >= p.frame_bytes && p.out_bound <= emit_query_bytes(fmt, h + chunk), "a bound below the frame or above the query's", h, chunk, is_last);
          expect(emit_fits(0, p.out_bound, p.out_bound) && (p.out_bound == 0 || !emit_fits(0, p.out_bound, p.out_bound - 1)), "the capacity test", h, chunk, is_last);
        }
  for (uint64_t raw : {0ull, 10ull, 64ull, 300ull, 4000ull, 1ull << 32, 1ull << 40})
    for (OutFormat fmt : {OutFormat::BAM, OutFormat::SAM}) {
      const uint64_t bound = emit_rec_bound(fmt, raw, 0xFFFFFFFFu);
      for (int tune : {0, 1, 97, 1 << 30}) {
        const uint32_t n = emit_pass_records(bound, tune);
        expect(n >= 1 && n <= EMIT_PASS_RECORDS && (tune <= 0 || n <= (uint32_t)tune) && (n == 1 || n * bound <= EMIT_PASS_BYTES), "a pass of no record or past 4 GiB", raw, tune, n);
      }
    }
  for (uint32_t cnt : {0u, 1u, 1000u, 1u << 21, 0xFFFFFFFFu}) {
    const EmitScratch4 s(cnt);
    expect(s.sizes + cnt <= s.offs && s.offs + cnt <= s.err && s.err + 1 <= s.words, "slot 4's sub-buffers overlap", cnt);
  }
  if (failures) return 1;
  printf("emit_plan_asan: ok\n");
  return 0;
}
