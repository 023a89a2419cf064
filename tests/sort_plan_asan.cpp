// sort_plan_asan.cpp — the sorts' plan (elprep_amd/csrc/sort_plan.hpp) on its own under the sanitizers: build with
// g++ -fsanitize=address,undefined -fno-sanitize-recover=all  and run.  The edge cases of tests/test_sort_plan_cpu.py, with every
// array the plan reads or fills allocated at exactly its size, so that an index one past an end, a shift by the width of the type or
// a signed overflow trips the sanitizer.  Exit status 0 and no report: passed (tests/test_sort_plan_cpu.py runs it).
#include "../elprep_amd/csrc/sort_plan.hpp"

#include <cstdio>
#include <cstring>
#include <memory>

using namespace elp;

static int failures = 0;
static void expect(bool ok, const char *what, long a = 0, long b = 0) {
  if (ok) return;
  failures++;
  fprintf(stderr, "sort_plan_asan: %s (%ld, %ld)\n", what, a, b);
}

// a value set of the first `count` of the values v0, v0 + step, ... (mod 256)
static void value_set(uint32_t *set, int count, int v0 = 0, int step = 1) {
  memset(set, 0, 32);
  for (int k = 0; k < count; k++) { const int v = (v0 + k * step) & 255; set[v >> 5] |= 1u << (v & 31); }
}

static void key_format() {
  const uint64_t ns[] = {0, 1, 2, 3, 4, (1ull << 31) - 1, 1ull << 31, (1ull << 32) - 1, 1ull << 32, ~0ull};
  const int want[] = {1, 1, 2, 2, 3, 31, 32, 32, 32, 32};
  for (int k = 0; k < 10; k++) expect(index_bits(ns[k]) == want[k], "index_bits", (long)k, index_bits(ns[k]));
  expect(sort_words(32, 32, 0) && !sort_words(33, 32, 0) && !sort_words(32, 32, 1) && !sort_words(0, 1, 0), "sort_words");
  expect(key_width(0, 0).key_bits == 3 && key_width(0x7FFFFFFFu, 65535).key_bits == 49 && key_width(0xFFFFFFFFu, 0x7FFFFFFF).key_bits == 65, "key_width");
}

static void runs() {
  expect(bounds_cap(0) == 2 && bounds_cap(1) == 3 && bounds_cap(14) == 16 && bounds_cap(0xFFFFFFFFull) == 0xFFFFFFFFull / 48 + 16, "bounds_cap");
  expect(segbits(0) == 0 && segbits(1) == 0 && segbits(2) == 2 && segbits(255) == 8 && segbits(256) == 9 && segbits(0x7FFFFFFFu) == 31, "segbits");
  for (uint32_t nr : {0u, 1u, TIE_HEAD, TIE_HEAD + 1}) {
    std::vector<uint32_t> s(nr), e(nr);
    for (uint32_t r = 0; r < nr; r++) { s[r] = 100 * (nr - 1 - r); e[(r * 7) % (nr ? nr : 1)] = 100 * r + 48; }  // 7 and nr coprime: a shuffle
    LongRuns lr;
    expect(long_runs(s, e, &lr) && lr.nr == nr && lr.nu == 49 * nr && lr.first.size() == (size_t)nr + 1, "long_runs", nr, lr.nu);
    for (uint32_t r = 0; r < nr; r++) expect(lr.starts[r] == 100 * r && lr.first[r] == 49 * r, "long_runs' order", nr, r);
  }
  LongRuns lr;
  expect(!long_runs({10}, {9}, &lr) && !long_runs({10, 59}, {59, 100}, &lr) && long_runs({10, 60}, {59, 100}, &lr) && !long_runs({1, 2}, {3}, &lr), "long_runs' refusals");
  expect(long_runs({0}, {0xFFFFFFFEu}, &lr) && lr.nu == 0xFFFFFFFFu, "one run over everything");
  expect(!run_counts_ok(3, 2, 8) && !run_counts_ok(3, 3, 2) && run_counts_ok(3, 3, 3), "run_counts_ok");
}

static void layout() {
  for (uint64_t n : {1ull, 13ull, 14ull, 15ull, 47ull, 48ull, 1000ull, (1ull << 32) - 1}) {
    const SortScratch s(n);
    expect(s.starts == 4 && s.starts + s.cap <= s.ends && s.ends + s.cap <= s.flags, "bounds outside their slot", (long)n, (long)s.cap);
  }
  for (uint32_t maxq : {0u, 1u, 2u, 17u, 18u, 994u, 1000u})
    for (uint32_t nu : {49u, 50u, 51u, 52u, 524288u, 524289u, 33554432u, 33554433u})
      for (uint32_t nr : {1u, 2u, 3u, 4u}) {
        const TieScratch t(nu, nr, maxq);
        expect(t.rw % 16 == 0 && t.rw >= t.m_bytes && t.rw - t.m_bytes < 16 && t.u_words % 4 == 0, "row width", maxq, t.rw);
        expect(t.d_first + nr + 1 <= t.u_words && t.u_words * 4 + (t.use_rows ? (uint64_t)nu * t.rw : 0) <= t.words3 * 4, "slot 3", nu, nr);
        expect(t.use_rows == ((uint64_t)nu * t.rw <= (512ull << 20)), "use_rows", nu, t.rw);
      }
  const QnScratch q0(0), q(1000);
  expect(q0.words3 == 2 && q.d_lut * 4 + 1000 * 256 <= q.words3 * 4, "queryname slot 3");
}

static void rank_tables() {
  const int counts[] = {1, 2, 3, 4, 5, 128, 129, 256}, widths[] = {1, 1, 2, 2, 3, 7, 8, 8};
  for (int k = 0; k < 8; k++) {
    std::unique_ptr<uint32_t[]> set(new uint32_t[8]);
    std::unique_ptr<uint8_t[]> row(new uint8_t[256]);
    value_set(set.get(), counts[k], 255, 101);  // (101 is odd: the values are distinct)
    const int nv = rank_row(set.get(), row.get());
    expect(nv == counts[k] && value_count(set.get()) == counts[k] && rank_bits(nv) == widths[k], "rank width", counts[k], rank_bits(nv));
  }
  std::unique_ptr<uint32_t[]> live(new uint32_t[32]);
  for (int w = 0; w < 32; w++) live[w] = 0xFFFFFFFFu;
  expect(live_positions(live.get(), 1015).size() == 1015 && live_positions(live.get(), 0).empty(), "live_positions");
  // the queryname sort's fields at the longest name: every position live with all 256 values, a NUL seen, records that are not output
  const uint32_t maxq = 1000;
  std::unique_ptr<uint32_t[]> sets(new uint32_t[QnScratch(maxq).vwords]);
  for (size_t k = 0; k < QnScratch(maxq).vwords; k++) sets[k] = 0xFFFFFFFFu;
  const RankFields f = qn_fields(sets.get(), maxq, true);
  expect(f.n() == 1002 && f.lut.size() == 256000 && f.pos.front() == QN_STATE && f.pos.back() == QN_LEN && f.bits[1] == 8, "qn_fields", f.n());
  const std::vector<FieldCut> cuts = lsd_cuts(f.bits);
  int top = f.n();
  for (const FieldCut &c : cuts) {
    expect(c.hi == top && c.lo < c.hi && c.total <= 64 && c.hi - c.lo <= 64, "an LSD cut", c.lo, c.hi);
    std::unique_ptr<uint8_t[]> shift(new uint8_t[c.hi - c.lo]);
    field_shifts(f.bits, c, shift.get());
    expect(shift[c.hi - c.lo - 1] == 0 && shift[0] + f.bits[c.lo] == c.total, "the shifts of a cut", c.lo, c.hi);
    top = c.lo;
  }
  expect(top == 0, "LSD cuts that do not reach the first field", top);
  // the coordinate sort's at TIE_MAX_PACKED positions
  std::vector<uint16_t> lp(TIE_MAX_PACKED);
  for (int k = 0; k < TIE_MAX_PACKED; k++) lp[k] = (uint16_t)(k * 10);
  std::unique_ptr<uint32_t[]> tsets(new uint32_t[TIE_MAX_PACKED * 8]);
  for (int k = 0; k < TIE_MAX_PACKED; k++) value_set(tsets.get() + k * 8, 1 + (k * 37) % 256, k);
  const RankFields t = tie_fields(lp, tsets.get());
  expect(t.n() == TIE_MAX_PACKED && t.lut.size() == (size_t)TIE_MAX_PACKED * 256 && t.lut.size() <= (size_t)TIE_MAX_PACKED * 64 * 4, "tie_fields");
  expect(rank_keys_apply(TIE_MAX_PACKED) && !rank_keys_apply(TIE_MAX_PACKED + 1) && !rank_keys_apply(0), "rank_keys_apply");
}

static void packing() {
  const std::vector<int> full(8, 8), ones(70, 1), none;
  std::vector<int> over(full);
  over.push_back(1);
  expect(pack_prefix(full, 0).hi == 8 && pack_prefix(over, 0).hi == 8 && pack_prefix(full, 1).hi == 7 && pack_prefix(ones, 0).hi == 64, "pack_prefix");
  expect(pack_prefix({3, 5, 2}, 59).hi == 1 && pack_prefix({3, 5, 2}, 62).hi == 0 && pack_prefix(none, 0).hi == 0, "pack_prefix beside reserved bits");
  expect(lsd_cuts(none).empty() && lsd_cuts(ones).size() == 2 && lsd_cuts(over).size() == 2, "lsd_cuts");
  expect(key_then_compare(0, 27, 8) && !key_then_compare(1, 27, 8) && !key_then_compare(0, 57, 8), "key_then_compare");
  const std::vector<FieldCut> bc = byte_cuts(97);
  expect(bc.size() == 13 && bc.front().lo == 89 && bc.front().hi == 97 && bc.back().lo == 0 && bc.back().hi == 1 && byte_cuts(0).empty(), "byte_cuts");
  expect(key_digits(0) == 0 && key_digits(1) == 1 && key_digits(64) == 8, "key_digits");
}

int main() {
  key_format();
  runs();
  layout();
  rank_tables();
  packing();
  if (failures) return 1;
  printf("sort_plan_asan: ok\n");
  return 0;
}
