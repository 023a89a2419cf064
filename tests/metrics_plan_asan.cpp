// metrics_plan_asan.cpp — the metrics pass's plan (elprep_amd/csrc/metrics_plan.hpp) and the optical-duplicate name parser
// (elprep_amd/csrc/optical_name.hpp) on their own under the sanitizers: build with
// g++ -fsanitize=address,undefined -fno-sanitize-recover=all  and run.  The edge cases of tests/test_metrics_plan_cpu.py and
// tests/test_optical_name_host_cpu.py, with every block mx_finish reads or fills allocated at exactly its size and every name in a
// buffer that ends with it, so that an index one past an end, a shift by the width of the type or a signed overflow trips the
// sanitizer.  Exit status 0 and no report: passed (tests/test_metrics_plan_cpu.py runs it).
#include "../elprep_amd/csrc/metrics_plan.hpp"
#include "../elprep_amd/csrc/optical_name.hpp"

#include <climits>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>

using namespace elp;

static int failures = 0;
static void expect(bool ok, const char *what, long long a = 0, long long b = 0) {
  if (ok) return;
  failures++;
  fprintf(stderr, "metrics_plan_asan: %s (%lld, %lld)\n", what, a, b);
}

static void sizes() {
  const MxSizes one(1, 1, 1, 0);
  expect(one.ncell == 14 && one.npr == 2 && one.cells == 16 && one.block == 24 && one.counters_lds == 64 && one.counters_grid == 1 && one.chunk == 1024 &&
             one.lcap == 8, "sizes of one record");
  const MxSizes none(0, 0, 1, 0);
  expect(none.counters_grid == 0 && none.chunk == 0 && none.origin_grid == 0 && none.ndig == 1, "no records");
  const uint64_t ns[] = {255, 256, 65535, 65536, (1ull << 24) - 1, 1ull << 24, (1ull << 32) - 1, ~0ull};
  const int digits[] = {1, 2, 2, 3, 3, 4, 4, 4};
  for (int k = 0; k < 8; k++) expect(MxSizes(ns[k], 0, 1, 0).ndig == digits[k], "ndig", k, MxSizes(ns[k], 0, 1, 0).ndig);
  expect(MxSizes(2097152, 0, 1, 0).chunk == 1024 && MxSizes(2097153, 0, 1, 0).chunk == 2048 && MxSizes(2097153, 0, 1, 0).counters_grid == 2048, "chunk");
  expect(!MxSizes(10, 99, 108, 0).lds_refused && MxSizes(10, 99, 109, 0).lds_refused, "lds refusal");
  expect(MxSizes(10, 83, 1, 32).lds_bins == 32 && MxSizes(10, 84, 1, 32).lds_bins == 0 && MxSizes(10, 1169, 1, 2).lds_bins == 2 &&
             MxSizes(10, 1170, 1, 2).lds_bins == 0 && MxSizes(10, 0, 1, 33).lds_bins == 32, "lds bins");
  expect(MxSizes(10, INT_MAX / 64, 65536, 1 << 20).cells > 0, "large arguments");  // (no signed overflow on the way)
}

static void layout() {
  for (uint64_t n : {2ull, 3ull, 255ull, 256ull, 2097153ull, (1ull << 32) - 1}) {
    const MxListScratch ls(MxSizes(n, 0, 1, 0).lcap);
    for (int kf = 0; kf < 2; kf++)
      for (int vf = 0; vf < 2; vf++) {
        const MxListScratch::Groups g = ls.groups(kf, vf);
        const size_t L = n / 2;
        expect(g.head == ls.keys_half(!kf) && g.gidx + L <= g.head + 2 * ls.lcap && g.gstart == ls.vals_half(!vf) && g.gstart + L + 1 <= g.gstart + ls.lcap &&
                   g.gstart + L + 1 <= ls.words, "groups outside their halves", (long long)n, kf * 2 + vf);
      }
  }
  for (uint32_t total : {1u, 8u, 9u, 262145u, 0xFFFFFFF8u, 0xFFFFFFFFu}) {
    const MxSetScratch s(total);
    expect(s.tp >= total && s.tp % 8 == 0 && s.lkeys_tmp + 2 * s.tp <= s.words3 && s.zero == s.linfo && s.zero + s.zero_words == s.lvals, "slot 3", total);
  }
}

// a block of exactly S.cells cells, counters and histograms of exactly their sizes
static void finish(int n_lib, int n_split, int hist_len) {
  const MxSizes S(100, n_lib, n_split, hist_len);
  std::unique_ptr<unsigned long long[]> h(new unsigned long long[S.cells]);
  for (size_t k = 0; k < S.cells; k++) h[k] = 0;
  for (int l = 0; l <= n_lib; l++) {
    for (int sp = 0; sp < n_split; sp++) h[S.pair_reads + (size_t)sp * (n_lib + 1) + l] = 2 * l + 3;  // odd: halving loses one per split
    if (hist_len) {
      h[S.origins + l] = 5 + l;
      h[S.hist + (size_t)l * 3 * hist_len + hist_len - 1] = 5;  // five sets in the last bin of the first histogram
    }
  }
  std::unique_ptr<int64_t[]> counters(new int64_t[(size_t)(n_lib + 1) * ELP_NCTR]);
  std::unique_ptr<int64_t[]> hist(hist_len ? new int64_t[(size_t)(n_lib + 1) * 3 * hist_len] : nullptr);
  mx_finish(S, h.get(), counters.get(), hist.get());
  for (int l = 0; l <= n_lib; l++) {
    expect(counters[l * ELP_NCTR + 1] == (int64_t)n_split * (l + 1), "pairs halved per split", l, counters[l * ELP_NCTR + 1]);
    if (hist_len) {
      const int64_t *out = hist.get() + (size_t)l * 3 * hist_len;
      const int64_t in_one = hist_len == 2 ? 5 : 0;  // (with two bins the sets are in bin 1 already)
      expect(out[1] == in_one + l && out[hist_len + 1] == l, "lone origins", l, out[1]);
    }
  }
}

// the name's bytes 8 k .. 8 k + 7 without reading past its end (the kernels rely on the column's padding instead)
static Tile parse(const std::string &name, bool *bad) {
  std::unique_ptr<uint8_t[]> buf(new uint8_t[name.size() ? name.size() : 1]);
  memcpy(buf.get(), name.data(), name.size());
  const uint32_t len = (uint32_t)name.size();
  *bad = false;
  return tile_parse(len, bad, [&](uint32_t k) {
    uint64_t w = 0;
    for (uint32_t j = 0; j < 8 && 8 * k + j < len; j++) w |= (uint64_t)buf[8 * k + j] << (8 * j);
    return w;
  });
}

static void names() {
  struct Case { const char *name; long long t, x, y; bool bad; };
  const Case cases[] = {
      {"", -1, -1, -1, false},
      {"a:b:1:2:3", 1, 2, 3, false},
      {"a:1:FC:1:1101:-42:+0042", 1101, -42, 42, false},
      {"a:b:1:9223372036854775807:-9223372036854775808", 1, LLONG_MAX, LLONG_MIN, false},
      {"a:b:1:9223372036854775808:3", -1, -1, -1, true},
      {"a:b:1:-9223372036854775809:3", -1, -1, -1, true},
      {"a:b:1:99999999999999999999999999999999:3", -1, -1, -1, true},
      {"a:b:1:0000000000000000000009223372036854775807:3", 1, LLONG_MAX, 3, false},
      {"a:b:1::3", -1, -1, -1, true},
      {"a:b:1:+:3", -1, -1, -1, true},
      {"a:b:1:1 :3", -1, -1, -1, true},
      {"a:b:1:\xff:3", -1, -1, -1, true},
      {"a:b:x:2:3:4", -1, -1, -1, false},
      {"::::", -1, -1, -1, true},
      {":::::::", -1, -1, -1, false},
  };
  for (const Case &c : cases) {
    bool bad;
    const Tile t = parse(c.name, &bad);
    expect(t.t == c.t && t.x == c.x && t.y == c.y && bad == c.bad, c.name, t.t, bad);
  }
  // names of 47 .. 57 bytes: the last word is partial, full, and one byte into the next
  for (size_t len : {47u, 48u, 49u, 56u, 57u}) {
    std::string nm = "u" + std::string(len - 11, 'N') + ":9:7:-8:+9";
    bool bad;
    const Tile t = parse(nm, &bad);
    expect(nm.size() == len && t.t == 7 && t.x == -8 && t.y == 9 && !bad, "a long name", (long long)len);
  }
  expect(go_abs_diff(LLONG_MAX, LLONG_MIN) == 1 && go_abs_diff(0, LLONG_MIN) == LLONG_MIN && go_abs_diff(LLONG_MIN, LLONG_MAX) == 1 &&
             go_abs_diff(-2, LLONG_MAX) == LLONG_MAX && go_abs_diff(5, 7) == 2, "go_abs_diff");
  const Member a{7, 0, 0, 2, 0}, b{7, LLONG_MIN, 0, 2, 0}, other_rg{7, 0, 0, 4, 0}, no_tile{-1, 0, 0, 2, 0};
  expect(optical_close(a, b, 0) && !optical_close(a, b, -1) && !optical_close(a, other_rg, 100) && !optical_close(no_tile, no_tile, 100), "optical_close");
}

int main() {
  sizes();
  layout();
  finish(0, 1, 0);
  finish(2, 3, 2);
  finish(2, 3, 8);
  finish(99, 108, 33);
  names();
  if (failures) return 1;
  printf("metrics_plan_asan: ok\n");
  return 0;
}
