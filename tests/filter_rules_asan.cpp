// filter_rules_asan.cpp — the filters' per-record rules and scratch layouts (elprep_amd/csrc/filter_rules.hpp) on their own under the
// sanitizers: build with  g++ -fsanitize=address,undefined -fno-sanitize-recover=all  and run.  clean_cigar writes into a buffer of
// exactly the count it returned, the strict walk reads records whose buffer ends with the record (also cut short inside a field), and
// every part of a layout is touched in a block of exactly the bytes asked for - so that an index one past an end or a signed overflow
// trips the sanitizer.  Exit status 0 and no report: passed (tests/test_filter_rules_cpu.py runs it).
#include "../elprep_amd/csrc/filter_rules.hpp"

#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

using namespace elp;

static int failures = 0;
static void expect(bool ok, const char *what, long long a = 0, long long b = 0) {
  if (ok) return;
  failures++;
  fprintf(stderr, "filter_rules_asan: %s (%lld, %lld)\n", what, a, b);
}

static uint32_t op(uint32_t len, char c) { return (len << 4) | (uint32_t)(strchr("MIDNSHP=X", c) - "MIDNSHP=X"); }

// count, then write into exactly that many words; the CIGAR itself in a buffer of exactly its size
static std::vector<uint32_t> clean(const std::vector<uint32_t> &cig, uint16_t flag, int32_t pos, int32_t length, int *rc) {
  std::unique_ptr<uint32_t[]> ops(new uint32_t[cig.size() ? cig.size() : 1]);
  for (size_t k = 0; k < cig.size(); k++) ops[k] = cig[k];
  bool c0 = false, c1 = false;
  const int n = clean_cigar(ops.get(), (int)cig.size(), flag, pos, length, nullptr, &c0);
  *rc = n;
  if (n < 0) return {};
  std::unique_ptr<uint32_t[]> out(new uint32_t[n ? n : 1]);
  const int m = clean_cigar(ops.get(), (int)cig.size(), flag, pos, length, out.get(), &c1);
  expect(m == n && c0 == c1, "count-only and writing call differ", n, m);
  return std::vector<uint32_t>(out.get(), out.get() + n);
}

static void cigars() {
  int rc;
  // the hand-derived rows of tests/test_clean_sam_kat.py (reference of 1000 bases)
  expect(clean({op(100, 'M')}, 0, 951, 1000, &rc) == std::vector<uint32_t>{op(49, 'M'), op(149, 'S')}, "100M at 951");
  expect(clean({op(10, 'S'), op(40, 'M')}, 0, 981, 1000, &rc) == std::vector<uint32_t>{op(10, 'S'), op(9, 'M'), op(69, 'S')}, "10S40M at 981");
  expect(clean({op(30, 'M'), op(10, 'I'), op(60, 'M')}, 0, 961, 1000, &rc) == std::vector<uint32_t>{op(30, 'M'), op(148, 'S')}, "30M10I60M at 961");
  expect(clean({op(30, 'M'), op(20, 'D'), op(50, 'M')}, 0, 961, 1000, &rc) == std::vector<uint32_t>{op(30, 'M'), op(20, 'D'), op(119, 'S')}, "30M20D50M");
  clean({op(5, 'M'), op(5, 'M'), op(15, 'M'), op(10, 'D'), op(65, 'M')}, 0, 961, 1000, &rc);
  expect(rc == -1, "the reference's panic", rc);
  expect(clean({op(100, 'M')}, 0, 901, 1000, &rc) == std::vector<uint32_t>{op(100, 'M')} && rc == 1, "ends at the reference's end");
  expect(clean({op(100, 'M')}, 0x4, 951, 1000, &rc) == std::vector<uint32_t>{op(100, 'M')}, "unmapped");
  expect(clean({op(10, 'M')}, 0, 5, 0, &rc) == std::vector<uint32_t>{op(5, 'S')}, "no reference, POS 5");
  expect(clean({}, 0, 5, 1000, &rc).empty() && rc == 0, "no CIGAR");
  clean({}, 0, 5, 0, &rc);  // End = 4 > 0 with nothing to clip: no operation, no write
  expect(rc == 0, "no CIGAR, no reference", rc);
  // the 28-bit limit: 99M + S of x + 99 (tests/test_filter_rules_cpu.py works it out)
  const uint32_t top = (1u << 28) - 1;
  expect(clean({op(top - 99, 'M')}, 0, 901, 1000, &rc) == std::vector<uint32_t>{op(99, 'M'), op(top, 'S')}, "S of 2^28 - 1");
  clean({op(top - 98, 'M')}, 0, 901, 1000, &rc);
  expect(rc == -2, "S of 2^28", rc);
  clean({op(3, 'M')}, 0, 50, 0, &rc);  // S of 3 - 50 + ... : negative
  expect(rc == -2, "negative clip", rc);
  const CigarFacts f = cigar_facts(nullptr, 0);
  expect(f.ref_len == 0 && f.read_len == 0 && f.exact, "facts of no CIGAR");
}

// a record (block_size in front) with these optional-field bytes, in a buffer that ends with the record - or `cut` bytes earlier, with
// block_size lowered to match (what the walk must survive: staging refuses such records, the rule must not read past them)
static int strict(const std::string &fields, size_t cut = 0) {
  std::string body(32, '\0');
  body[8] = 2;                 // l_read_name
  body[12] = 1;                // n_cigar_op
  body[16] = 3;                // l_seq
  body += std::string("r\0", 2) + std::string("\x30\0\0\0", 4) + std::string("\x12\x40", 2) + std::string("\x1e\x1e\x1e", 3) + fields;
  body.resize(body.size() - cut);
  const uint32_t bs = (uint32_t)body.size();
  std::unique_ptr<uint8_t[]> buf(new uint8_t[4 + bs]);
  for (int k = 0; k < 4; k++) buf[k] = (uint8_t)(bs >> (8 * k));
  memcpy(buf.get() + 4, body.data(), bs);
  const uint8_t *rec = buf.get() + 4, *end = rec + ld_u32(buf.get());
  return strict_decide(strict_walk(bam_fields_at(rec), end));
}

static void strict_rule() {
  const std::string good = std::string("X0C\1", 4) + std::string("X1C\0", 4) + std::string("XMC\0", 4) + std::string("XOC\0", 4) + std::string("XGC\0", 4);
  expect(strict(good) == STRICT_KEEP, "all five");
  expect(strict("") == STRICT_REJECT, "no fields");
  for (size_t cut = 1; cut <= good.size(); cut++) expect(strict(good, cut) == STRICT_REJECT, "a record cut short", (long long)cut);
  expect(strict(good.substr(4) + std::string("X0i\1\0\0\0", 7)) == STRICT_KEEP, "X0 last, as int32");
  expect(strict(std::string("X0Z1\0", 5) + good.substr(4)) == STRICT_PANICS, "X0 a string");
  expect(strict(std::string("X0C\2", 4) + std::string("X1Z0\0", 5) + good.substr(8)) == STRICT_REJECT, "X0 wrong in front of X1 a string");
  expect(strict(std::string("XGZ0\0", 5) + good.substr(0, 16)) == STRICT_PANICS, "XG a string, first field");
  const std::string barr = std::string("BBBS\3\0\0\0\1\0\2\0\3\0", 14), z = std::string("ZZZX0X1\0", 8);
  expect(strict(z + good.substr(0, 8) + barr + good.substr(8)) == STRICT_KEEP, "Z and B between");
  for (size_t cut = 1; cut < barr.size(); cut++) expect(strict(good.substr(0, 16) + barr, cut) == STRICT_REJECT, "a B field cut short", (long long)cut);
  expect(strict(good.substr(0, 16) + std::string("BBBS\xff\xff\xff\xff", 8)) == STRICT_REJECT, "a B count that overflows the record");
  expect(strict(good.substr(0, 16) + std::string("ZZZabc", 6)) == STRICT_REJECT, "a Z field without its NUL");
  expect(strict(good + std::string("ZZZabc", 6)) == STRICT_KEEP, "an unterminated field behind all five");
  expect(tag_int_value('c', (const uint8_t *)"\x80") == -128 && tag_int_value('s', (const uint8_t *)"\0\x80") == -32768 &&
             tag_int_value('i', (const uint8_t *)"\0\0\0\x80") == -2147483648ll && tag_int_value('I', (const uint8_t *)"\xff\xff\xff\xff") == 4294967295ll,
         "integer values at the types' ends");
}

// every part of a layout written in a block of exactly L.bytes
static void layouts() {
  for (int32_t n_ref = 0; n_ref <= 5; n_ref++) {
    for (size_t total : {0u, 1u, 2u, 1000u}) {
      const RegionLayout L(total, n_ref);
      std::unique_ptr<uint8_t[]> blk(new uint8_t[L.bytes]);
      memset(blk.get() + L.pool, 1, total * 8);
      memset(blk.get() + L.ptr, 2, (size_t)n_ref * 8);
      memset(blk.get() + L.cnt, 3, (size_t)n_ref * 8);
      bool ok = L.ptr % 8 == 0 && L.cnt % 8 == 0;
      for (size_t k = 0; k < total * 8; k++) ok = ok && blk[L.pool + k] == 1;
      for (size_t k = 0; k < (size_t)n_ref * 8; k++) ok = ok && blk[L.ptr + k] == 2 && blk[L.cnt + k] == 3;
      expect(ok, "region layout", n_ref, (long long)total);
    }
    for (int32_t n_groups : {0, 1, 8000})
      for (uint64_t n : {0ull, 1ull, 257ull}) {
        const ClassifyLayout L(n, n_ref, n_groups);
        std::unique_ptr<uint8_t[]> blk(new uint8_t[L.bytes]);
        memset(blk.get() + L.gof, 1, (size_t)n_ref * 4);
        memset(blk.get() + L.counts, 2, L.n_counts * 8);
        memset(blk.get() + L.split, 3, (size_t)n * 2);
        memset(blk.get() + L.spread, 4, (size_t)n);
        bool ok = L.counts % 8 == 0 && L.split % 2 == 0 && L.n_counts == (size_t)n_groups + 2;
        for (size_t k = 0; k < (size_t)n_ref * 4; k++) ok = ok && blk[L.gof + k] == 1;
        for (size_t k = 0; k < L.n_counts * 8; k++) ok = ok && blk[L.counts + k] == 2;
        for (size_t k = 0; k < (size_t)n * 2; k++) ok = ok && blk[L.split + k] == 3;
        for (size_t k = 0; k < (size_t)n; k++) ok = ok && blk[L.spread + k] == 4;
        expect(ok, "classify layout", n_ref, n_groups);
      }
    const DictionaryLayout D(n_ref);
    std::unique_ptr<uint8_t[]> blk(new uint8_t[D.bytes]);
    memset(blk.get() + D.counters, 1, 16);
    memset(blk.get() + D.map, 2, (size_t)n_ref * 4);
    expect(blk[D.counters + 15] == 1 && (n_ref == 0 || blk[D.map] == 2) && D.counters % 8 == 0 && D.map % 4 == 0, "dictionary layout", n_ref);
  }
  expect(clear_flag_grid(0, 256) == 1 && clear_flag_grid(~0ull >> 32, 304) == 2432 && DictionaryLayout::grid(1, 0) == 1 && ClassifyLayout::grid(1) == 1 &&
             ClassifyLayout::grid(~0ull >> 32) == 2048, "grids");
}

static void routes() {
  int32_t g = -5;
  expect(!split_route(-1, -1, nullptr, 0, &g) && g == 0, "no contigs");
  expect(split_route(3, -1, nullptr, 0, &g) == false && g == 0, "a refid the header does not hold, no table");
  std::unique_ptr<int32_t[]> gof(new int32_t[2]{1, 2});
  expect(split_route(0, 1, gof.get(), 2, &g) && g == 1 && !split_route(1, 1, gof.get(), 2, &g) && g == 2 && split_route(1, 2, gof.get(), 2, &g), "two contigs");
  expect(merge_upper_bound(nullptr, 0, 5) == 0, "no group keys");
  std::unique_ptr<uint64_t[]> kg(new uint64_t[3]{merge_key(0, 5), merge_key(0, 5), merge_key(-1, 0)});
  expect(merge_upper_bound(kg.get(), 3, merge_key(0, 4)) == 0 && merge_upper_bound(kg.get(), 3, merge_key(0, 5)) == 2 &&
             merge_upper_bound(kg.get(), 3, merge_key(-1, 0)) == 3 && merge_upper_bound(kg.get(), 3, merge_key(-1, -1)) == 3, "upper bound");
  std::unique_ptr<int32_t[]> iv(new int32_t[4]{100, 200, 300, 400});
  expect(!overlap(nullptr, 0, 1, 1000) && overlap(iv.get(), 2, 200, 200) && !overlap(iv.get(), 2, 201, 300) && overlap(iv.get(), 2, 201, 301), "overlap");
}

int main() {
  cigars();
  strict_rule();
  layouts();
  routes();
  if (failures) return 1;
  printf("filter_rules_asan: ok\n");
  return 0;
}
