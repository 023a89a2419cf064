// apply_plan_asan.cpp — the two scratch layouts of elprep_amd/csrc/apply_plan.hpp on their own under the sanitizers (built and run by
// tests/test_apply_plan_cpu.py with -fsanitize=address,undefined): for a grid of shapes a heap block of exactly the size the layout asks
// for, every byte of every region written through the layout's offsets with the region's tag, then every tag read back - a region that
// ends behind the block is the sanitizer's finding, two regions that overlap this program's.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../elprep_amd/csrc/apply_plan.hpp"

using namespace elp;

struct Region { size_t at, bytes; };

static int fill_and_check(size_t block_bytes, const std::vector<Region> &regions, const char *what) {
  uint8_t *block = static_cast<uint8_t *>(malloc(block_bytes ? block_bytes : 1));
  if (!block) { printf("%s: no memory for %zu bytes\n", what, block_bytes); return 1; }
  for (size_t r = 0; r < regions.size(); r++) memset(block + regions[r].at, (int)(r + 1), regions[r].bytes);
  int bad = 0;
  for (size_t r = 0; r < regions.size() && !bad; r++)
    for (size_t k = 0; k < regions[r].bytes; k++)
      if (block[regions[r].at + k] != (uint8_t)(r + 1)) { printf("%s: region %zu overwritten at byte %zu\n", what, r, k); bad = 1; break; }
  free(block);
  return bad;
}

static int dict_case(int n_cov, int n_qi, int lmax) {
  const LutDictLayout L(n_cov, n_qi, lmax);
  char what[96];
  snprintf(what, sizeof what, "LutDictLayout(%d, %d, %d)", n_cov, n_qi, lmax);
  return fill_and_check(L.words * 4, {{L.counter * 4, 256 * 4}, {L.slots * 4, (size_t)L.n_slots * 4}, {L.slot_id * 4, (size_t)L.n_slots * 4},
                                      {L.row_slot * 4, L.n_rows * 4}, {L.t1 * 4, L.n1 * 2}, {L.t2 * 4, L.t2_bytes}}, what);
}

static int slot5_case(uint64_t n, uint32_t len, bool split) {
  const Apply3Launch P(n, len, 256, 18080, split, 0, 512, 2304);
  char what[96];
  snprintf(what, sizeof what, "Apply3Launch(n %llu, len %u, split %d)", (unsigned long long)n, len, (int)split);
  std::vector<Region> regions = {{P.recs, (size_t)n * 8}, {P.dump, (size_t)P.grid * A3_NT * 16}};
  if (split) {
    regions.push_back({P.ridx, (size_t)n * 4});
    regions.push_back({P.cw, (3 * A3_MAXCOV + 1) * 4});
    regions.push_back({P.blk, (size_t)A3_RBLOCKS * A3_MAXCOV * 4});
  }
  return fill_and_check(P.size8 * 8, regions, what);
}

int main() {
  int bad = 0, cases = 0;
  const int covs[] = {1, 4, 16, 255}, nqis[] = {0, 1, 36, 88}, lmaxs[] = {1, 16, 150, 1023};
  for (int n_cov : covs)
    for (int n_qi : nqis)
      for (int lmax : lmaxs) {
        if ((size_t)n_cov * (size_t)n_qi * (size_t)(2 * lmax + 1) >= LUT_MAX_ROWS) continue;  // (no dictionary is built over that many rows)
        bad |= dict_case(n_cov, n_qi, lmax);
        cases++;
      }
  bad |= dict_case(89, 69, 341);  // 89 * 69 * 683 = 2^22 - 1 rows: the largest shape under the row cap
  cases++;
  const uint64_t ns[] = {0, 1, 1000, 1001, 100003};
  const uint32_t lens[] = {16, 33, 150, 160};
  for (uint64_t n : ns)
    for (uint32_t len : lens)
      for (int split = 0; split < 2; split++) {
        bad |= slot5_case(n, len, split != 0);
        cases++;
      }
  if (bad) return 1;
  printf("apply_plan_asan: ok (%d cases)\n", cases);
  return 0;
}
