// sw_plan_asan.cpp - a stand-alone program (own main, no Python) that walks elprep_amd/csrc/sw_plan.hpp over heap buffers of exactly the
// planned sizes, built with -fsanitize=address,undefined by tests/test_sw_plan_cpu.py: the checks over offset arrays of exact length, the
// chunks' regions written in full where the kernels write them (every backtrack cell through sw_bt_index, the raw operations and their
// count word, the tile edge), the per-problem arrays and the input layout.  A region that overlaps its neighbour shows as a wrong
// tag below, one that leaves its buffer as a sanitizer report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "../elprep_amd/csrc/sw_plan.hpp"

using namespace elp;

static int fail(const char *what, unsigned long long a = 0, unsigned long long b = 0) {
  printf("sw_plan_asan: FAILED %s (%llu, %llu)\n", what, a, b);
  return 1;
}

static int walk(const std::vector<uint32_t> &lens_ref, const std::vector<uint32_t> &lens_alt, uint64_t budget) {
  const uint64_t n = lens_ref.size();
  // pools of exactly the lengths' sum, offsets of exactly n + 1
  std::unique_ptr<uint64_t[]> a_off(new uint64_t[n + 1]), b_off(new uint64_t[n + 1]);
  std::unique_ptr<uint32_t[]> ref_of(new uint32_t[n]), alt_of(new uint32_t[n]), len_ref(new uint32_t[n]), len_alt(new uint32_t[n]);
  a_off[0] = b_off[0] = 0;
  for (uint64_t k = 0; k < n; k++) {
    a_off[k + 1] = a_off[k] + lens_ref[k];
    b_off[k + 1] = b_off[k] + lens_alt[n - 1 - k];  // (the alternates in reverse order: alt_of is not the identity)
    ref_of[k] = (uint32_t)k;
    alt_of[k] = (uint32_t)(n - 1 - k);
  }
  const SwCheck r = sw_check_batch(n, a_off.get(), n, b_off.get(), n, ref_of.get(), alt_of.get(), len_ref.get(), len_alt.get());
  if (r.code) return fail("a valid batch was refused");
  uint64_t bound = 0;
  for (uint64_t k = 0; k < n; k++) {
    if (len_ref[k] != lens_ref[k] || len_alt[k] != lens_alt[k]) return fail("lengths", k);
    bound += lens_ref[k] + lens_alt[k] + 2;
  }
  if (r.ops_bound != bound) return fail("ops_bound", r.ops_bound, bound);

  std::vector<SwProb> probs(n);
  for (uint64_t k = 0; k < n; k++) probs[k] = SwProb{(uint32_t)k, 0, 0, 0, 0};
  const std::vector<SwChunkCut> cuts = sw_chunks(probs, len_ref.get(), len_alt.get(), budget);
  uint64_t next = 0;
  for (const SwChunkCut &cut : cuts) {
    if (cut.first != next || cut.end <= cut.first) return fail("chunks are not consecutive", cut.first, next);
    next = cut.end;
    const SwChunk ch(cut);
    if (cut.end - cut.first > 1 && ch.bytes > budget) return fail("a chunk of several problems exceeds the budget", ch.bytes, budget);
    if (ch.bt_at % 8 || ch.raw_at % 8 || ch.edge_at % 8) return fail("a chunk array is not 8-byte aligned");
    std::unique_ptr<uint8_t[]> buf(new uint8_t[ch.bytes ? ch.bytes : 1]);
    memset(buf.get(), 0xFF, ch.bytes);
    int16_t *bt = reinterpret_cast<int16_t *>(buf.get() + ch.bt_at);
    uint32_t *raw = reinterpret_cast<uint32_t *>(buf.get() + ch.raw_at);
    int32_t *edge = reinterpret_cast<int32_t *>(buf.get() + ch.edge_at);
    for (uint64_t i = cut.first; i < cut.end; i++) {  // every problem tags what it owns ...
      const uint32_t m = len_ref[i], q = len_alt[i], tag = (uint32_t)(i - cut.first) & 0x3FFF;
      if (probs[i].bt_at % SW_COLS) return fail("a backtrack region is not aligned for the strips' 8-byte stores", i);
      for (uint32_t row = 1; row <= m; row++)
        for (uint32_t col = 1; col <= q; col++) {
          int16_t &cell = bt[probs[i].bt_at + sw_bt_index(m, q, row, col)];
          if (cell != -1) return fail("two cells share a place", i, row);
          cell = (int16_t)tag;
        }
      for (uint32_t w = 0; w <= m + q + 3; w++) {  // m + q + 3 operations and the count word
        if (raw[probs[i].raw_at + w] != 0xFFFFFFFFu) return fail("raw regions overlap", i, w);
        raw[probs[i].raw_at + w] = tag;
      }
      if (q > SW_TILE)
        for (uint32_t w = 0; w < 3 * m; w++) {
          if (edge[probs[i].edge_at + w] != -1) return fail("edge regions overlap", i, w);
          edge[probs[i].edge_at + w] = (int32_t)tag;
        }
    }
    for (uint64_t i = cut.first; i < cut.end; i++) {  // ... and finds it untouched by the others
      const uint32_t m = len_ref[i], q = len_alt[i], tag = (uint32_t)(i - cut.first) & 0x3FFF;
      for (uint32_t row = 1; row <= m; row++)
        for (uint32_t col = 1; col <= q; col++)
          if (bt[probs[i].bt_at + sw_bt_index(m, q, row, col)] != (int16_t)tag) return fail("a backtrack cell was overwritten", i, row);
      for (uint32_t w = 0; w <= m + q + 3; w++)
        if (raw[probs[i].raw_at + w] != tag) return fail("a raw word was overwritten", i, w);
    }
  }
  if (next != n) return fail("problems left out", next, n);

  // the per-problem arrays and the inputs, each array written in full inside a buffer of exactly `bytes`
  const SwPerProblem lay(n, n);
  std::unique_ptr<uint8_t[]> w1(new uint8_t[lay.bytes]);
  memset(w1.get() + lay.miss, 1, 4 * n);
  memset(w1.get() + lay.n_ops, 2, 4 * (n + 1));
  memset(w1.get() + lay.scan, 3, 4 * (n + 1));
  memset(w1.get() + lay.offset, 4, 4 * n);
  memset(w1.get() + lay.cigar_off, 5, 8 * (n + 1));
  memset(w1.get() + lay.probs, 6, sizeof(SwProb) * n);
  const uint64_t starts[7] = {lay.miss, lay.n_ops, lay.scan, lay.offset, lay.cigar_off, lay.probs, lay.bytes};
  const uint64_t sizes[6] = {4 * n, 4 * (n + 1), 4 * (n + 1), 4 * n, 8 * (n + 1), sizeof(SwProb) * n};
  for (int i = 0; i < 6; i++) {
    if (starts[i] % 8 || starts[i] + sizes[i] > starts[i + 1]) return fail("per-problem arrays overlap", (unsigned long long)i);
    for (uint64_t x = 0; x < sizes[i]; x++)
      if (w1[starts[i] + x] != i + 1) return fail("a per-problem array was overwritten", (unsigned long long)i);
  }
  const SwInputs in(a_off[n], n, n);
  std::unique_ptr<uint8_t[]> w0(new uint8_t[in.bytes]);
  memset(w0.get() + in.seq, 1, a_off[n]);
  memset(w0.get() + in.off, 2, 8 * (n + 1));
  memset(w0.get() + in.idx0, 3, 4 * n);
  memset(w0.get() + in.idx1, 4, 4 * n);
  memset(w0.get() + in.idx2, 5, 4 * n);
  if (in.off < a_off[n] || in.idx0 < in.off + 8 * (n + 1) || in.idx1 < in.idx0 + 4 * n || in.idx2 < in.idx1 + 4 * n || in.bytes < in.idx2 + 4 * n) return fail("inputs overlap");
  return 0;
}

int main() {
  // lengths around the layouts' parities (1 .. 9), a strip's end, a tile's end and one column into the second and third tile
  std::vector<uint32_t> m, q;
  for (uint32_t a = 1; a <= 9; a++)
    for (uint32_t b : {1u, 2u, 3u, 4u, 5u, 6u, 7u, 8u, 9u, 255u, 256u, 257u, 258u, 513u}) { m.push_back(a); q.push_back(b); }
  for (uint32_t a : {63u, 64u, 65u, 130u}) { m.push_back(a); q.push_back(a + 200); }
  for (const uint64_t budget : {1ull, 5000ull, 60000ull, 1ull << 30})
    if (walk(m, q, budget)) return 1;
  // refusals over arrays of exact length
  std::unique_ptr<uint64_t[]> off(new uint64_t[3]{0, 0, 4096});
  std::unique_ptr<uint32_t[]> idx(new uint32_t[1]{0}), l1(new uint32_t[1]), l2(new uint32_t[1]);
  if (sw_check_batch(2, off.get(), 2, off.get(), 1, idx.get(), idx.get(), l1.get(), l2.get()).code != SW_REFUSE_ARG) return fail("an empty sequence passed");
  idx[0] = 1;
  if (sw_check_batch(2, off.get(), 2, off.get(), 1, idx.get(), idx.get(), l1.get(), l2.get()).code != SW_REFUSE_UNSUPPORTED) return fail("4096 bytes passed");
  idx[0] = 2;
  if (sw_check_batch(2, off.get(), 2, off.get(), 1, idx.get(), idx.get(), l1.get(), l2.get()).code != SW_REFUSE_ARG) return fail("an index outside the pool passed");
  printf("sw_plan_asan: ok\n");
  return 0;
}
