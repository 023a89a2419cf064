// keep.hip — the permutation of a run that does not sort: `--sorting-order keep` (the default, cmd/filter.go:451), `unknown` and `unsorted`,
// and a requested `coordinate` on an input whose header already says SO:coordinate (effectiveSortingOrder, sam/filter-pipeline.go:208-225).
// Sam.AddNodes collects the alignments with StrictOrd(Slice) - input order - for Keep / Unknown (:110-112) and with Seq(Slice), of which
// input order is one legal result, for Unsorted (:123-124); RemoveOptionalReads and the filters1 predicates have taken their records out
// before the slice is made.
//
// Order: the records that are output (state 0 in the has_sr column) in staging order, then the records that are not (sr-tagged copies,
// rejected records) in staging order.  With by_split both parts are ordered by split id first: a context that holds several `elprep split`
// files delivers them file after file (MergeUnsortedFilesSplitPerChromosome, sam/split-merge.go:581-619, reads them one after the other).
//
// by_split == 0 is a stable two-class partition in two passes over the state column (about 6 B per record: the state byte twice, the
// permutation once):
//   (1) k_keep_count: the number of state-0 records of every tile of KEEP_W records; exclusive_scan_u32 over the tiles' counts;
//   (2) k_keep_scatter: a record's rank among the state-0 records of its tile from wavefront ballots (__ballot + mbcnt) and the waves'
//       counts in LDS; a record that is not output goes to n_out + (its index - the state-0 records in front of it).
// No tile waits for another one: the tiles' bases come from the scan between the two launches.
// by_split != 0 runs only in the merge of unsorted splits: the key (state != 0) << b | split, b = bit width of the largest split id, through
// the stable radix pair sort (radix.hip) with identity values, ceil((b + 1) / 8) passes.
#include "common.hpp"

namespace elp {

constexpr uint32_t KEEP_THREADS = 256;
constexpr uint32_t KEEP_ROUNDS = 2;                      // records per thread
constexpr uint32_t KEEP_W = 512;                         // records per workgroup of the two partition kernels (KEEP_THREADS * KEEP_ROUNDS)
constexpr uint32_t KEEP_WAVES = KEEP_THREADS / WAVE;
static_assert(KEEP_W == KEEP_THREADS * KEEP_ROUNDS, "a tile is KEEP_ROUNDS sweeps of the workgroup");

// lanes of the wave below this one
__device__ __forceinline__ uint32_t lanes_below(unsigned long long mask) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// counts[b] = state-0 records among records [b * KEEP_W, (b + 1) * KEEP_W)
__global__ __launch_bounds__(KEEP_THREADS) void k_keep_count(uint64_t n, const uint8_t *__restrict__ state, uint32_t *__restrict__ counts) {
  __shared__ uint32_t s_cnt[KEEP_WAVES];
  const uint64_t base = (uint64_t)blockIdx.x * KEEP_W;
  uint32_t mine = 0;  // (wave-uniform)
#pragma unroll
  for (uint32_t j = 0; j < KEEP_ROUNDS; j++) {
    const uint64_t i = base + j * KEEP_THREADS + threadIdx.x;
    const bool out = i < n && state[i] == 0;
    mine += (uint32_t)__popcll(__ballot(out));
  }
  if ((threadIdx.x & 63u) == 0) s_cnt[threadIdx.x >> 6] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0;
#pragma unroll
    for (uint32_t w = 0; w < KEEP_WAVES; w++) t += s_cnt[w];
    counts[blockIdx.x] = t;
  }
}

// perm[tile_base[b] + rank among the tile's state-0 records] = i for a state-0 record i; perm[n_out + i - (state-0 records in front of i)] = i
// for any other.  Within a tile the records are visited round by round, wave by wave, lane by lane - which is ascending i.
__global__ __launch_bounds__(KEEP_THREADS) void k_keep_scatter(uint64_t n, uint64_t n_out, const uint8_t *__restrict__ state,
                                                               const uint32_t *__restrict__ tile_base, uint32_t *__restrict__ perm) {
  __shared__ uint32_t s_cnt[KEEP_ROUNDS * KEEP_WAVES];
  const uint64_t base = (uint64_t)blockIdx.x * KEEP_W;
  const uint32_t w = threadIdx.x >> 6;
  bool out[KEEP_ROUNDS];
  uint32_t below[KEEP_ROUNDS];
#pragma unroll
  for (uint32_t j = 0; j < KEEP_ROUNDS; j++) {
    const uint64_t i = base + j * KEEP_THREADS + threadIdx.x;
    out[j] = i < n && state[i] == 0;
    const unsigned long long b = __ballot(out[j]);
    below[j] = lanes_below(b);
    if ((threadIdx.x & 63u) == 0) s_cnt[j * KEEP_WAVES + w] = (uint32_t)__popcll(b);
  }
  __syncthreads();
  const uint64_t first = tile_base[blockIdx.x];  // state-0 records in front of the tile
#pragma unroll
  for (uint32_t j = 0; j < KEEP_ROUNDS; j++) {
    const uint64_t i = base + j * KEEP_THREADS + threadIdx.x;
    if (i >= n) continue;
    uint32_t before = below[j];  // ... in front of record i inside the tile
    for (uint32_t k = 0; k < j * KEEP_WAVES + w; k++) before += s_cnt[k];
    const uint64_t zeros = first + before;
    const uint64_t at = out[j] ? zeros : n_out + (i - zeros);
    if (at < n) perm[at] = (uint32_t)i;  // (always, while n_out is the column's count of state-0 records)
  }
}

// keys[i] = (state != 0) << bits | split id
__global__ __launch_bounds__(256) void k_keep_split_keys(uint64_t n, const uint8_t *__restrict__ state, const uint16_t *__restrict__ split, int bits,
                                                         uint64_t *__restrict__ keys) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) keys[i] = ((uint64_t)(state[i] != 0) << bits) | (uint64_t)split[i];
}

// *first = the number of leading entries of perm[0 .. n_out) whose record has split id 0 (perm is ordered by split id: one thread's
// binary search, ~32 dependent loads)
__global__ void k_keep_split0_end(uint64_t n_out, const uint32_t *__restrict__ perm, const uint16_t *__restrict__ split, uint32_t *__restrict__ first) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  uint64_t lo = 0, hi = n_out;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (split[perm[mid]] == 0) lo = mid + 1; else hi = mid;
  }
  *first = (uint32_t)lo;
}

// MergeUnsortedFilesSplitPerChromosome's stream (sam/split-merge.go:581-619) as the source array of the emitters: ranks [0, g0) of the
// groups' output (the unmapped file), the ns records of the spread's output, ranks [g0, ng) of the groups' output (the group files)
__global__ __launch_bounds__(256) void k_keep_concat_src(uint64_t ng, uint64_t ns, const uint32_t *__restrict__ g0_dev, uint32_t *__restrict__ src) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= ng + ns) return;
  const uint64_t g0 = *g0_dev;
  src[k] = k < g0 ? (uint32_t)k : (k < g0 + ns ? MERGE_SECOND | (uint32_t)(k - g0) : (uint32_t)(k - ns));
}

// the keep permutation of c's records into c->perm, on c's stream (c: the side lane's shadow context, order_keep below)
static int keep_impl(elp_ctx *c, bool by_split) {
  const uint64_t n = c->n, n_out = n - c->n_sr;
  if (n == 0) return 0;
  if (n >= 0xFFFFFFF0ull) return set_error(c, ELP_ERR_UNSUPPORTED, "elp_order_keep: more than 2^32-16 records");
  const uint8_t *state = c->has_sr.p;
  if (!by_split) {
    // scratch slot 1: slot 0 of the sort lane holds the coordinate key passes made ahead (elp_sort_ahead), which stay valid
    const unsigned nb = blocks_for(n, KEEP_W);
    uint32_t *counts;
    ELP_TRY(scratch(c, 1, 2 * ((size_t)nb + 8), &counts));
    uint32_t *tile_base = counts + nb + 8;
    ELP_LAUNCH(c, "keep_count", k_keep_count, dim3(nb), dim3(KEEP_THREADS), 0, n, state, counts);
    ELP_TRY(exclusive_scan_u32(c, counts, tile_base, nb, nullptr));
    ELP_LAUNCH(c, "keep_scatter", k_keep_scatter, dim3(nb), dim3(KEEP_THREADS), 0, n, n_out, state, (const uint32_t *)tile_base, c->perm.p);
    return 0;
  }
  int bits = 1;
  while (bits < 16 && (c->max_split >> bits) != 0) bits++;
  uint64_t *kbuf;
  uint32_t *vbuf;
  ELP_TRY(scratch(c, 1, 2 * n + 8, &kbuf));
  ELP_TRY(scratch(c, 2, 2 * n + 8, &vbuf));
  ELP_LAUNCH(c, "keep_split_keys", k_keep_split_keys, dim3(blocks_for(n, 256)), dim3(256), 0, n, state, (const uint16_t *)c->split.p, bits, kbuf);
  uint64_t *ko;
  uint32_t *vo;
  ELP_TRY(radix_sort_pairs_low(c, kbuf, vbuf, kbuf + n, vbuf + n, n, (bits + 1 + 7) / 8, &ko, &vo, nullptr, true));
  c->radix_check_pending = true;  // (read by the caller: radix_check)
  ELP_HIP(c, hipMemcpyAsync(c->perm.p, vo, n * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
  return 0;
}

// On the context's side lane 1, as the sorts (sort.hip: sort_on_side, qsort.hip: sort_queryname): the shadow sees the state column, the
// split-id column and the permutation's buffer as views for the duration of the call.  Nothing of the adapt stage is read or made.
static int order_keep(elp_ctx *c, bool by_split) {
  ELP_TRY(ensure(c, c->perm, c->n + 1));
  elp_ctx *s = nullptr;
  ELP_TRY(side_lane(c, 1, &s));
  s->n = c->n; s->n_sr = c->n_sr; s->max_split = c->max_split;
  int rc;
  {
    LaneViews views(s, c, &elp_ctx::has_sr, &elp_ctx::split);
    views.view(s->perm, c->perm, true);
    rc = keep_impl(s, by_split && c->max_split != 0);
  }
  if (rc == 0) rc = radix_check(s);  // (the lane's own error words: a look-back timeout of the radix passes is read here)
  if (rc == 0 && elp::stream_wait(s->stream) != hipSuccess) rc = set_error(s, ELP_ERR_HIP, "elp_order_keep: the sort lane's stream failed");
  if (rc != 0) {
    (void)elp::stream_wait(s->stream);
    c->err = s->err;
    return rc;
  }
  ELP_TRY(side_join(c, 1));
  c->derived.set_sorted_keep(by_split);
  return 0;
}

// src[0 .. ng + ns) of elp_emit_concat_bam / _bgzf, queued on groups->stream; g0_dev: one word of the caller's scratch
int keep_concat_src(elp_ctx *groups, uint64_t ng, uint64_t ns, uint32_t *g0_dev, uint32_t *src) {
  ELP_LAUNCH(groups, "keep_split0_end", k_keep_split0_end, dim3(1), dim3(64), 0, ng, (const uint32_t *)groups->perm.p, (const uint16_t *)groups->split.p, g0_dev);
  ELP_LAUNCH(groups, "keep_concat_src", k_keep_concat_src, dim3(blocks_for(ng + ns, 256)), dim3(256), 0, ng, ns, (const uint32_t *)g0_dev, src);
  return 0;
}

}  // namespace elp

extern "C" int elp_order_keep(elp_ctx *c, int by_split) {
  if (!c) return ELP_ERR_ARG;
  ELP_HIP(c, hipSetDevice(c->device));
  c->derived.drop_sorted();
  return elp::order_keep(c, by_split != 0);
}
