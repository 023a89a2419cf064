// split_merge.hip — the `elprep split` / `elprep merge` bookkeeping, done in HBM.
//
// `elprep split`: SplitFilePerChromosome's routing rule (sam/split-merge.go:280-293) per record — split of RNAME and the "spread" test —
// and the per-split record counts, so that a host can partition a staged file across GPUs without touching the payload on the CPU
// (elp_split_classify).
// `elprep merge`: MergeSortedFilesSplitPerChromosome (sam/split-merge.go:410-576) as a rank computation: where every record of the
// coordinate-sorted spread split goes among the concatenated, coordinate-sorted group splits (behind all group reads of its position;
// merge_spread_slots, elp_merge_spread).
// The rules (split_route, merge_key, merge_upper_bound) and the layout of scratch slot 5 are filter_rules.hpp's.
#include "common.hpp"
#include "filter_rules.hpp"

namespace elp {

// ---- split: routing rule of SplitFilePerChromosome
__global__ __launch_bounds__(256) void k_split_classify(uint64_t n, const int32_t *__restrict__ refid, const int32_t *__restrict__ next_refid,
                                                        const int32_t *__restrict__ group_of_ref, int32_t n_ref, int32_t n_groups,
                                                        uint16_t *__restrict__ split_out, uint8_t *__restrict__ spread_out,
                                                        unsigned long long *__restrict__ counts /* [n_groups + 2]: unmapped, groups, spread */,
                                                        uint16_t *__restrict__ split_col /* the context's split-id column */) {
  extern __shared__ unsigned int lds_cnt[];
  for (int k = threadIdx.x; k < n_groups + 2; k += blockDim.x) lds_cnt[k] = 0;
  __syncthreads();
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    int32_t g;
    const bool spread = split_route(refid[i], next_refid[i], group_of_ref, n_ref, &g);  // (the rule the split emitters share)
    split_out[i] = (uint16_t)g;
    split_col[i] = (uint16_t)g;  // the record's split file: travels with it (elp_copy_records / elp_exchange_records keep it)
    spread_out[i] = spread ? 1 : 0;
    atomicAdd(&lds_cnt[g], 1u);
    if (spread) atomicAdd(&lds_cnt[n_groups + 1], 1u);
  }
  __syncthreads();
  for (int k = threadIdx.x; k < n_groups + 2; k += blockDim.x)
    if (lds_cnt[k]) atomicAdd(&counts[k], (unsigned long long)lds_cnt[k]);
}

// ---- merge: spread read j (key ks[j]) goes behind every group read with key <= ks[j]
__global__ __launch_bounds__(256) void k_merge_rank(uint64_t ng, const uint64_t *__restrict__ kg, uint64_t ns, const uint64_t *__restrict__ ks,
                                                    uint64_t *__restrict__ slot_of_spread) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= ns) return;
  slot_of_spread[j] = merge_upper_bound(kg, ng, ks[j]) + j;  // spread reads keep their own order
}
__global__ __launch_bounds__(256) void k_perm_keys(uint64_t n_out, const uint32_t *__restrict__ perm, const int32_t *__restrict__ refid,
                                                   const int32_t *__restrict__ pos, uint64_t *__restrict__ keys) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_out) return;
  const uint32_t i = perm[k];
  keys[k] = merge_key(refid[i], pos[i]);
}

// The merge of queryname-sorted contexts: the reference panics with "Merging of files sorted by queryname not yet implemented."
// (cmd/merge.go:175-176)
int merge_refuses_queryname(elp_ctx *groups, const char *who) {
  return set_error(groups, ELP_ERR_UNSUPPORTED, "%s: a context holds a queryname permutation (elp_sort_queryname); merging queryname-sorted "
                   "files is not implemented (cmd/merge.go:175-176)", who);
}

// keys[0 .. n_out) of a keep-ordered context must be non-decreasing for the merge's binary search: (refid, POS) ascending, refid -1 (the
// high word 0xFFFFFFFF) last - what a file with SO:coordinate in its header holds.  *bad |= 1 if entry k is smaller than entry k - 1.
// MERGE_CHECK_W entries per workgroup; the first entry of a workgroup looks at the last of the one in front.
constexpr uint32_t MERGE_CHECK_W = 256;
__global__ __launch_bounds__(MERGE_CHECK_W) void k_merge_check_order(uint64_t n_out, const uint64_t *__restrict__ keys, uint32_t *__restrict__ bad) {
  const uint64_t k = (uint64_t)blockIdx.x * MERGE_CHECK_W + threadIdx.x;
  const bool inv = k > 0 && k < n_out && keys[k] < keys[k - 1];
  if (__ballot(inv) && (threadIdx.x & 63u) == 0) atomicOr(bad, 1u);
}

// The same check for ONE context that holds a plain keep permutation (the index of its stream, bai.hip): its n_out output records' keys
// into `keys` (n_out entries of the caller's scratch), *in_order = none of them is smaller than the one in front.  Waits for the stream.
int keep_coordinate_order(elp_ctx *c, uint64_t n_out, uint64_t *keys, uint32_t *bad_dev, bool *in_order) {
  *in_order = true;
  if (n_out < 2) return 0;
  ELP_HIP(c, hipMemsetAsync(bad_dev, 0, 4, c->stream));
  ELP_LAUNCH(c, "merge_keys", k_perm_keys, dim3(blocks_for(n_out, 256)), dim3(256), 0, n_out, (const uint32_t *)c->perm.p, (const int32_t *)c->refid.p,
             (const int32_t *)c->pos.p, keys);
  ELP_LAUNCH(c, "merge_check_order", k_merge_check_order, dim3(blocks_for(n_out, MERGE_CHECK_W)), dim3(MERGE_CHECK_W), 0, n_out, (const uint64_t *)keys, bad_dev);
  uint32_t h_bad = 0;
  ELP_HIP(c, hipMemcpyAsync(&h_bad, bad_dev, 4, hipMemcpyDeviceToHost, c->stream));
  ELP_HIP(c, elp::stream_wait(c->stream));
  *in_order = h_bad == 0;
  return 0;
}

// MergeSortedFilesSplitPerChromosome's order as ranks, on the device: slots[j] = output slot of the j-th record of `spread`'s output
// among `groups`' output (scratch slot 5 of `groups`; valid until that slot is reused).  Queued on groups->stream.
// Either context holds a coordinate permutation or a plain keep permutation (elp_order_keep, by_split = 0): by choosing this call for
// keep-ordered contexts the host vouches for SO:coordinate, as cmd/merge.go:157-174 chooses by header.HDSO() - a context that received
// its records in file order (contigs in refid order, `*` last) then holds them in the merge's order.  The keys of a keep-ordered side
// are checked (one pass, one word read back): an inversion is ELP_ERR_DATA, where the reference would write some order of its own.
int merge_spread_slots(elp_ctx *groups, elp_ctx *spread, uint64_t **slots_out) {
  if (groups->derived.sorted_qname || spread->derived.sorted_qname) return merge_refuses_queryname(groups, "elp_merge_spread");
  if (!groups->derived.sorted || !spread->derived.sorted)
    return set_error(groups, ELP_ERR_ARG, "elp_merge_spread: both contexts must be coordinate-sorted (elp_sort_coordinate) or hold coordinate-sorted input in "
                     "input order (elp_order_keep with by_split = 0)");
  if (groups->derived.sorted_keep_by_split || spread->derived.sorted_keep_by_split)
    return set_error(groups, ELP_ERR_ARG, "elp_merge_spread: a context holds a keep permutation ordered by split id (elp_order_keep with by_split != 0): "
                     "the coordinate merge takes plain input order only");
  if (groups->device != spread->device) return set_error(groups, ELP_ERR_ARG, "elp_merge_spread: contexts on different devices");
  ELP_HIP(groups, hipSetDevice(groups->device));
  // (a sort defers the read of its radix passes' look-back timeout bit: nothing is merged from a permutation that was flagged wrong)
  ELP_TRY(radix_check(groups));
  if (radix_check(spread) != 0) return set_error(groups, ELP_ERR_HIP, "elp_merge_spread: the spread context's sort failed: %s", spread->err.c_str());
  // the mapped part of the groups' output (the unmapped split is appended behind the merge, :560-576)
  const uint64_t ns = spread->n - spread->n_sr;
  uint64_t *kg, *ks, *slots;
  ELP_TRY(scratch(groups, 5, (groups->n + 8) + 2 * (ns + 8) + 2, &kg));
  ks = kg + groups->n + 8;
  slots = ks + ns + 8;
  uint32_t *bad = reinterpret_cast<uint32_t *>(slots + ns + 8);
  const uint64_t ng_all = groups->n - groups->n_sr;
  const bool check_g = groups->derived.sorted_keep && ng_all > 1, check_s = spread->derived.sorted_keep && ns > 1;
  ELP_HIP(groups, elp::stream_wait(spread->stream));
  if (check_g || check_s) ELP_HIP(groups, hipMemsetAsync(bad, 0, 4, groups->stream));
  if (ng_all)
    ELP_LAUNCH(groups, "merge_keys", k_perm_keys, dim3(blocks_for(ng_all, 256)), dim3(256), 0, ng_all, (const uint32_t *)groups->perm.p,
               (const int32_t *)groups->refid.p, (const int32_t *)groups->pos.p, kg);
  if (ns)
    ELP_LAUNCH(groups, "merge_keys", k_perm_keys, dim3(blocks_for(ns, 256)), dim3(256), 0, ns, (const uint32_t *)spread->perm.p,
               (const int32_t *)spread->refid.p, (const int32_t *)spread->pos.p, ks);
  if (check_g)
    ELP_LAUNCH(groups, "merge_check_order", k_merge_check_order, dim3(blocks_for(ng_all, MERGE_CHECK_W)), dim3(MERGE_CHECK_W), 0, ng_all, (const uint64_t *)kg, bad);
  if (check_s)
    ELP_LAUNCH(groups, "merge_check_order", k_merge_check_order, dim3(blocks_for(ns, MERGE_CHECK_W)), dim3(MERGE_CHECK_W), 0, ns, (const uint64_t *)ks, bad);
  if (check_g || check_s) {
    uint32_t h_bad = 0;
    ELP_HIP(groups, hipMemcpyAsync(&h_bad, bad, 4, hipMemcpyDeviceToHost, groups->stream));
    ELP_HIP(groups, elp::stream_wait(groups->stream));
    if (h_bad)
      return set_error(groups, ELP_ERR_DATA, "elp_merge_spread: records are not in coordinate order ((refid, POS) must not decrease in a context that holds "
                       "its input order, elp_order_keep; sort it with elp_sort_coordinate instead)");
  }
  // unmapped reads (refid -1 -> 0xFFFFFFFF........) sort behind every contig: the search covers them without a special case
  if (ns) ELP_LAUNCH(groups, "merge_rank", k_merge_rank, dim3(blocks_for(ns, 256)), dim3(256), 0, ng_all, (const uint64_t *)kg, ns, (const uint64_t *)ks, slots);
  *slots_out = slots;
  return 0;
}

}  // namespace elp

using namespace elp;

extern "C" {

int elp_split_classify(elp_ctx *c, const int32_t *group_of_ref, int32_t n_groups, uint16_t *split_out, uint8_t *spread_out, uint64_t *counts_out) {
  if (!c || !group_of_ref || n_groups < 0 || n_groups > 8000) return set_error(c, ELP_ERR_ARG, "elp_split_classify: bad arguments");
  ELP_HIP(c, hipSetDevice(c->device));
  const uint64_t n = c->n;
  const ClassifyLayout L(n, c->n_ref, n_groups);
  const size_t nc = L.n_counts;
  uint8_t *blk;
  ELP_TRY(scratch(c, 5, L.bytes, &blk));
  int32_t *d_gof = reinterpret_cast<int32_t *>(blk + L.gof);
  unsigned long long *d_cnt = reinterpret_cast<unsigned long long *>(blk + L.counts);
  uint16_t *d_split = reinterpret_cast<uint16_t *>(blk + L.split);
  uint8_t *d_spread = blk + L.spread;
  if (c->n_ref) ELP_HIP(c, hipMemcpyAsync(d_gof, group_of_ref, (size_t)c->n_ref * 4, hipMemcpyHostToDevice, c->stream));
  ELP_HIP(c, hipMemsetAsync(d_cnt, 0, nc * 8, c->stream));
  if (n) {
    ELP_LAUNCH(c, "split_classify", k_split_classify, dim3(ClassifyLayout::grid(n)), dim3(256), nc * sizeof(unsigned int), n, (const int32_t *)c->refid.p,
               (const int32_t *)c->next_refid.p, (const int32_t *)d_gof, c->n_ref, n_groups, d_split, d_spread, d_cnt, c->split.p);
    // the split ids are part of every duplicate-marking key; records with equal keys share their contig, hence their split: no result changes
    c->max_split = std::max<uint32_t>(c->max_split, (uint32_t)n_groups);
    c->derived.split_changed();
    if (split_out) ELP_HIP(c, hipMemcpyAsync(split_out, d_split, n * 2, hipMemcpyDeviceToHost, c->stream));
    if (spread_out) ELP_HIP(c, hipMemcpyAsync(spread_out, d_spread, n, hipMemcpyDeviceToHost, c->stream));
  }
  std::vector<unsigned long long> h(nc);
  ELP_HIP(c, hipMemcpyAsync(h.data(), d_cnt, nc * 8, hipMemcpyDeviceToHost, c->stream));
  ELP_HIP(c, elp::stream_wait(c->stream));
  if (counts_out)
    for (size_t k = 0; k < nc; k++) counts_out[k] = h[k];
  return 0;
}

int elp_merge_spread(elp_ctx *groups, elp_ctx *spread, uint64_t *slot_of_spread_out) {
  if (!groups || !spread || groups == spread) return ELP_ERR_ARG;
  uint64_t *slots = nullptr;
  ELP_TRY(merge_spread_slots(groups, spread, &slots));
  const uint64_t ns = spread->n - spread->n_sr;
  if (ns) ELP_HIP(groups, hipMemcpyAsync(slot_of_spread_out, slots, ns * 8, hipMemcpyDeviceToHost, groups->stream));
  ELP_HIP(groups, elp::stream_wait(groups->stream));
  return 0;
}

}  // extern "C"
