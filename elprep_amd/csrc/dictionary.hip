// dictionary.hip — ReplaceReferenceSequenceDictionary (filters/simple-filters.go:32-60) + AddREFID under the new dictionary (:208-231): the
// filter keeps an alignment iff dictTable[aln.RNAME] (:58; "*" is in the table, :53); AddREFID then gives RNAME and RNEXT the index of their
// name in the new header.SQ, -1 for a name it does not hold (:215-227).  Here the names are indices already: map[r] = index of old contig
// r's name in the new dictionary, -1 = not in it (elp_host_dictionary_map).  `--replace-reference-sequences` is
// elp_replace_reference_dictionary: REFID / RNEXT through that map, records of a contig that left rejected.
#include "common.hpp"
#include "bqsr_common.hpp"  // REF_LDS: the map is held in LDS up to the bound on contigs the BQSR kernels keep there - one number for "a
                            // dictionary that fits LDS" in the library (tests/test_gpu_replace_dictionary.py steps over it)
#include "filter_rules.hpp"

namespace elp {

// One record per thread: 9 bytes read (two refids, the state), up to 9 written - a write that would change nothing is skipped, so an
// identity map writes nothing.  EVERY record's columns are renumbered, whatever its state: the columns must not mix two numberings (the
// sort's key of a rejected record does not read them, a later elp_copy_records does).  A refid the old dictionary does not hold (RNEXT of
// BAM bytes is not bounded at staging) names nothing: -1.
// MAP_LDS: the map of an old dictionary of <= REF_LDS contigs is read once per workgroup into LDS; a larger one (hg38 with alts: 3366
// contigs, 13 KB) is read from HBM and stays in L2.
template <bool MAP_LDS>
__global__ __launch_bounds__(256) void k_replace_dictionary(uint64_t n, int32_t *__restrict__ refid, int32_t *__restrict__ next_refid, uint8_t *__restrict__ state,
                                                            const int32_t *__restrict__ map, int32_t n_old,
                                                            unsigned long long *__restrict__ cnt /* [0] rejected, [1] rejected tagged copies */) {
  __shared__ int32_t s_map[MAP_LDS ? REF_LDS : 1];
  __shared__ unsigned int s_cnt[2];
  if (MAP_LDS)
    for (int k = threadIdx.x; k < n_old; k += blockDim.x) s_map[k] = map[k];
  if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  const int32_t *mp = MAP_LDS ? s_map : map;
  // a grid of a few workgroups per CU strides over the records: with a workgroup per 256 records, the one counter word in HBM took an
  // atomic from every workgroup that rejects anything (profiles/replace_dictionary_speed_16Mreads.txt: 16 M reads, a contig of 8 % of them
  // dropped, 1.98 ms in that form against 0.14 ms in this one; 0.05 - 0.08 ms in either form for maps without rejects)
  unsigned int n_drop = 0, n_tagged = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const int32_t r = refid[i], nr = next_refid[i];
    const uint8_t st = state[i];
    const int32_t r_new = (uint32_t)r < (uint32_t)n_old ? mp[r] : -1, nr_new = (uint32_t)nr < (uint32_t)n_old ? mp[nr] : -1;
    if (r_new != r) refid[i] = r_new;
    if (nr_new != nr) next_refid[i] = nr_new;
    if (r >= 0 && r_new < 0 && st != 2) {  // dictTable[aln.RNAME] is false (:58); a record an earlier filter rejected never got here
      if (st == 1) n_tagged++;  // (as k_filter_records: a rejected tagged copy was already counted among the records that leave the output)
      else n_drop++;
      state[i] = 2;
    }
  }
  for (int d = 32; d > 0; d >>= 1) {  // per wavefront, then one LDS atomic per wave and one HBM atomic per workgroup and count
    n_drop += __shfl_down(n_drop, d);
    n_tagged += __shfl_down(n_tagged, d);
  }
  if ((threadIdx.x & 63) == 0) {
    if (n_drop) atomicAdd(&s_cnt[0], n_drop);
    if (n_tagged) atomicAdd(&s_cnt[1], n_tagged);
  }
  __syncthreads();
  if (threadIdx.x < 2 && s_cnt[threadIdx.x]) atomicAdd(cnt + threadIdx.x, (unsigned long long)s_cnt[threadIdx.x]);
}

}  // namespace elp

using namespace elp;

extern "C" {

int elp_replace_reference_dictionary(elp_ctx *c, const int32_t *new_of_old, int32_t n_ref_new, const int32_t *ref_len_new, uint64_t *n_rejected_out) {
  if (!c) return ELP_ERR_ARG;
  std::lock_guard<std::mutex> g(c->stage_mu);
  // every ARGUMENT check in front of the first launch and the first change: a call refused with ELP_ERR_ARG leaves columns, counts and
  // header as they were.  A HIP failure further down (a copy, a wait) is another matter: the columns may be renumbered by then and the
  // reference table replaced in part - the context is good for elp_reset / elp_set_header only, as after any failed launch.
  if (!c->have_header) return set_error(c, ELP_ERR_ARG, "elp_replace_reference_dictionary: call elp_set_header first");
  if (n_ref_new < 0 || (c->n_ref && !new_of_old) || (n_ref_new && !ref_len_new))
    return set_error(c, ELP_ERR_ARG, "elp_replace_reference_dictionary: bad arguments");
  const int32_t n_old = c->n_ref;
  for (int32_t r = 0; r < n_old; r++)
    if (new_of_old[r] < -1 || new_of_old[r] >= n_ref_new)
      return set_error(c, ELP_ERR_ARG, "elp_replace_reference_dictionary: new_of_old[%d] = %d is outside [-1, %d)", r, new_of_old[r], n_ref_new);
  ELP_HIP(c, hipSetDevice(c->device));
  if (n_rejected_out) *n_rejected_out = 0;
  const uint64_t n = c->n;
  unsigned long long h[2] = {0, 0};
  ELP_TRY(ensure(c, c->ref_len, (size_t)n_ref_new + 1));  // (what install_dictionary needs, while nothing has changed yet)
  if (n) {
    const DictionaryLayout L(n_old);
    uint8_t *blk;
    ELP_TRY(scratch(c, 5, L.bytes, &blk));
    unsigned long long *cnt = reinterpret_cast<unsigned long long *>(blk + L.counters);
    int32_t *d_map = reinterpret_cast<int32_t *>(blk + L.map);
    ELP_HIP(c, hipMemsetAsync(cnt, 0, 16, c->stream));
    if (n_old) ELP_HIP(c, hipMemcpyAsync(d_map, new_of_old, (size_t)n_old * 4, hipMemcpyHostToDevice, c->stream));
    const unsigned grid = DictionaryLayout::grid(n, c->n_cu);
    if (n_old <= REF_LDS)
      ELP_LAUNCH(c, "replace_dictionary", k_replace_dictionary<true>, dim3(grid), dim3(256), 0, n, c->refid.p, c->next_refid.p, c->has_sr.p,
                 (const int32_t *)d_map, n_old, cnt);
    else
      ELP_LAUNCH(c, "replace_dictionary", k_replace_dictionary<false>, dim3(grid), dim3(256), 0, n, c->refid.p, c->next_refid.p, c->has_sr.p,
                 (const int32_t *)d_map, n_old, cnt);
    ELP_HIP(c, hipMemcpyAsync(h, cnt, 16, hipMemcpyDeviceToHost, c->stream));
    ELP_HIP(c, elp::stream_wait(c->stream));
  }
  commit_rejects(c, h[0], h[1]);
  c->derived.dictionary_replaced();
  c->dict_replaced = true;
  ELP_TRY(install_dictionary(c, n_ref_new, ref_len_new));
  if (n_rejected_out) *n_rejected_out = h[0];
  return 0;
}

}  // extern "C"
