// bqsr_lut.hip — ApplyBQSR's LUT on the device: its way there ahead of the apply call, and the row dictionary of its resident part.
//   k_lut_rows_*, lut_dict_build   the distinct 17-byte rows of the resident part of the dense LUT (LutDict: one dictionary, or one per covariate)
//   k_lut_expand_rows   the dense LUT from its rows form (elp_bqsr_lut_upload_rows)
//   apply_shape         what ApplyBQSR's plan (apply_plan.hpp) depends on, from the context
//   elp_bqsr_lut_upload, elp_bqsr_lut_upload_rows   the LUT ahead of the apply call, on the copy stream; lut_uploaded builds the dictionary
//                       behind it when the facts the plan depends on are known
#include "bqsr_common.hpp"

namespace elp {

// ---- distinct rows of the dense LUT over (read group, quality in [qlo, qlo + n_qi), cycle in [-lmax, lmax]) ----
// per_cov (round 5, apply3's covariate split): one dictionary PER covariate - rows of different covariates never share an id, the ids
// count from 0 in every covariate (counter[cov]), covariate c's rows lie at t2 + c * LUT_PC_ROWS * 17
// (LUT_PC_ROWS, LUT_T2_CAP and the block's layout: apply_plan.hpp)
struct LutRows { const uint8_t *lut; int n_cov, qlo, n_qi, lmax, max_cycle, per_cov; };
__device__ __forceinline__ const uint8_t *lut_row(const LutRows &R, int r) {  // r = (cov * n_qi + qi) * w + x
  const int w = 2 * R.lmax + 1, ncyc = 2 * R.max_cycle + 1;
  const int x = r % w, qi = (r / w) % R.n_qi, cov = r / (w * R.n_qi);
  return R.lut + (((size_t)cov * ELP_NQUAL + (size_t)(R.qlo + qi)) * ncyc + (size_t)(x - R.lmax + R.max_cycle)) * 17;
}
__device__ __forceinline__ int lut_row_cov(const LutRows &R, int r) { return r / ((2 * R.lmax + 1) * R.n_qi); }
__device__ __forceinline__ bool row_eq(const uint8_t *a, const uint8_t *b) {
  bool eq = true;
#pragma unroll
  for (int k = 0; k < 17; k++) eq &= a[k] == b[k];
  return eq;
}
// every row finds or becomes the representative of its content in an open-addressing table of row indices
__global__ __launch_bounds__(256) void k_lut_rows_insert(LutRows R, int n_rows, uint32_t *slots, uint32_t mask, uint32_t *__restrict__ row_slot) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_rows) return;
  const uint8_t *mine = lut_row(R, r);
  const int my_cov = R.per_cov ? lut_row_cov(R, r) : 0;
  uint64_t h = 0x9e3779b97f4a7c15ull + (uint64_t)my_cov;
#pragma unroll
  for (int k = 0; k < 17; k++) h = (h ^ mine[k]) * 0x100000001b3ull;
  uint32_t s = (uint32_t)mix64(h) & mask;
  for (;;) {
    uint32_t cur = __hip_atomic_load(&slots[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == 0xFFFFFFFFu) {
      cur = atomicCAS(&slots[s], 0xFFFFFFFFu, (uint32_t)r);
      if (cur == 0xFFFFFFFFu) break;
    }
    if ((!R.per_cov || lut_row_cov(R, (int)cur) == my_cov) && row_eq(lut_row(R, (int)cur), mine)) break;
    s = (s + 1) & mask;
  }
  row_slot[r] = s;
}
// occupied slots get dense ids; the representative's row becomes row `id` of level 2
__global__ __launch_bounds__(256) void k_lut_rows_number(LutRows R, const uint32_t *__restrict__ slots, uint32_t n_slots, uint32_t *__restrict__ slot_id,
                                                         uint32_t *counter, uint8_t *__restrict__ t2, uint32_t t2_cap) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_slots) return;
  const uint32_t rep = slots[s];
  if (rep == 0xFFFFFFFFu) return;
  const int cov = R.per_cov ? lut_row_cov(R, (int)rep) : 0;
  const uint32_t id = atomicAdd(counter + cov, 1u);
  slot_id[s] = id;
  if (id < t2_cap) {
    const uint8_t *src = lut_row(R, (int)rep);
    uint8_t *dst = t2 + ((size_t)cov * LUT_PC_ROWS + id) * 17;  // (cov = 0 without per_cov)
    for (int k = 0; k < 17; k++) dst[k] = src[k];
  }
}
// level 1 [cov][n_qi + 1][w]: ids; the extra row per read group and (below) the extra level-2 row stand for "not resident"
__global__ __launch_bounds__(256) void k_lut_rows_index(LutRows R, const uint32_t *__restrict__ row_slot, const uint32_t *__restrict__ slot_id,
                                                        const uint32_t *__restrict__ counter, uint16_t *__restrict__ t1, uint8_t *__restrict__ t2,
                                                        uint32_t t2_cap) {
  const int w = 2 * R.lmax + 1, n1 = R.n_cov * (R.n_qi + 1) * w;
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < 17 * (R.per_cov ? R.n_cov : 1)) {  // the 0x80 row behind (every covariate's) distinct rows
    const int cv = k / 17;
    const uint32_t nd = counter[cv];
    if (nd < t2_cap) t2[((size_t)cv * LUT_PC_ROWS + nd) * 17 + (k - 17 * cv)] = 0x80;
  }
  if (k >= n1) return;
  const int x = k % w, qi = (k / w) % (R.n_qi + 1), cov = k / (w * (R.n_qi + 1));
  const uint32_t n_dict = counter[R.per_cov ? cov : 0];
  t1[k] = qi == R.n_qi ? (uint16_t)n_dict : (uint16_t)slot_id[row_slot[(cov * R.n_qi + qi) * w + x]];
}

// the dense LUT [n_cov][94][ncyc][17] from its rows form: rows [n_cov][nq][ncyc][17] for the qualities with a slot, the default byte else
__global__ __launch_bounds__(256) void k_lut_expand_rows(const uint8_t *__restrict__ rows, const uint8_t *__restrict__ defaults, const uint8_t *__restrict__ slot_of /* [94], 255 = none */,
                                                        int n_cov, int nq, int ncyc, uint8_t *__restrict__ lut) {
  const size_t row_b = (size_t)ncyc * 17, k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= (size_t)n_cov * ELP_NQUAL * row_b) return;
  const size_t r = k / row_b, w = k - r * row_b, cv = r / ELP_NQUAL, q = r % ELP_NQUAL;
  const uint8_t sl = slot_of[q];
  lut[k] = sl == 255 ? defaults[r] : rows[((cv * (size_t)nq + sl) * row_b) + w];
}

// Distinct rows of the resident part of the dense LUT (three small kernels) into the block D lies in.
// (plain launches, no profiling brackets: also called from the upload thread while the context's own stream is busy)
int lut_dict_build(elp_ctx *c, hipStream_t st, const LutDict &D, const uint8_t *dl, int qlo, int n_qi, int lmax, int max_cycle, bool per_cov) {
  ELP_HIP(c, hipMemsetAsync(D.slots, 0xFF, (size_t)D.n_slots * 4, st));
  ELP_HIP(c, hipMemsetAsync(D.counter, 0, 256 * 4, st));
  LutRows R{dl, c->n_cov, qlo, n_qi, lmax, max_cycle, per_cov ? 1 : 0};
  const uint32_t cap = per_cov ? LUT_PC_ROWS : LUT_T2_CAP;
  hipLaunchKernelGGL(k_lut_rows_insert, dim3(blocks_for(D.n_rows, 256)), dim3(256), 0, st, R, (int)D.n_rows, D.slots, D.n_slots - 1, D.row_slot);
  hipLaunchKernelGGL(k_lut_rows_number, dim3(blocks_for(D.n_slots, 256)), dim3(256), 0, st, R, (const uint32_t *)D.slots, D.n_slots, D.slot_id, D.counter, D.t2, cap);
  hipLaunchKernelGGL(k_lut_rows_index, dim3(blocks_for(std::max<size_t>(D.n1, 17 * 256), 256)), dim3(256), 0, st, R, (const uint32_t *)D.row_slot, (const uint32_t *)D.slot_id,
                     (const uint32_t *)D.counter, D.t1, D.t2, cap);
  ELP_HIP(c, hipGetLastError());
  return 0;
}

// the resident quality range of ApplyBQSR's LDS tables, from the quality hint (-1: no quality >= 6 seen)
static void lut_quality_range(const elp_ctx *c, int *qlo, int *qhi) {
  *qlo = 0; *qhi = -1;
  for (int q = 6; q < ELP_NQUAL; q++)
    if ((q < 64 ? (c->qual_present[0] >> q) : (c->qual_present[1] >> (q - 64))) & 1ull) { if (*qhi < 0) *qlo = q; *qhi = q; }
}
// reads the quality hint and the one-length fact as they stand: the caller has made them (ensure_qual_present, ensure_uniform_len) or found them made
ApplyShape apply_shape(const elp_ctx *c, int max_cycle) {
  ApplyShape s{};
  s.n = c->n; s.n_cov = c->n_cov; s.max_l_seq = c->max_l_seq; s.uniform_len = c->uniform_len; s.max_cycle = max_cycle;
  lut_quality_range(c, &s.qlo, &s.qhi);
  s.apply_kernel = c->tune.apply_kernel; s.apply_wgs = c->tune.apply_wgs; s.n_cu = c->n_cu;
  s.lds_flat = APPLY_STATIC_LDS; s.lds_apply3 = APPLY3_STATIC_LDS; s.lds_apply3_split = APPLY3_STATIC_LDS_SPLIT;
  return s;
}

}  // namespace elp

using namespace elp;

extern "C" {

// The LUT's way to the device ahead of the apply call: from the thread that built it, on the context's copy stream, while the context's
// own stream still runs the sort / metrics pass (6.4 MB at --max-cycle 500: ~0.2 ms that elp_bqsr_apply otherwise spends in front of its
// first kernel).  The LUT lives in a buffer of its own (not in the scratch pool: other stages are running).
//
// What both forms of the upload begin with: the pinned buffer free again and large enough for `small` bytes and - unless `bulk` already sits in
// page-locked memory (elp_pinned_alloc) - `bulk_bytes` more.  A pinned LUT is copied from where it is - with many read groups the LUT is tens of
// megabytes and the staging copy was the longest part of the host's table path; the caller then leaves it alone until the elp_bqsr_apply that
// uses it has been called and the context synchronised.
static int lut_staging(elp_ctx *c, const void *bulk, size_t bulk_bytes, size_t small, bool *caller_pinned) {
  ELP_HIP(c, hipSetDevice(c->device));
  if (c->lut_ev) ELP_HIP(c, hipEventSynchronize(c->lut_ev));  // (a previous upload still in flight reads the pinned buffer)
  hipPointerAttribute_t pa;
  *caller_pinned = bulk_bytes && hipPointerGetAttributes(&pa, bulk) == hipSuccess && pa.type == hipMemoryTypeHost;
  if (!*caller_pinned) (void)hipGetLastError();  // (ordinary memory: the query fails, by design)
  const size_t staged = small + (*caller_pinned ? 0 : bulk_bytes);
  if (staged > c->lut_pinned_cap) {
    if (c->lut_pinned) (void)hipHostFree(c->lut_pinned);
    c->lut_pinned = nullptr; c->lut_pinned_cap = 0;
    ELP_HIP(c, hipHostMalloc(&c->lut_pinned, staged, hipHostMallocDefault));
    c->lut_pinned_cap = staged;
  }
  if (!c->lut_ev) ELP_HIP(c, hipEventCreateWithFlags(&c->lut_ev, hipEventDisableTiming));
  if (!c->copy_stream) ELP_HIP(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));  // (not the NULL stream all contexts share)
  if (c->apply_ev) ELP_HIP(c, hipStreamWaitEvent(c->copy_stream, c->apply_ev, 0));  // an apply that still reads the previous LUT
  return 0;
}

// behind the LUT's arrival in lut_dev on the copy stream: the row dictionary apply3 works from - if what the plan depends on is known now (the
// quality hint of the gather that produced these tables, the one-length fact for this read set): 0.25 ms that elp_bqsr_apply otherwise spends
// in front of its kernel - and the event the apply waits for.  (No ensure_* here: the context's own stream is busy.)
static int lut_uploaded(elp_ctx *c, int max_cycle) {
  c->dict_built = LutDictBuilt();
  if (c->derived.have_qual_present && c->derived.uniform_n == c->n && c->n > 0) {
    const ApplyPlan P = apply_plan(apply_shape(c, max_cycle));
    if (P.a3) {
      const LutDictLayout L(c->n_cov, P.n_qi, P.lmax);
      ELP_TRY(ensure(c, c->lut_wk, L.words));
      ELP_TRY(lut_dict_build(c, c->copy_stream, lut_dict_at(c->lut_wk.p, L), c->lut_dev.p, P.qlo, P.n_qi, P.lmax, max_cycle, P.a3 == 2));
      c->dict_built = LutDictBuilt::of(P);
    }
  }
  ELP_HIP(c, hipEventRecord(c->lut_ev, c->copy_stream));
  c->lut_uploaded_cycle = max_cycle;
  return 0;
}

int elp_bqsr_lut_upload(elp_ctx *c, int max_cycle, const uint8_t *lut, const uint8_t *cov_present) {
  if (!c || !lut || !cov_present || max_cycle < 1) return set_error(c, ELP_ERR_ARG, "elp_bqsr_lut_upload: bad arguments");
  const size_t lut_bytes = (size_t)c->n_cov * ELP_NQUAL * (2 * (size_t)max_cycle + 1) * 17, all = lut_bytes + (size_t)c->n_cov;
  bool caller_pinned;
  ELP_TRY(lut_staging(c, lut, lut_bytes, (size_t)c->n_cov, &caller_pinned));
  ELP_TRY(ensure(c, c->lut_dev, all + 64));
  if (!caller_pinned) memcpy(c->lut_pinned, lut, lut_bytes);
  memcpy(static_cast<uint8_t *>(c->lut_pinned) + (caller_pinned ? 0 : lut_bytes), cov_present, (size_t)c->n_cov);
  if (caller_pinned) {
    ELP_HIP(c, hipMemcpyAsync(c->lut_dev.p, lut, lut_bytes, hipMemcpyHostToDevice, c->copy_stream));
    ELP_HIP(c, hipMemcpyAsync(c->lut_dev.p + lut_bytes, c->lut_pinned, (size_t)c->n_cov, hipMemcpyHostToDevice, c->copy_stream));
  } else {
    ELP_HIP(c, hipMemcpyAsync(c->lut_dev.p, c->lut_pinned, all, hipMemcpyHostToDevice, c->copy_stream));
  }
  return lut_uploaded(c, max_cycle);
}

// elp_bqsr_lut_upload for the LUT in rows form (the host library's elp_bqsr_tables_build_lut_rows): n_cov x n_quals rows + one default byte
// per other row instead of n_cov x 94 rows - with 16 read groups 1.9 MB instead of 25.6 MB over PCIe (and 13 x less for the host to fill);
// a kernel on the copy stream expands it into the dense LUT every apply kernel reads.
int elp_bqsr_lut_upload_rows(elp_ctx *c, int max_cycle, const uint8_t *quals, int n_quals, const uint8_t *rows, const uint8_t *defaults, const uint8_t *cov_present) {
  if (!c || max_cycle < 1 || n_quals < 0 || n_quals > ELP_NQUAL || (n_quals && (!quals || !rows)) || !defaults || !cov_present)
    return set_error(c, ELP_ERR_ARG, "elp_bqsr_lut_upload_rows: bad arguments");
  uint8_t slot_of[ELP_NQUAL];
  memset(slot_of, 255, sizeof slot_of);
  for (int k = 0; k < n_quals; k++) {
    if (quals[k] >= ELP_NQUAL || slot_of[quals[k]] != 255) return set_error(c, ELP_ERR_ARG, "elp_bqsr_lut_upload_rows: quality list");
    slot_of[quals[k]] = (uint8_t)k;
  }
  const size_t ncyc = 2 * (size_t)max_cycle + 1, row_b = ncyc * 17;
  const size_t rows_bytes = (size_t)c->n_cov * (size_t)n_quals * row_b, def_bytes = (size_t)c->n_cov * ELP_NQUAL;
  const size_t lut_bytes = (size_t)c->n_cov * ELP_NQUAL * row_b, small = def_bytes + ELP_NQUAL + (size_t)c->n_cov;  // defaults | slot_of | cov_present
  bool caller_pinned;
  ELP_TRY(lut_staging(c, rows, rows_bytes, small, &caller_pinned));
  uint8_t *hp = static_cast<uint8_t *>(c->lut_pinned);
  memcpy(hp, defaults, def_bytes);
  memcpy(hp + def_bytes, slot_of, ELP_NQUAL);
  memcpy(hp + def_bytes + ELP_NQUAL, cov_present, (size_t)c->n_cov);
  if (!caller_pinned && rows_bytes) memcpy(hp + small, rows, rows_bytes);
  ELP_TRY(ensure(c, c->lut_dev, lut_bytes + (size_t)c->n_cov + 64));
  ELP_TRY(ensure(c, c->lut_rows_dev, rows_bytes + small + 64));
  uint8_t *d_small = c->lut_rows_dev.p, *d_rows = c->lut_rows_dev.p + ((small + 63) & ~(size_t)63);
  ELP_HIP(c, hipMemcpyAsync(d_small, hp, small, hipMemcpyHostToDevice, c->copy_stream));
  if (rows_bytes) ELP_HIP(c, hipMemcpyAsync(d_rows, caller_pinned ? rows : hp + small, rows_bytes, hipMemcpyHostToDevice, c->copy_stream));
  hipLaunchKernelGGL(k_lut_expand_rows, dim3(blocks_for(lut_bytes, 256)), dim3(256), 0, c->copy_stream, (const uint8_t *)d_rows, (const uint8_t *)d_small,
                     (const uint8_t *)(d_small + def_bytes), c->n_cov, n_quals, (int)ncyc, c->lut_dev.p);
  ELP_HIP(c, hipGetLastError());
  ELP_HIP(c, hipMemcpyAsync(c->lut_dev.p + lut_bytes, d_small + def_bytes + ELP_NQUAL, (size_t)c->n_cov, hipMemcpyDeviceToDevice, c->copy_stream));
  return lut_uploaded(c, max_cycle);
}

}  // extern "C"
