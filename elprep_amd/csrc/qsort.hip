// qsort.hip — the queryname sort: By(QNAMELess).ParallelStableSort (sam/filter-pipeline.go:118-122, sam/sam-types.go:475-481, :639-641).
//
// Order: QNAME bytes as Go compares strings (unsigned bytes, a proper prefix first), ties keep staging order; records that are not
// output (has_sr column != 0: sr-tagged copies, records rejected by elp_filter_records) go behind the others, in the same order.
//
// Every record is a member of one tie group whose comparator is the name alone, so the coordinate sort's tie-break (sort.hip) is run
// over the whole read set, without its keys (the rank tables and the packing of the keys are the same host code, sort_plan.hpp):
//   (1) k_qn_values: one sweep over the names, eight bytes per load, zero-padded to the longest name: the set of byte values that occur
//       at every position (256 bits per position, in LDS); positions with more than one value are live.  One read-back.
//   (2) k_qn_keys: a 64-bit key per record = {state, ranks of its bytes at the most significant live positions} (a rank takes as few
//       bits as the position's value count needs: read names have ~10 values per live position), then ONE stable radix pair sort.
//   (3) k_qn_ties: what the key leaves open is settled by whole-name comparison inside the groups of equal keys (the two mates of a
//       pair, mostly) and written into the permutation.  A group of more than QN_CAP members raises a flag (one read-back): the host then
//       runs stable LSD rounds over every field instead.
// Zero padding is a coarsening of Go's order: names that differ only in trailing NUL bytes pad to the same string.  The sweep flags a
// NUL inside a name; the name length then becomes the least significant field of the key (a shorter name is a prefix of the longer).
#include <algorithm>
#include <cstring>
#include <vector>

#include "common.hpp"
#include "sort_plan.hpp"  // QN_STATE, QN_LEN; the fields, their ranks and the cuts of the rounds

namespace elp {

// fields of a key, most significant first: pos[j] < QN_LEN is a byte position (rank = lut[slot[j] * 256 + padded byte]), QN_STATE the
// record state (not output = 1), QN_LEN the name length; field j sits at bit shift[j]
struct QnFields { uint16_t pos[64]; uint16_t slot[64]; uint8_t shift[64]; uint32_t n; };
constexpr uint32_t QN_CAP = 64;  // largest group of equal keys ranked by comparison (all pairs)

// vals[k * 8 .. k * 8 + 7] |= the byte values at position k (k < maxq, past a name's end: 0); vals[maxq * 8] = 1 if a name holds a NUL
__global__ __launch_bounds__(256) void k_qn_values(uint64_t n, const uint64_t *__restrict__ qoff, const uint8_t *__restrict__ q, uint32_t maxq,
                                                   uint32_t *vals) {
  extern __shared__ uint32_t acc[];  // [maxq * 8]
  for (uint32_t k = threadIdx.x; k < maxq * 8; k += blockDim.x) acc[k] = 0;
  __syncthreads();
  bool nul = false;
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t o = qoff[r];
    const uint32_t l = (uint32_t)(qoff[r + 1] - o);
    for (uint32_t k = 0; k < maxq; k += 8) {
      const uint64_t w = k < l ? low_bytes(load8(q + o + k), l - k) : 0ull;  // (the column is padded by 64 bytes)
      const uint32_t m = maxq - k < 8 ? maxq - k : 8;
      for (uint32_t i = 0; i < m; i++) {
        const uint32_t v = (uint32_t)(w >> (8 * i)) & 0xFFu;
        nul |= v == 0 && k + i < l;
        uint32_t *a = &acc[(k + i) * 8 + (v >> 5)];
        const uint32_t bit = 1u << (v & 31u);
        if (!(*a & bit)) atomicOr(a, bit);
      }
    }
  }
  if (nul) atomicOr(&vals[maxq * 8], 1u);
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < maxq * 8; k += blockDim.x)
    if (acc[k]) atomicOr(&vals[k], acc[k]);
}

// keys[j] = the fields of record order[j] (order == nullptr: record j)
__global__ __launch_bounds__(256) void k_qn_keys(uint64_t n, const uint32_t *__restrict__ order, QnFields f, const uint8_t *__restrict__ lut,
                                                 const uint64_t *__restrict__ qoff, const uint8_t *__restrict__ q, const uint8_t *__restrict__ state,
                                                 uint64_t *__restrict__ keys) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const uint32_t r = order ? order[j] : (uint32_t)j;
  const uint64_t o = qoff[r];
  const uint32_t l = (uint32_t)(qoff[r + 1] - o);
  uint64_t k = 0, w = 0;
  uint32_t wi = 0xFFFFFFFFu;  // index of the eight-byte word in w (byte positions ascend within a key: most loads are reused)
  for (uint32_t b = 0; b < f.n; b++) {
    const uint32_t p = f.pos[b];
    uint64_t v;
    if (p == QN_STATE) v = state[r] != 0;
    else if (p == QN_LEN) v = l;
    else {
      if ((p >> 3) != wi) {
        wi = p >> 3;
        const uint32_t at = wi * 8;
        w = at < l ? low_bytes(load8(q + o + at), l - at) : 0ull;
      }
      v = lut[(uint32_t)f.slot[b] * 256u + ((uint32_t)(w >> (8 * (p & 7))) & 0xFFu)];
    }
    k |= v << f.shift[b];
  }
  keys[j] = k;
}

// perm[j] = the record at sorted position j.  settled: equal keys are equal names (the stable passes kept staging order).  Otherwise a
// record whose neighbours have other keys is final, and the members of a group of equal keys rank themselves by whole-name comparison
// (equal names: the earlier record first); a group of more than QN_CAP members sets *over (the host runs the LSD rounds instead).
__global__ __launch_bounds__(256) void k_qn_ties(uint64_t n, const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals,
                                                 uint32_t *__restrict__ perm, const uint64_t *__restrict__ qoff, const uint8_t *__restrict__ q,
                                                 uint32_t settled, uint32_t *over) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const uint32_t me = vals[j];
  if (settled) { perm[j] = me; return; }
  const uint64_t k = keys[j];
  const bool eq_prev = j > 0 && keys[j - 1] == k, eq_next = j + 1 < n && keys[j + 1] == k;
  if (!eq_prev && !eq_next) { perm[j] = me; return; }
  uint64_t s = j, e = j + 1;  // the group [s, e)
  bool large = false;
  while (s > 0 && keys[s - 1] == k) {
    s--;
    if (j - s >= QN_CAP) { large = true; break; }
  }
  while (!large && e < n && keys[e] == k) {
    e++;
    if (e - s > QN_CAP) large = true;
  }
  if (large) {
    perm[j] = me;
    if (!eq_prev) atomicOr(over, 1u);
    return;
  }
  uint32_t rank = 0;
  for (uint64_t i = s; i < e; i++) {
    if (i == j) continue;
    const uint32_t other = vals[i];
    const int c = qname_cmp(q, qoff, other, me);
    if (c < 0 || (c == 0 && other < me)) rank++;
  }
  perm[s + rank] = me;
}

// What the phases of one queryname sort hand on.  Scratch slots 1 .. 3 of the lane (sort_plan.hpp: slot 0 holds the coordinate key
// passes made ahead, elp_sort_ahead, which stay valid).
struct QnWork {
  uint64_t n;
  uint32_t maxq;  // <= MAX_QNAME (elp_stage enforces it)
  QnScratch lay;
  uint64_t *k0 = nullptr, *k1 = nullptr;
  uint32_t *vcur = nullptr, *vtmp = nullptr;
  uint32_t *d_vals = nullptr, *d_over = nullptr;
  uint8_t *d_lut = nullptr;
  const uint64_t *qoff = nullptr;
  const uint8_t *q = nullptr, *state = nullptr;
  QnWork(uint64_t records, uint32_t longest) : n(records), maxq(longest), lay(longest) {}
};

static QnFields qn_packed(const RankFields &f, FieldCut cut) {
  QnFields p;
  memset(&p, 0, sizeof p);
  for (int k = cut.lo; k < cut.hi; k++, p.n++) { p.pos[p.n] = f.pos[k]; p.slot[p.n] = f.slot[k]; }
  field_shifts(f.bits, cut, p.shift);
  return p;
}

// (1) the values at every position: one kernel, one read-back; from them the key's fields and the rank LUT
static int qn_tables(elp_ctx *c, QnWork &w, RankFields *f) {
  const SortScratch sc(w.n);
  uint64_t *kbuf;
  uint32_t *vbuf, *small;
  ELP_TRY(scratch(c, 1, sc.keys, &kbuf));
  ELP_TRY(scratch(c, 2, sc.vals, &vbuf));
  ELP_TRY(scratch(c, 3, w.lay.words3, &small));
  w.k0 = kbuf; w.k1 = kbuf + w.n;
  w.vcur = vbuf; w.vtmp = vbuf + w.n;
  w.d_vals = small; w.d_over = small + w.lay.d_over;
  w.d_lut = reinterpret_cast<uint8_t *>(small + w.lay.d_lut);
  w.qoff = c->qname_off.p; w.q = c->qname.p; w.state = c->has_sr.p;
  std::vector<uint32_t> hv(w.lay.vwords, 0);
  if (w.maxq > 0) {
    ELP_HIP(c, hipMemsetAsync(w.d_vals, 0, (w.lay.vwords + 1) * 4, c->stream));
    const unsigned grid = std::min<unsigned>(blocks_for(w.n, 256), (unsigned)c->n_cu * 4);
    ELP_LAUNCH(c, "qn_values", k_qn_values, dim3(grid), dim3(256), (size_t)w.maxq * 8 * 4, w.n, w.qoff, w.q, w.maxq, w.d_vals);
    ELP_HIP(c, hipMemcpyAsync(hv.data(), w.d_vals, w.lay.vwords * 4, hipMemcpyDeviceToHost, c->stream));
    ELP_HIP(c, elp::stream_wait(c->stream));
  } else {
    ELP_HIP(c, hipMemsetAsync(w.d_over, 0, 4, c->stream));
  }
  *f = qn_fields(hv.data(), w.maxq, c->n_sr > 0);
  if (!f->lut.empty()) ELP_HIP(c, hipMemcpyAsync(w.d_lut, f->lut.data(), f->lut.size(), hipMemcpyHostToDevice, c->stream));
  return 0;
}

// (2) one key of the most significant fields that fit, (3) the groups of equal keys, into the permutation.  *done = the permutation
// stands; else a group of more than QN_CAP equal keys was found
static int qn_key_round(elp_ctx *c, QnWork &w, const RankFields &f, bool *done) {
  const unsigned g = blocks_for(w.n, 256);
  const FieldCut cut = pack_prefix(f.bits, 0);
  const bool settled = cut.hi == f.n();
  const QnFields p = qn_packed(f, cut);
  ELP_LAUNCH(c, "qn_keys", k_qn_keys, dim3(g), dim3(256), 0, w.n, (const uint32_t *)nullptr, p, (const uint8_t *)w.d_lut, w.qoff, w.q, w.state, w.k0);
  uint64_t *ko;
  uint32_t *vo;
  ELP_TRY(radix_sort_pairs_low(c, w.k0, w.vcur, w.k1, w.vtmp, w.n, key_digits(cut.total), &ko, &vo, nullptr, true));
  c->radix_check_pending = true;  // (read by the caller: radix_check)
  ELP_LAUNCH(c, "qn_ties", k_qn_ties, dim3(g), dim3(256), 0, w.n, (const uint64_t *)ko, (const uint32_t *)vo, c->perm.p, w.qoff, w.q,
             (uint32_t)settled, w.d_over);
  *done = settled;
  if (settled) return 0;
  uint32_t h_over = 0;
  ELP_HIP(c, hipMemcpyAsync(&h_over, w.d_over, 4, hipMemcpyDeviceToHost, c->stream));
  ELP_HIP(c, elp::stream_wait(c->stream));
  *done = !h_over;
  return 0;
}

// a group of more than QN_CAP equal keys: stable LSD rounds over every field, least significant first, from staging order
static int qn_lsd_rounds(elp_ctx *c, QnWork &w, const RankFields &f) {
  const unsigned g = blocks_for(w.n, 256);
  const uint32_t *order = nullptr;
  for (const FieldCut &cut : lsd_cuts(f.bits)) {
    const QnFields p = qn_packed(f, cut);
    ELP_LAUNCH(c, "qn_keys", k_qn_keys, dim3(g), dim3(256), 0, w.n, order, p, (const uint8_t *)w.d_lut, w.qoff, w.q, w.state, w.k0);
    uint64_t *ko;
    uint32_t *vo;
    ELP_TRY(radix_sort_pairs_low(c, w.k0, w.vcur, w.k1, w.vtmp, w.n, key_digits(cut.total), &ko, &vo, nullptr, order == nullptr));
    if (vo != w.vcur) std::swap(w.vcur, w.vtmp);
    order = w.vcur;
  }
  ELP_LAUNCH(c, "qn_ties", k_qn_ties, dim3(g), dim3(256), 0, w.n, (const uint64_t *)w.k0, (const uint32_t *)w.vcur, c->perm.p, w.qoff, w.q, 1u, w.d_over);
  return 0;
}

// the queryname sort of c's records into c->perm, on c's stream (c: the side lane's shadow context, sort_queryname below)
static int qname_sort_impl(elp_ctx *c) {
  if (c->n == 0) return 0;
  QnWork w(c->n, c->max_qname_len);
  RankFields f;
  ELP_TRY(qn_tables(c, w, &f));
  bool done = false;
  ELP_TRY(qn_key_round(c, w, f, &done));
  return done ? 0 : qn_lsd_rounds(c, w, f);
}


// On the context's side lane 1, as the coordinate sort (sort.hip, sort_on_side): the shadow sees the name columns, the state column and
// the permutation's buffer as views for the duration of the call.  Nothing of the adapt stage (keys, scores) is read or made.
static int sort_queryname(elp_ctx *c) {
  ELP_TRY(ensure(c, c->perm, c->n + 1));
  elp_ctx *s = nullptr;
  ELP_TRY(side_lane(c, 1, &s));
  s->n = c->n; s->n_sr = c->n_sr; s->max_qname_len = c->max_qname_len;
  int rc;
  {
    LaneViews views(s, c, &elp_ctx::qname_off, &elp_ctx::qname, &elp_ctx::has_sr);
    views.view(s->perm, c->perm, true);
    rc = qname_sort_impl(s);
  }
  if (rc == 0) rc = radix_check(s);  // (the lane's own error words: a look-back timeout of its passes is read here)
  if (rc != 0) {
    (void)elp::stream_wait(s->stream);
    c->err = s->err;
    return rc;
  }
  ELP_TRY(side_join(c, 1));
  c->derived.set_sorted(true);
  return 0;
}

}  // namespace elp

extern "C" int elp_sort_queryname(elp_ctx *c) {
  if (!c) return ELP_ERR_ARG;
  ELP_HIP(c, hipSetDevice(c->device));
  c->derived.drop_sorted();
  return elp::sort_queryname(c);
}
