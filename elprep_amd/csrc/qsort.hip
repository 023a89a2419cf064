// qsort.hip — the queryname sort: By(QNAMELess).ParallelStableSort (sam/filter-pipeline.go:118-122, sam/sam-types.go:475-481, :639-641).
//
// Order: QNAME bytes as Go compares strings (unsigned bytes, a proper prefix first), ties keep staging order; records that are not
// output (has_sr column != 0: sr-tagged copies, records rejected by elp_filter_records) go behind the others, in the same order.
//
// Every record is a member of one tie group whose comparator is the name alone, so the coordinate sort's tie-break (sort.hip) is run
// over the whole read set, without its keys:
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

namespace elp {

// fields of a key, most significant first: pos[j] < QN_STATE is a byte position (rank = lut[slot[j] * 256 + padded byte]), QN_STATE the
// record state (not output = 1), QN_LEN the name length; field j sits at bit shift[j]
constexpr uint16_t QN_STATE = 0xFFFF, QN_LEN = 0xFFFE;
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

// the queryname sort of c's records into c->perm, on c's stream (c: the side lane's shadow context, sort_queryname below)
static int qname_sort_impl(elp_ctx *c) {
  const uint64_t n = c->n;
  if (n == 0) return 0;
  const uint32_t maxq = c->max_qname_len;  // <= MAX_QNAME (elp_stage enforces it)
  // scratch slots 1 .. 3: slot 0 of the sort lane holds the coordinate key passes made ahead (elp_sort_ahead), which stay valid
  uint64_t *kbuf;
  uint32_t *vbuf, *small;
  ELP_TRY(scratch(c, 1, 2 * n + 8, &kbuf));
  ELP_TRY(scratch(c, 2, 2 * n + 8, &vbuf));
  const size_t vwords = (size_t)maxq * 8 + 1, lut_words = ((size_t)maxq * 256 + 3) / 4;
  ELP_TRY(scratch(c, 3, vwords + 1 + lut_words, &small));
  uint32_t *d_vals = small, *d_over = small + vwords;
  uint8_t *d_lut = reinterpret_cast<uint8_t *>(small + vwords + 1);
  const uint64_t *qoff = c->qname_off.p;
  const uint8_t *q = c->qname.p, *state = c->has_sr.p;
  // (1) the values at every position: one kernel, one read-back
  std::vector<uint32_t> hv(vwords, 0);
  if (maxq > 0) {
    ELP_HIP(c, hipMemsetAsync(d_vals, 0, (vwords + 1) * 4, c->stream));
    const unsigned grid = std::min<unsigned>(blocks_for(n, 256), (unsigned)c->n_cu * 4);
    ELP_LAUNCH(c, "qn_values", k_qn_values, dim3(grid), dim3(256), (size_t)maxq * 8 * 4, n, qoff, q, maxq, d_vals);
    ELP_HIP(c, hipMemcpyAsync(hv.data(), d_vals, vwords * 4, hipMemcpyDeviceToHost, c->stream));
    ELP_HIP(c, elp::stream_wait(c->stream));
  } else {
    ELP_HIP(c, hipMemsetAsync(d_over, 0, 4, c->stream));
  }
  // the fields, most significant first: the state (if any record is not output), the live positions (ranks), the length (if a name
  // holds a NUL byte)
  std::vector<uint16_t> fpos, fslot;
  std::vector<int> fbits;
  if (c->n_sr > 0) { fpos.push_back(QN_STATE); fslot.push_back(0); fbits.push_back(1); }
  std::vector<uint8_t> lut;
  uint32_t nlive = 0;
  for (uint32_t p = 0; p < maxq; p++) {
    int cnt = 0;
    for (int w = 0; w < 8; w++) cnt += __builtin_popcount(hv[(size_t)p * 8 + w]);
    if (cnt < 2) continue;
    lut.resize((size_t)(nlive + 1) * 256, 0);
    int rank = 0;
    for (int v = 0; v < 256; v++)
      if ((hv[(size_t)p * 8 + (v >> 5)] >> (v & 31)) & 1u) lut[(size_t)nlive * 256 + v] = (uint8_t)rank++;
    int b = 1;
    while ((1 << b) < rank) b++;
    fpos.push_back((uint16_t)p); fslot.push_back((uint16_t)nlive); fbits.push_back(b);
    nlive++;
  }
  if (maxq > 0 && hv[(size_t)maxq * 8]) { fpos.push_back(QN_LEN); fslot.push_back(0); fbits.push_back(11); }  // lengths <= MAX_QNAME < 2^11
  if (!lut.empty()) ELP_HIP(c, hipMemcpyAsync(d_lut, lut.data(), lut.size(), hipMemcpyHostToDevice, c->stream));
  const int nf = (int)fpos.size();
  // fields [lo, hi) as one key, packed below bit 64 (lower fields in lower bits)
  auto pack = [&](int lo, int hi, int *total) {
    QnFields f;
    memset(&f, 0, sizeof f);
    int sh = 0;
    for (int k = lo; k < hi; k++) sh += fbits[k];
    *total = sh;
    for (int k = lo; k < hi; k++) {
      sh -= fbits[k];
      f.pos[f.n] = fpos[k]; f.slot[f.n] = fslot[k]; f.shift[f.n] = (uint8_t)sh;
      f.n++;
    }
    return f;
  };
  uint64_t *k0 = kbuf, *k1 = kbuf + n;
  uint32_t *vcur = vbuf, *vtmp = vbuf + n;
  const unsigned g = blocks_for(n, 256);
  // (2) one key of the most significant fields that fit
  int hi = 0, bits = 0;
  while (hi < nf && hi < 64 && bits + fbits[hi] <= 64) bits += fbits[hi++];
  const bool settled = hi == nf;
  int total = 0;
  QnFields f = pack(0, hi, &total);
  ELP_LAUNCH(c, "qn_keys", k_qn_keys, dim3(g), dim3(256), 0, n, (const uint32_t *)nullptr, f, (const uint8_t *)d_lut, qoff, q, state, k0);
  uint64_t *ko;
  uint32_t *vo;
  ELP_TRY(radix_sort_pairs_low(c, k0, vcur, k1, vtmp, n, (total + 7) / 8, &ko, &vo, nullptr, true));
  c->radix_check_pending = true;  // (read by the caller: radix_check)
  // (3) the groups of equal keys, into the permutation
  ELP_LAUNCH(c, "qn_ties", k_qn_ties, dim3(g), dim3(256), 0, n, (const uint64_t *)ko, (const uint32_t *)vo, c->perm.p, qoff, q,
             (uint32_t)settled, d_over);
  if (settled) return 0;
  uint32_t h_over = 0;
  ELP_HIP(c, hipMemcpyAsync(&h_over, d_over, 4, hipMemcpyDeviceToHost, c->stream));
  ELP_HIP(c, elp::stream_wait(c->stream));
  if (!h_over) return 0;
  // a group of more than QN_CAP equal keys: stable LSD rounds over every field, least significant first, from staging order
  const uint32_t *order = nullptr;
  for (int top = nf; top > 0;) {
    int lo = top, tb = 0;
    while (lo > 0 && tb + fbits[lo - 1] <= 64 && top - lo < 64) tb += fbits[--lo];
    QnFields fr = pack(lo, top, &total);
    ELP_LAUNCH(c, "qn_keys", k_qn_keys, dim3(g), dim3(256), 0, n, order, fr, (const uint8_t *)d_lut, qoff, q, state, k0);
    ELP_TRY(radix_sort_pairs_low(c, k0, vcur, k1, vtmp, n, (total + 7) / 8, &ko, &vo, nullptr, order == nullptr));
    if (vo != vcur) std::swap(vcur, vtmp);
    order = vcur;
    top = lo;
  }
  ELP_LAUNCH(c, "qn_ties", k_qn_ties, dim3(g), dim3(256), 0, n, (const uint64_t *)k0, (const uint32_t *)vcur, c->perm.p, qoff, q, 1u, d_over);
  return 0;
}

// On the context's side lane 1, as the coordinate sort (sort.hip, sort_on_side): the shadow sees the name columns, the state column and
// the permutation's buffer as views for the duration of the call.  Nothing of the adapt stage (keys, scores) is read or made.
static int sort_queryname(elp_ctx *c) {
  ELP_TRY(ensure(c, c->perm, c->n + 1));
  elp_ctx *s = nullptr;
  ELP_TRY(side_lane(c, 1, &s));
  s->n = c->n; s->n_sr = c->n_sr; s->max_qname_len = c->max_qname_len;
  s->qname_off.p = c->qname_off.p; s->qname.p = c->qname.p; s->has_sr.p = c->has_sr.p;
  s->perm.p = c->perm.p; s->perm.cap = c->perm.cap;
  int rc = qname_sort_impl(s);
  s->qname_off.p = nullptr; s->qname.p = nullptr; s->has_sr.p = nullptr;
  s->perm.p = nullptr; s->perm.cap = 0;
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
