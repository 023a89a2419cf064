// bqsr.hip — the host side of the BQSR gather on the HBM column store, and what it keeps on the device between calls.
//
// Reference: BaseRecalibrator.Recalibrate (filters/bqsr.go:467-551).
//
//   reference and known sites   elp_bqsr_set_reference / elp_bqsr_set_known_sites: contigs as 4-bit codes (k_pack_reference), known-site
//                               flags inside them (k_ref_mark_sites), a bucket index over the site lists (k_site_index); sync_bqsr_ptrs
//   gather_impl                 elp_bqsr_gather / elp_bqsr_gather_device: checks, the plan (bqsr_plan.hpp), scratch, the three prologue passes
//                               (bqsr_prologue.hip), then the one-length count kernel twice (count3.hip) or the general kernel's passes
//                               (bqsr_count.hip), the error word, and the retry with the exact quality set when the sampled hint missed one
//   the tables' way back        elp_bqsr_tables_fetch, elp_bqsr_tables_fetch_rows (k_tables_pack_rows), elp_bqsr_quals_counted
//   bqsr_error                  the device error word as the call's error, for this file and bqsr_apply.hip
// ApplyBQSR is in bqsr_apply.hip, bqsr_lut.hip, apply_flat.hip and apply3.hip.
#include <utility>

#include "bqsr_common.hpp"

namespace elp {

// reference contigs are kept as 4-bit code nibbles like the restaged SEQ column (ctx.hip k_recode_seq), first base in the LOW
// nibble: A 0, C 1, G 2, T 3, anything else 8 (baseToIntMap, bqsr.go:247-252: a/A/'*' -> A ...; a read base is only ever compared
// when it is A, C, G or T, so "other" needs no finer code).  Comparing 16 read bases with 16 reference bases is one 64-bit XOR.
__global__ __launch_bounds__(256) void k_pack_reference(const uint8_t *__restrict__ ascii, int64_t len, uint8_t *__restrict__ packed, int64_t packed_bytes) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= packed_bytes) return;
  uint32_t out = 0;
  for (int h = 0; h < 2; h++) {
    const int64_t j = 2 * i + h;
    uint32_t code = 8;  // past the contig: "other"
    if (j < len) {
      switch (ascii[j]) {
        case 'a': case 'A': case '*': code = 0; break;
        case 'c': case 'C': code = 1; break;
        case 'g': case 'G': code = 2; break;
        case 't': case 'T': code = 3; break;
        default: code = 8;
      }
    }
    out |= code << (4 * h);
  }
  packed[i] = (uint8_t)out;
}
// idx[b] = first site whose End is >= 64 b (sites are sorted and flattened, so Ends increase with the index)
// Known sites inside the packed reference: bit 2 of the nibble of every base that lies in a site interval (the base codes use bits 0, 1
// and 3; nib_code_differs ignores bit 2).  A read whose clipped copy is ONE run of matches then has its known-site bits in the
// reference window the count kernel loads anyway (count3.hip): no walk over the site list and no skip-column bits for it.
__global__ __launch_bounds__(256) void k_ref_clear_site_flags(uint32_t *__restrict__ packed_words, int64_t n_words) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_words) packed_words[i] &= 0xBBBBBBBBu;
}
__global__ __launch_bounds__(256) void k_ref_mark_sites(const int32_t *__restrict__ sv, int64_t ns, int64_t cap_bases, uint32_t *__restrict__ packed_words) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= ns) return;
  int64_t lo = (int64_t)sv[2 * s] - 1, hi = (int64_t)sv[2 * s + 1] - 1;  // 0-based, inclusive
  lo = lo < 0 ? 0 : lo;
  hi = hi >= cap_bases ? cap_bases - 1 : hi;  // (bases behind the contig's end are "other" codes inside the allocation: flags there are harmless and exact)
  for (int64_t j = lo; j <= hi;) {  // word by word (8 bases)
    const int64_t w = j >> 3;
    int64_t last = (w << 3) + 7;
    last = last > hi ? hi : last;
    const int a = (int)(j & 7), b = (int)(last & 7);
    const uint32_t m = (0x44444444u >> (4 * (7 - b))) & (0x44444444u << (4 * a));
    atomicOr(&packed_words[w], m);
    j = last + 1;
  }
}

__global__ __launch_bounds__(256) void k_site_index(const int32_t *__restrict__ sv, int64_t ns, int64_t nbuck, uint32_t *__restrict__ idx) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= nbuck) return;
  const int64_t x = b << 6;
  int64_t lo = 0, hi = ns;
  while (lo < hi) { const int64_t md = lo + (hi - lo) / 2; if (sv[2 * md + 1] < x) lo = md + 1; else hi = md; }
  idx[b] = (uint32_t)lo;
}

int bqsr_error(elp_ctx *c, uint32_t e) {
  ELP_HIP(c, hipMemsetAsync(c->err_flag.p, 0, 4, c->stream));
  if (e & 2u) return set_error(c, ELP_ERR_UNSUPPORTED, "BQSR: read longer than %d bases", MAX_DESC_READ);
  if (e & 4u) return set_error(c, ELP_ERR_DATA, "reference coordinate matches a non-existing base in read (reference: log.Panicf, filters/utils.go:253,262)");
  if (e & 8u) return set_error(c, ELP_ERR_DATA, "BQSR: base quality above 93");
  if (e & 16u) return set_error(c, ELP_ERR_DATA, "cycle value exceeds maximum cycle value (reference: log.Panic, filters/bqsr.go:364-369)");
  if (e & 32u) return set_error(c, ELP_ERR_DATA, "BQSR requires input with read groups (reference: log.Panic, filters/bqsr.go:38)");
  if (e & 64u) return set_error(c, ELP_ERR_DATA, "ApplyBQSR: len(QUAL) != len(SEQ) (reference: index out of range panic)");
  if (e & 256u) return set_error(c, ELP_ERR_HIP, "radix sort: tile look-back timed out");
  if (e & 1024u) return set_error(c, ELP_ERR_HIP, "BQSR prologue: a read without known-site bits took a record form that needs them (internal)");
  return set_error(c, ELP_ERR_DATA, "BQSR: device error word %u", e);
}

static int sync_bqsr_ptrs(elp_ctx *c) {
  if (!c->bqsr_ptrs_dirty) return 0;
  const size_t nr = (size_t)c->n_ref;
  // known-site flags of the packed contigs whose reference or site list changed (either order of the two setters)
  for (size_t r = 0; r < nr; r++) {
    if (!c->ref_flags_dirty[r] || !c->h_ref_seq[r]) continue;
    const int64_t len = c->h_ref_seq_len[r], n_words = ((len + 1) / 2 + REF_PAD) / 4;
    uint32_t *pw = reinterpret_cast<uint32_t *>(c->h_ref_seq[r]);
    hipLaunchKernelGGL(k_ref_clear_site_flags, dim3(blocks_for((uint64_t)std::max<int64_t>(n_words, 1), 256)), dim3(256), 0, c->stream, pw, n_words);
    if (c->h_sites[r] && c->h_n_sites[r] > 0)
      hipLaunchKernelGGL(k_ref_mark_sites, dim3(blocks_for((uint64_t)c->h_n_sites[r], 256)), dim3(256), 0, c->stream, (const int32_t *)c->h_sites[r], c->h_n_sites[r], n_words * 8, pw);
    ELP_HIP(c, hipGetLastError());
    c->ref_flags_dirty[r] = 0;
  }
  ELP_TRY(ensure(c, c->d_ref_seq, nr + 1));
  ELP_TRY(ensure(c, c->d_ref_seq_len, nr + 1));
  ELP_TRY(ensure(c, c->d_sites, nr + 1));
  ELP_TRY(ensure(c, c->d_n_sites, nr + 1));
  ELP_TRY(ensure(c, c->d_site_idx, nr + 1));
  if (nr) {
    ELP_HIP(c, hipMemcpyAsync(c->d_ref_seq.p, c->h_ref_seq.data(), nr * sizeof(uint8_t *), hipMemcpyHostToDevice, c->stream));
    ELP_HIP(c, hipMemcpyAsync(c->d_ref_seq_len.p, c->h_ref_seq_len.data(), nr * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    ELP_HIP(c, hipMemcpyAsync(c->d_sites.p, c->h_sites.data(), nr * sizeof(int32_t *), hipMemcpyHostToDevice, c->stream));
    ELP_HIP(c, hipMemcpyAsync(c->d_n_sites.p, c->h_n_sites.data(), nr * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    ELP_HIP(c, hipMemcpyAsync(c->d_site_idx.p, c->h_site_idx.data(), nr * sizeof(uint32_t *), hipMemcpyHostToDevice, c->stream));
    ELP_HIP(c, elp::stream_wait(c->stream));
  }
  c->bqsr_ptrs_dirty = false;
  return 0;
}

// dev_tables were just written on c->stream: the event the table fetches on the copy stream wait for
int tables_written(elp_ctx *c) {
  if (!c->tables_ev) ELP_HIP(c, hipEventCreateWithFlags(&c->tables_ev, hipEventDisableTiming));
  ELP_HIP(c, hipEventRecord(c->tables_ev, c->stream));
  return 0;
}

// ---- the tables' and the LUT's rows form (round 5): with many read groups the dense tables / LUT are tens of megabytes of which only the
// rows of the qualities that occur hold anything; only those rows cross PCIe.
// packs the rows of `quals` (slot k = quality quals[k]) of the three dense tables behind each other: q [n_cov][nq][2] | c [n_cov][nq][ncyc][2]
// | x [n_cov][nq][16][2]; flags a row with observations whose quality is not among them (the caller then fetches the dense tables)
__global__ __launch_bounds__(256) void k_tables_pack_rows(const unsigned long long *__restrict__ tb, int n_cov, int ncyc, const uint8_t *__restrict__ quals, int nq,
                                                          unsigned long long *__restrict__ out, uint32_t *uncovered) {
  const size_t row_w = 2 + (size_t)ncyc * 2 + ELP_NCTX * 2;  // words of one (covariate, quality) row over the three tables
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x, n_rows = (size_t)n_cov * (size_t)nq;
  if (k < (size_t)n_cov * ELP_NQUAL) {  // (the first n_cov * 94 threads also check the qualities that were not asked for)
    const int q = (int)(k % ELP_NQUAL);
    bool asked = false;
    for (int j = 0; j < nq; j++) asked |= quals[j] == q;
    if (!asked && tb[2 * k] != 0) atomicOr(uncovered, 1u);
  }
  if (k >= n_rows * row_w) return;
  const size_t r = k / row_w, w = k - r * row_w;
  const size_t cv = r / (size_t)nq, q = quals[r % (size_t)nq], src_row = cv * ELP_NQUAL + q;
  const size_t nq_all = (size_t)n_cov * ELP_NQUAL * 2, nc_all = nq_all * (size_t)ncyc;
  const size_t oq = 0, oc = n_rows * 2, ox = oc + n_rows * (size_t)ncyc * 2;
  if (w < 2) out[oq + r * 2 + w] = tb[src_row * 2 + w];
  else if (w < 2 + (size_t)ncyc * 2) out[oc + r * (size_t)ncyc * 2 + (w - 2)] = tb[nq_all + src_row * (size_t)ncyc * 2 + (w - 2)];
  else out[ox + r * ELP_NCTX * 2 + (w - 2 - (size_t)ncyc * 2)] = tb[nq_all + nc_all + src_row * ELP_NCTX * 2 + (w - 2 - (size_t)ncyc * 2)];
}

// quality values to give table slots (>= 6, <= 93): the context's hint, or the exact set after a retry
static std::vector<int> quality_slots(const elp_ctx *c) {
  std::vector<int> quals;
  for (int q = 6; q < ELP_NQUAL; q++)
    if ((q < 64 ? (c->qual_present[0] >> q) : (c->qual_present[1] >> (q - 64))) & 1ull) quals.push_back(q);
  if (quals.empty()) quals.push_back(6);
  return quals;
}

// The record area of the one-length kernel in `mode` (0: none - descriptors are written) and where the prologue passes put records:
// class-1 segments | the other region | (mode 2) the other region sorted by covariate; the counters and the segments' first slots
static int rec_buffers(elp_ctx *c, const GatherScratch &S, uint32_t *block, int mode, uint32_t ncs, RecOut *ro) {
  const uint32_t nseg = mode == 2 ? std::max<uint32_t>((uint32_t)C3_NSEG, ncs) : (uint32_t)C3_NSEG;  // (ncs <= 256: n_cov <= 255)
  BqRec *recs = nullptr;
  if (mode) ELP_TRY(scratch(c, 4, S.rec_slots(mode), &recs));
  *ro = RecOut{recs, block + S.rec_cnt, block + S.seg_base, S.other_at(mode), nseg, mode == 2 ? ncs : 0u};
  if (mode) ELP_TRY(c3_segments_launch(c, S, block, nseg, ro->ncs));
  return 0;
}

// the one-length kernel over the records the prologues left: launch 1: the reads that are one run of matches, in the class-1 segments;
// launch 2: the others (indels, clipped windows, descriptors) - one segment, or (covariate split) one per covariate
static int count_one_length(elp_ctx *c, const GatherShape &g, const GatherScratch &S, const PrologueBufs &b, const RecOut &ro, const std::vector<int> &quals,
                            unsigned long long *cycle_tbl, unsigned long long *ctx_tbl) {
  const bool split = ro.ncs != 0;
  int rsw3 = 0, rlog3 = 0;
  size_t dyn3 = 0;
  (void)count3_plan(split ? 1 : g.n_cov, (int)quals.size(), g.lmax, g.lds_count3, &rsw3, &rlog3, &dyn3, g.count3_rlog);
  QMap qm;
  memset(qm.slot, 254, sizeof qm.slot);
  for (size_t s = 0; s < quals.size(); s++) qm.slot[quals[s]] = (uint8_t)s;
  const uint4 *other = reinterpret_cast<const uint4 *>(ro.recs) + 2 * (size_t)ro.other_at;  // the other region (32-byte records)
  const uint32_t *n_other = ro.cnt + (size_t)ro.nseg * C3_CSTRIDE;
  uint32_t *cw = b.block + S.cw, *ooff = cw + CO_MAXCOV;
  ELP_HIP(c, hipMemsetAsync(cw, 0, (3 * CO_MAXCOV + 1) * sizeof(uint32_t), c->stream));
  if (split) {
    // the other region sorted by covariate (behind it), counts and offsets per covariate
    uint4 *sorted = const_cast<uint4 *>(other) + 2 * (size_t)c->n;
    ELP_TRY(c3_other_sort_launch(c, other, n_other, cw, sorted));
    other = sorted;
  }
  Count3Args A3{ro.cnt, (uint32_t)C3_CSTRIDE, ro.seg_base, reinterpret_cast<const uint4 *>(ro.recs), ro.nseg, 0, (int)ro.ncs, c->uniform_len, c->qual.p,
                c->seq4.p + elp_ctx::SEQ_FRONT, reinterpret_cast<const uint8_t *>(b.skipbits), reinterpret_cast<const uint4 *>(b.desc), c->cigar.p, b.cs_pool,
                c->d_ref_seq.p, c->d_ref_seq_len.p, g.n_cov, (int)quals.size(), g.lmax, g.max_cycle, rsw3, rlog3, cycle_tbl, ctx_tbl, c->err_flag.p};
  ELP_TRY(count3_launch(c, A3, qm, dyn3));
  // (without the split the one segment's first slot is the zero in front of the offsets: ooff[0], cleared above)
  A3.other = 1;
  A3.srecs = other;
  A3.seg_base = ooff;
  A3.cnt_stride = 1;
  if (split) { A3.seg_cnt = cw; A3.nseg = ro.ncs; }
  else { A3.seg_cnt = n_other; A3.nseg = 1; }
  return count3_launch(c, A3, qm, dyn3);
}

// the general kernel over the descriptors: the plan's passes over covariate subsets and quality subsets
static int count_general(elp_ctx *c, const GatherShape &g, const CountPlan &p, const PrologueBufs &b, const std::vector<int> &quals,
                         unsigned long long *cycle_tbl, unsigned long long *ctx_tbl) {
  for (int cov0 = 0; cov0 < g.n_cov; cov0 += p.ncp)
    for (size_t q0 = 0; q0 < quals.size(); q0 += (size_t)p.qcap) {
      const int nqs = (int)std::min<size_t>((size_t)p.qcap, quals.size() - q0), ncov_pass = std::min(p.ncp, g.n_cov - cov0);
      QMap qm;
      memset(qm.slot, 254, sizeof qm.slot);
      for (int q : quals) qm.slot[q] = 255;
      for (int s = 0; s < nqs; s++) qm.slot[quals[q0 + s]] = (uint8_t)s;
      CountArgs A{c->n, c->qual_bytes, c->qual_off.p, c->seq_off.p, c->qual.p, c->seq4.p, b.desc, c->cigar.p, b.cs_pool,
                  reinterpret_cast<const uint8_t *>(b.skipbits), c->d_ref_seq.p, c->d_ref_seq_len.p, c->n_ref, ncov_pass, nqs, g.lmax, p.rs, g.max_cycle,
                  cycle_tbl, ctx_tbl, c->err_flag.p, c->tile_first.p, cov0};
      ELP_TRY(count_general_launch(c, A, qm, p, p.dyn(ncov_pass, nqs)));
    }
  return 0;
}

// one pinned copy of the three tables (they lie behind each other on the device), then into the caller's arrays
static int tables_to_host(elp_ctx *c, size_t nq, size_t nc, size_t nx, int64_t *qual_tbl, int64_t *cycle_tbl, int64_t *ctx_tbl) {
  const size_t bytes = (nq + nc + nx) * 8;
  if (bytes > c->h_pinned_cap) {
    if (c->h_pinned) (void)hipHostFree(c->h_pinned);
    c->h_pinned = nullptr; c->h_pinned_cap = 0;
    ELP_HIP(c, hipHostMalloc(&c->h_pinned, bytes, hipHostMallocDefault));
    c->h_pinned_cap = bytes;
  }
  ELP_HIP(c, hipMemcpyAsync(c->h_pinned, c->dev_tables.p, bytes, hipMemcpyDeviceToHost, c->stream));
  uint32_t e[4];
  ELP_TRY(fetch_err(c, e));
  if (e[0]) return bqsr_error(c, e[0]);
  const int64_t *hp = static_cast<const int64_t *>(c->h_pinned);
  memcpy(qual_tbl, hp, nq * 8);
  memcpy(cycle_tbl, hp + nq, nc * 8);
  memcpy(ctx_tbl, hp + nq + nc, nx * 8);
  return 0;
}

// builds the three tables in c->dev_tables; qual_tbl != nullptr: also copies them to the host
static int gather_impl(elp_ctx *c, int max_cycle, int64_t *qual_tbl, int64_t *cycle_tbl, int64_t *ctx_tbl) {
  for (int r = 0; r < c->n_ref; r++)
    if (!c->h_ref_seq[r]) return set_error(c, ELP_ERR_ARG, "elp_bqsr_gather: no reference sequence set for refid %d", r);
  for (int r = 0; r < c->n_ref; r++)
    if (!c->h_sites[r]) ELP_TRY(elp_bqsr_set_known_sites(c, r, nullptr, 0));
  ELP_TRY(sync_bqsr_ptrs(c));
  ELP_TRY(ensure_adapted(c, false));  // low-quality-tail bounds per read (adapt_score)
  ELP_TRY(ensure_flat_index(c));
  ELP_TRY(ensure_qual_present(c));  // sizing hint: the set of quality values seen in a sample of the column
  if (c->n_cov > 255) return set_error(c, ELP_ERR_UNSUPPORTED, "more than 255 read-group covariates");
  if (c->cigar_ops + 4 * c->n >= 0x7FFFFFFFull) return set_error(c, ELP_ERR_UNSUPPORTED, "CIGAR pool exceeds 2^31 operations per context");
  const int ncyc_g = 2 * max_cycle + 1;
  const size_t nq = (size_t)c->n_cov * ELP_NQUAL * 2, nc = nq * ncyc_g, nx = nq * ELP_NCTX;
  c->tables_n = 0;
  ELP_TRY(ensure(c, c->dev_tables, nq + nc + nx + elp_ctx::TABLES_TAIL));
  unsigned long long *tb = c->dev_tables.p;
  hipStream_t st = c->stream;
  ELP_HIP(c, hipMemsetAsync(tb, 0, (nq + nc + nx) * sizeof(unsigned long long), st));
  const uint64_t n = c->n;
  if (n && c->qual_bytes) {
    const GatherScratch S(n);
    PrologueBufs b;
    ELP_TRY(scratch(c, 1, 2 * (c->cigar_ops + 4 * n) + 64, &b.cs_pool));
    ELP_TRY(scratch(c, 2, n + 4, &b.desc));
    ELP_TRY(scratch(c, 0, 4 * n + 8, &b.plain_rec));
    const size_t skip_words = (size_t)((c->qual_bytes + 31) / 32 + 8);
    ELP_TRY(scratch(c, 3, skip_words, &b.skipbits));
    ELP_TRY(ensure_uniform_len(c));
    ELP_TRY(scratch(c, 5, S.words, &b.block));
    ELP_HIP(c, hipMemsetAsync(b.block, 0, 16, st));  // the two lists' counts
    // the plan (bqsr_plan.hpp): count3.hip works from 32-byte records the prologue kernels write instead of the descriptors
    const GatherShape g{c->n_cov, (int)std::max<uint32_t>(c->max_l_seq, 1), max_cycle, c->uniform_len, c->tune.count_kernel, c->tune.count3_rlog,
                        COUNT3_STATIC_LDS, COUNT_STATIC_LDS, COUNT_STATIC_LDS_1024};
    uint32_t ncs = 1;  // the covariate split's segments per group
    while ((int)ncs < c->n_cov) ncs <<= 1;
    int mode = c3_mode(g, (int)quality_slots(c).size());
    if (S.too_many()) return set_error(c, ELP_ERR_UNSUPPORTED, "BQSR: more than ~1.4 G records per context");
    RecOut ro;
    ELP_TRY(rec_buffers(c, S, b.block, mode, ncs, &ro));
    if (!ro.recs) ELP_HIP(c, hipMemsetAsync(b.skipbits, 0, skip_words * 4, st));  // (with records the reads that use the column clear their own bits: clear_skip_bits)
    ELP_TRY(prologue_launch(c, b, S, ro));
    if (g.lmax > MAX_DESC_READ) return set_error(c, ELP_ERR_UNSUPPORTED, "BQSR: read longer than %d bases", MAX_DESC_READ);
    for (int attempt = 0;; attempt++) {
      const std::vector<int> quals = quality_slots(c);
      const CountPlan p = count_general_plan(g, (int)quals.size());
      if (!p.fits) return set_error(c, ELP_ERR_UNSUPPORTED, "BQSR: one covariate's private table rows do not fit in LDS (max read length=%d)", g.lmax);
      // the sampled hint chose a form of the one-length kernel; the exact set (taken after the count met a quality without a slot) may
      // need another one - the covariate split, or the general kernel with its several passes: the reference just runs
      // (filters/bqsr.go:467-551), so does this - the prologues once more, leaving what the new form reads
      const int mode2 = ro.recs ? c3_mode(g, (int)quals.size()) : mode;
      if (mode2 != mode) {
        mode = mode2;
        ELP_TRY(rec_buffers(c, S, b.block, mode, ncs, &ro));
        ELP_HIP(c, hipMemsetAsync(b.skipbits, 0, skip_words * 4, st));
        ELP_HIP(c, hipMemsetAsync(b.block, 0, 16, st));
        ELP_TRY(prologue_launch(c, b, S, ro));
      }
      if (ro.recs) ELP_TRY(count_one_length(c, g, S, b, ro, quals, tb + nq, tb + nq + nc));
      else ELP_TRY(count_general(c, g, p, b, quals, tb + nq, tb + nq + nc));
      uint32_t e[4];
      ELP_TRY(fetch_err(c, e));
      if ((e[0] & ~128u) != 0) return bqsr_error(c, e[0] & ~128u);
      if (!(e[0] & 128u)) break;
      // a counted base had a quality the sampled hint did not contain: take the exact set (full scan) and redo the count
      ELP_HIP(c, hipMemsetAsync(c->err_flag.p, 0, 4, st));
      c->derived.qual_hint_refuted();
      ELP_TRY(ensure_qual_present(c, true));
      if (attempt >= 2) return set_error(c, ELP_ERR_HIP, "BQSR: quality-slot retry did not converge");
      ELP_HIP(c, hipMemsetAsync(tb, 0, (nq + nc + nx) * sizeof(unsigned long long), st));
    }
    ELP_TRY(qual_from_cycle_launch(c, ncyc_g, tb + nq, tb));
  }
  c->tables_n = nq + nc + nx;
  c->tables_max_cycle = max_cycle;
  c->tables_quals[0] = c->qual_present[0] & ~0x3Full;  // (qualities below 6 are never counted)
  c->tables_quals[1] = c->qual_present[1];
  ELP_TRY(tables_written(c));
  if (!qual_tbl) return 0;  // tables stay in HBM (the count loop above fetched the error word behind the last kernel that can raise one)
  return tables_to_host(c, nq, nc, nx, qual_tbl, cycle_tbl, ctx_tbl);
}

}  // namespace elp

using namespace elp;

extern "C" {

int elp_bqsr_set_reference(elp_ctx *c, int32_t refid, const uint8_t *bases, int64_t len) {
  if (!c || !c->have_header || refid < 0 || refid >= c->n_ref || len < 0 || (len && !bases)) return set_error(c, ELP_ERR_ARG, "elp_bqsr_set_reference: bad arguments");
  ELP_HIP(c, hipSetDevice(c->device));
  if (c->h_ref_seq[refid]) { (void)elp::stream_wait(c->stream); (void)hipFree(c->h_ref_seq[refid]); c->h_ref_seq[refid] = nullptr; }
  // the contig is kept as 4-bit base codes (k_pack_reference); the ASCII bytes only pass through scratch
  const int64_t packed = (len + 1) / 2;
  uint8_t *d = nullptr;
  ELP_HIP(c, hipMalloc((void **)&d, (size_t)(packed + REF_PAD)));
  ELP_HIP(c, hipMemsetAsync(d, 0x88, (size_t)(packed + REF_PAD), c->stream));
  if (len) {
    uint8_t *tmp;
    ELP_TRY(scratch(c, 7, (size_t)len + 16, &tmp));
    ELP_HIP(c, hipMemcpyAsync(tmp, bases, (size_t)len, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_pack_reference, dim3(blocks_for((uint64_t)packed, 256)), dim3(256), 0, c->stream, (const uint8_t *)tmp, len, d, packed);
    ELP_HIP(c, hipGetLastError());
  }
  ELP_HIP(c, elp::stream_wait(c->stream));
  c->h_ref_seq[refid] = d;
  c->h_ref_seq_len[refid] = len;
  c->ref_flags_dirty[refid] = 1;
  c->bqsr_ptrs_dirty = true;
  return 0;
}

int elp_bqsr_set_known_sites(elp_ctx *c, int32_t refid, const int32_t *start_end, int64_t n) {
  if (!c || !c->have_header || refid < 0 || refid >= c->n_ref || n < 0 || (n && !start_end)) return set_error(c, ELP_ERR_ARG, "elp_bqsr_set_known_sites: bad arguments");
  for (int64_t k = 1; k < n; k++)
    if (!(start_end[2 * k] > start_end[2 * k - 1])) return set_error(c, ELP_ERR_ARG, "known sites of refid %d are not sorted and flattened at index %lld", refid, (long long)k);
  ELP_HIP(c, hipSetDevice(c->device));
  if (c->h_sites[refid]) { (void)elp::stream_wait(c->stream); (void)hipFree(c->h_sites[refid]); c->h_sites[refid] = nullptr; }
  if (c->h_site_idx[refid]) { (void)hipFree(c->h_site_idx[refid]); c->h_site_idx[refid] = nullptr; }
  int32_t *d = nullptr;
  ELP_HIP(c, hipMalloc((void **)&d, (size_t)(2 * n + 4) * sizeof(int32_t)));
  if (n) ELP_HIP(c, hipMemcpyAsync(d, start_end, (size_t)(2 * n) * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
  const int64_t nbuck = ((int64_t)c->h_ref_len[refid] >> 6) + 1;
  uint32_t *ix = nullptr;
  ELP_HIP(c, hipMalloc((void **)&ix, (size_t)(nbuck + 4) * sizeof(uint32_t)));
  hipLaunchKernelGGL(k_site_index, dim3(blocks_for((uint64_t)nbuck, 256)), dim3(256), 0, c->stream, (const int32_t *)d, n, nbuck, ix);
  ELP_HIP(c, hipGetLastError());
  ELP_HIP(c, elp::stream_wait(c->stream));
  c->h_site_idx[refid] = ix;
  c->h_sites[refid] = d;
  c->h_n_sites[refid] = n;
  c->ref_flags_dirty[refid] = 1;
  c->bqsr_ptrs_dirty = true;
  return 0;
}

int elp_bqsr_gather(elp_ctx *c, int max_cycle, int64_t *qual_tbl, int64_t *cycle_tbl, int64_t *ctx_tbl) {
  if (!c || !qual_tbl || !cycle_tbl || !ctx_tbl || max_cycle < 1) return set_error(c, ELP_ERR_ARG, "elp_bqsr_gather: bad arguments");
  ELP_HIP(c, hipSetDevice(c->device));
  return gather_impl(c, max_cycle, qual_tbl, cycle_tbl, ctx_tbl);
}

int elp_bqsr_gather_device(elp_ctx *c, int max_cycle) {
  if (!c || max_cycle < 1) return set_error(c, ELP_ERR_ARG, "elp_bqsr_gather_device: bad arguments");
  ELP_HIP(c, hipSetDevice(c->device));
  return gather_impl(c, max_cycle, nullptr, nullptr, nullptr);
}

int elp_bqsr_tables_fetch(elp_ctx *c, int64_t *qual_tbl, int64_t *cycle_tbl, int64_t *ctx_tbl) {
  if (!c || !qual_tbl || !cycle_tbl || !ctx_tbl) return ELP_ERR_ARG;
  if (!c->tables_n) return set_error(c, ELP_ERR_ARG, "elp_bqsr_tables_fetch: no device tables (elp_bqsr_gather_device)");
  ELP_HIP(c, hipSetDevice(c->device));
  const size_t nq = (size_t)c->n_cov * ELP_NQUAL * 2, nc = nq * (size_t)(2 * c->tables_max_cycle + 1), nx = nq * ELP_NCTX;
  const size_t bytes = (nq + nc + nx) * 8;
  if (bytes > c->h_pinned_cap) {
    if (c->h_pinned) (void)hipHostFree(c->h_pinned);
    c->h_pinned = nullptr; c->h_pinned_cap = 0;
    ELP_HIP(c, hipHostMalloc(&c->h_pinned, bytes, hipHostMallocDefault));
    c->h_pinned_cap = bytes;
  }
  // on the copy stream, behind the last writer of the tables: a host thread can fetch (and finalise) while another one runs the
  // next stage on the context's stream (the copy is 6 MB over PCIe: ~0.2 ms during which the GPU would otherwise sit idle)
  if (!c->copy_stream) ELP_HIP(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
  if (c->tables_ev) ELP_HIP(c, hipStreamWaitEvent(c->copy_stream, c->tables_ev, 0));
  else ELP_HIP(c, elp::stream_wait(c->stream));
  ELP_HIP(c, hipMemcpyAsync(c->h_pinned, c->dev_tables.p, bytes, hipMemcpyDeviceToHost, c->copy_stream));
  ELP_HIP(c, elp::stream_wait(c->copy_stream));
  const int64_t *hp = static_cast<const int64_t *>(c->h_pinned);
  memcpy(qual_tbl, hp, nq * 8);
  memcpy(cycle_tbl, hp + nq, nc * 8);
  memcpy(ctx_tbl, hp + nq + nc, nx * 8);
  return 0;
}

// the qualities that had table slots in the gather that made the device tables: bit q of bits[q / 64]
int elp_bqsr_quals_counted(elp_ctx *c, uint64_t *bits) {
  if (!c || !bits) return ELP_ERR_ARG;
  if (!c->tables_n) return set_error(c, ELP_ERR_ARG, "elp_bqsr_quals_counted: no device tables (elp_bqsr_gather_device)");
  bits[0] = c->tables_quals[0];
  bits[1] = c->tables_quals[1];
  return 0;
}

// elp_bqsr_tables_fetch for the rows of the qualities `quals` only: q_rows [n_cov][n_quals][2], c_rows [n_cov][n_quals][2*max_cycle+1][2],
// x_rows [n_cov][n_quals][16][2] - packed on the device, one copy.  Returns 1 (and copies nothing) if a quality that was not asked for has
// observations (tables that were summed with another context's or rank's: the caller fetches the dense tables then).
int elp_bqsr_tables_fetch_rows(elp_ctx *c, const uint8_t *quals, int n_quals, int64_t *q_rows, int64_t *c_rows, int64_t *x_rows) {
  if (!c || n_quals < 0 || n_quals > ELP_NQUAL || (n_quals && (!quals || !q_rows || !c_rows || !x_rows))) return ELP_ERR_ARG;
  if (!c->tables_n) return set_error(c, ELP_ERR_ARG, "elp_bqsr_tables_fetch_rows: no device tables (elp_bqsr_gather_device)");
  for (int k = 0; k < n_quals; k++)
    if (quals[k] >= ELP_NQUAL) return set_error(c, ELP_ERR_ARG, "elp_bqsr_tables_fetch_rows: quality %d", (int)quals[k]);
  ELP_HIP(c, hipSetDevice(c->device));
  const int ncyc = 2 * c->tables_max_cycle + 1;
  const size_t n_rows = (size_t)c->n_cov * (size_t)n_quals, row_w = 2 + (size_t)ncyc * 2 + ELP_NCTX * 2, words = n_rows * row_w;
  const size_t bytes = words * 8 + 256;
  if (bytes > c->h_pinned_cap) {
    if (c->h_pinned) (void)hipHostFree(c->h_pinned);
    c->h_pinned = nullptr; c->h_pinned_cap = 0;
    ELP_HIP(c, hipHostMalloc(&c->h_pinned, bytes, hipHostMallocDefault));
    c->h_pinned_cap = bytes;
  }
  ELP_TRY(ensure(c, c->tables_pack, words + 64));
  if (!c->copy_stream) ELP_HIP(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
  if (c->tables_ev) ELP_HIP(c, hipStreamWaitEvent(c->copy_stream, c->tables_ev, 0));
  else ELP_HIP(c, elp::stream_wait(c->stream));
  // the quality list and the "uncovered" word ride in the pack buffer's tail
  uint8_t *d_quals = reinterpret_cast<uint8_t *>(c->tables_pack.p + words);
  uint32_t *d_unc = reinterpret_cast<uint32_t *>(c->tables_pack.p + words + 16);
  uint8_t *hq = static_cast<uint8_t *>(c->h_pinned) + words * 8;
  memset(hq, 0, 256);
  if (n_quals) memcpy(hq, quals, (size_t)n_quals);
  ELP_HIP(c, hipMemcpyAsync(d_quals, hq, 128 + 8, hipMemcpyHostToDevice, c->copy_stream));  // (also clears the word)
  const size_t work = std::max(words, (size_t)c->n_cov * ELP_NQUAL);
  hipLaunchKernelGGL(k_tables_pack_rows, dim3(blocks_for(work, 256)), dim3(256), 0, c->copy_stream, (const unsigned long long *)c->dev_tables.p, c->n_cov, ncyc,
                     (const uint8_t *)d_quals, n_quals, c->tables_pack.p, d_unc);
  ELP_HIP(c, hipGetLastError());
  ELP_HIP(c, hipMemcpyAsync(c->h_pinned, c->tables_pack.p, words * 8, hipMemcpyDeviceToHost, c->copy_stream));
  uint32_t unc = 0;
  ELP_HIP(c, hipMemcpyAsync(&unc, d_unc, 4, hipMemcpyDeviceToHost, c->copy_stream));
  ELP_HIP(c, elp::stream_wait(c->copy_stream));
  if (unc) return 1;
  const int64_t *hp = static_cast<const int64_t *>(c->h_pinned);
  if (n_rows) {
    memcpy(q_rows, hp, n_rows * 2 * 8);
    memcpy(c_rows, hp + n_rows * 2, n_rows * (size_t)ncyc * 2 * 8);
    memcpy(x_rows, hp + n_rows * 2 + n_rows * (size_t)ncyc * 2, n_rows * ELP_NCTX * 2 * 8);
  }
  return 0;
}

}  // extern "C"
