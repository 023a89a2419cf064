// bai.hip — the BAM index of a coordinate-sorted stream the device has just written: elp_index_sorted_bgzf and elp_index_merged_bgzf make
// the .bai (SAM specification 5.2, in the canonical form include/elprep_hip.h states) of the members elp_emit_sorted_bgzf /
// elp_emit_merged_bgzf returned, from the context's columns and the members' sizes alone - nothing is inflated, no record is read back.
// The host walks the members' headers (bai_plan.hpp: bai_members), copies their offsets up and the finished index out; everything per
// record, per chunk and per contig, and the assembly of the bytes, is done here:
//   the emitters' size launch pass by pass with a 64-bit running base      -> where every output record starts and ends in the stream
//   k_bai_records      bin, last window, FLAG & 4 of every output record (through out_source: the merged stream needs its list only)
//   k_bai_contigs      the contigs' record ranges from adjacent refids (the stream is in coordinate order: a contig's records are one run)
//   radix_sort_pairs   (refid << 16 | bin, k): stable, so a bin's records stay in output order; the constant key bytes cost no pass
//   k_bai_heads        the first record of every bin and of every chunk, by an adjacent compare over the sorted list; two scans count them
//   k_bai_scan_*       the running maximum of refid << 15 | last window over the output order: within a contig the records' first windows
//                      do not decrease, so record k is the first to reach the windows in (maximum before it, maximum with it] and writes
//                      its start into exactly those - every window once, no atomics, and the windows nobody touches take the value to
//                      their right for free (a contig's first record writes from window 0 on)
//   k_bai_contig_sizes, the same scan as a sum     -> every contig's place in the index, and the index's size
//   k_bai_write_*      contigs (n_bin, pseudo-bin, n_intv, head and tail), bins and chunks, windows: 32-bit stores, every field is 4-aligned
// Sizes, offsets and the scratch layout are bai_plan.hpp's.
#include "common.hpp"
#include "bamout.hpp"
#include "bai_plan.hpp"

namespace elp {

// ---- the stream positions: pass j0 .. j0 + cnt of the size launch, `base` bytes in front of it
__global__ __launch_bounds__(256) void k_bai_place(uint32_t cnt, uint64_t k0, uint64_t base, const uint32_t *__restrict__ sizes, const uint32_t *__restrict__ offs,
                                                   uint64_t *__restrict__ start, uint32_t *__restrict__ size) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= cnt) return;
  start[k0 + j] = base + offs[j];
  size[k0 + j] = sizes[j];
  if (j + 1 == cnt) start[k0 + cnt] = base + offs[j] + sizes[j];  // (the next pass overwrites it with the same value; the last leaves the stream's length)
}

// ---- per output record: key = refid << 16 | bin (all ones: unplaced, or refused), gmax = refid << 15 | last window, unm = FLAG & 4
__global__ __launch_bounds__(256) void k_bai_records(BamOut m, BamOut m2, const uint32_t *__restrict__ src, uint64_t n_out, int32_t n_ref, uint64_t *__restrict__ key,
                                                     uint64_t *__restrict__ gmax, uint32_t *__restrict__ val, uint32_t *__restrict__ unm, BaiRes *__restrict__ res) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_out) return;
  uint32_t i;
  const BamOut &mm = out_source(m, m2, src, k, &i);
  const int32_t refid = mm.refid[i];
  uint64_t ky = ~0ull, g = 0;
  uint32_t u = 0, e = 0;
  if (refid >= n_ref) e = BAI_ERR_REFID;
  else if (refid >= 0) {
    const uint16_t f = mm.flag[i];
    const int64_t pos = mm.pos[i];
    const uint64_t beg = pos > 0 ? (uint64_t)(pos - 1) : 0;
    uint64_t span = 0;
    if (!(f & F_UNMAPPED)) {
      const uint64_t c0 = mm.cigar_off[i], c1 = mm.cigar_off[i + 1];
      for (uint64_t q = c0; q < c1; q++) {
        const uint32_t c = mm.cigar[q];
        if (op_consumes_ref(c & 0xF)) span += c >> 4;
      }
    }
    if (span == 0) span = 1;
    const uint64_t end = beg + span;
    if (end > BAI_MAX_END) e = BAI_ERR_END;
    else {
      ky = ((uint64_t)refid << 16) | reg2bin((int32_t)beg, (int32_t)(end - 1));
      g = ((uint64_t)refid << 15) | ((end - 1) >> BAI_WINDOW_SHIFT);
      u = (f & F_UNMAPPED) ? 1u : 0u;
    }
  }
  key[k] = ky;
  gmax[k] = g;
  val[k] = (uint32_t)k;
  unm[k] = u;
  if (e) atomicOr(&res->err, e);
}

// ---- the contigs' runs [first, end) among the output, and the count of placed records (they stand in front of the unplaced ones).
// A refid that descends, or a placed record behind an unplaced one, is BAI_ERR_ORDER: the windows' writes below rely on the order.
__global__ __launch_bounds__(256) void k_bai_contigs(uint64_t n_out, const uint64_t *__restrict__ key, uint32_t *__restrict__ first, uint32_t *__restrict__ end,
                                                     BaiRes *__restrict__ res) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_out) return;
  const uint64_t none = ~0ull >> 16;
  const uint64_t r = key[k] >> 16, rp = k ? key[k - 1] >> 16 : none;
  if (k == 0 || r != rp) {
    if (k && r < rp) atomicOr(&res->err, BAI_ERR_ORDER);
    if (r != none) first[r] = (uint32_t)k;
    else res->n_placed = (uint32_t)k;
    if (k && rp != none) end[rp] = (uint32_t)k;
  }
  if (k + 1 == n_out && r != none) { end[r] = (uint32_t)n_out; res->n_placed = (uint32_t)n_out; }
}

// ---- the sorted list (ks = refid << 16 | bin, vs = k), np placed records: heads of bins and chunks.  A record extends the chunk in
// front of it iff it starts in the member that chunk ends in (the members' offsets ascend: equal members = equal high parts of the
// virtual offsets).  Entry np of both arrays is 0: the scans over np + 1 entries leave the totals there.
__global__ __launch_bounds__(256) void k_bai_heads(uint64_t np, const uint64_t *__restrict__ ks, const uint32_t *__restrict__ vs, const uint64_t *__restrict__ start,
                                                   const uint32_t *__restrict__ size, uint32_t *__restrict__ head_bin, uint32_t *__restrict__ head_chunk) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j > np) return;
  uint32_t hb = 0, hc = 0;
  if (j < np) {
    hb = j == 0 || ks[j] != ks[j - 1];
    hc = hb;
    if (!hb) {
      const uint32_t kp = vs[j - 1];
      hc = start[vs[j]] / BGZF_PAYLOAD != (start[kp] + size[kp]) / BGZF_PAYLOAD;
    }
  }
  head_bin[j] = hb;
  head_chunk[j] = hc;
}
__global__ __launch_bounds__(256) void k_bai_bin_first(uint64_t np, const uint32_t *__restrict__ head_bin, const uint32_t *__restrict__ bins,
                                                       const uint32_t *__restrict__ chunks, uint32_t *__restrict__ bin_chunk0) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < np && head_bin[j]) bin_chunk0[bins[j]] = chunks[j];
}

// ---- 64-bit scans in three launches: a sum per tile, the tiles' sums scanned by one workgroup, the tiles scanned from their bases.
// MAX: the running maximum, inclusive, else the exclusive sum.  (exclusive_scan_u32, radix.hip, is the 32-bit sum.)
template <bool MAX>
__device__ __forceinline__ unsigned long long bai_op(unsigned long long a, unsigned long long b) { return MAX ? (a > b ? a : b) : a + b; }
// inclusive scan of one value per thread over the workgroup of 256; *total = the workgroup's (all threads)
template <bool MAX>
__device__ __forceinline__ unsigned long long bai_block_scan(unsigned long long v, unsigned long long *total, unsigned long long *lds /* 4 */) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long t = __shfl_up(v, d, 64);
    if (lane >= d) v = bai_op<MAX>(t, v);
  }
  __syncthreads();  // (lds may still be read from the call before)
  if (lane == 63) lds[w] = v;
  __syncthreads();
  unsigned long long base = 0, tot = 0;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const unsigned long long s = lds[q];
    if (q < w) base = bai_op<MAX>(base, s);
    tot = bai_op<MAX>(tot, s);
  }
  *total = tot;
  return bai_op<MAX>(base, v);
}
constexpr int BAI_SCAN_ITEMS = BAI_SCAN_TILE / 256;
template <bool MAX>
__global__ __launch_bounds__(256) void k_bai_scan_tiles(const uint64_t *__restrict__ in, uint64_t n, uint64_t *__restrict__ partials) {
  __shared__ unsigned long long lds[4];
  const uint64_t at = (uint64_t)blockIdx.x * BAI_SCAN_TILE + (uint64_t)threadIdx.x * BAI_SCAN_ITEMS;
  unsigned long long s = 0, tot;
  for (int q = 0; q < BAI_SCAN_ITEMS; q++)
    if (at + q < n) s = bai_op<MAX>(s, in[at + q]);
  (void)bai_block_scan<MAX>(s, &tot, lds);
  if (threadIdx.x == 0) partials[blockIdx.x] = tot;
}
// one workgroup: the tiles' sums become what stands in front of every tile; *total (may be null) = all of them
template <bool MAX>
__global__ __launch_bounds__(256) void k_bai_scan_partials(uint64_t *__restrict__ partials, uint64_t n_tiles, uint64_t *__restrict__ total) {
  __shared__ unsigned long long lds[4];
  unsigned long long carry = 0;
  for (uint64_t t0 = 0; t0 < n_tiles; t0 += 256) {  // (n_tiles is uniform: every thread takes every turn)
    const uint64_t t = t0 + threadIdx.x;
    const unsigned long long v = t < n_tiles ? partials[t] : 0ull;
    unsigned long long tot;
    const unsigned long long inc = bai_block_scan<MAX>(v, &tot, lds);
    // what stands in front of tile t: the carry and the tiles of this turn in front of it
    const unsigned long long left = __shfl_up(inc, 1, 64);
    __shared__ unsigned long long edge[4];
    if ((threadIdx.x & 63) == 63) edge[threadIdx.x >> 6] = inc;
    __syncthreads();
    unsigned long long before = (threadIdx.x & 63) ? left : (threadIdx.x ? edge[(threadIdx.x >> 6) - 1] : 0ull);
    if (t < n_tiles) partials[t] = threadIdx.x ? bai_op<MAX>(carry, before) : carry;
    carry = bai_op<MAX>(carry, tot);
    __syncthreads();
  }
  if (total && threadIdx.x == 0) *total = carry;
}
template <bool MAX>
__global__ __launch_bounds__(256) void k_bai_scan_apply(const uint64_t *in, uint64_t *out /* may be `in` */, uint64_t n, const uint64_t *__restrict__ partials) {
  __shared__ unsigned long long lds[4];
  const uint64_t at = (uint64_t)blockIdx.x * BAI_SCAN_TILE + (uint64_t)threadIdx.x * BAI_SCAN_ITEMS;
  unsigned long long v[BAI_SCAN_ITEMS], s = 0, tot;
  for (int q = 0; q < BAI_SCAN_ITEMS; q++) {
    v[q] = at + q < n ? in[at + q] : 0ull;
    s = bai_op<MAX>(s, v[q]);
  }
  const unsigned long long inc = bai_block_scan<MAX>(s, &tot, lds);
  // what stands in front of this thread's items: the tile's base and the threads in front (the inclusive value of the thread to the left)
  __shared__ unsigned long long incs[256];
  incs[threadIdx.x] = inc;
  __syncthreads();
  unsigned long long run = partials[blockIdx.x];
  if (threadIdx.x) run = bai_op<MAX>(run, incs[threadIdx.x - 1]);
  for (int q = 0; q < BAI_SCAN_ITEMS; q++) {
    if (at + q >= n) break;
    if (MAX) { run = bai_op<MAX>(run, v[q]); out[at + q] = run; }
    else { out[at + q] = run; run += v[q]; }
  }
}
template <bool MAX>
static int bai_scan(elp_ctx *c, const char *name, const uint64_t *in, uint64_t *out, uint64_t n, uint64_t *partials, uint64_t *total_dev) {
  if (n == 0) {
    if (total_dev) ELP_HIP(c, hipMemsetAsync(total_dev, 0, 8, c->stream));
    return 0;
  }
  const uint64_t n_tiles = (n + BAI_SCAN_TILE - 1) / BAI_SCAN_TILE;
  ELP_LAUNCH(c, name, k_bai_scan_tiles<MAX>, dim3((unsigned)n_tiles), dim3(256), 0, in, n, partials);
  ELP_LAUNCH(c, name, k_bai_scan_partials<MAX>, dim3(1), dim3(256), 0, partials, n_tiles, total_dev);
  ELP_LAUNCH(c, name, k_bai_scan_apply<MAX>, dim3((unsigned)n_tiles), dim3(256), 0, in, out, n, (const uint64_t *)partials);
  return 0;
}

// ---- what a contig's records amount to: read by the three kernels below from the run and the scans
struct BaiContig {
  uint32_t first, n, n_bins, n_chunks, n_intv, n_unm;
};
struct BaiCols {
  const uint32_t *first, *end, *bins, *chunks, *unms;
  const uint64_t *gmax;  // the running maximum
};
__device__ __forceinline__ BaiContig bai_contig(const BaiCols &t, uint64_t r) {
  BaiContig g;
  const uint32_t f = t.first[r], e = t.end[r];
  g.first = f;
  g.n = e - f;
  if (g.n == 0) { g.n_bins = g.n_chunks = g.n_intv = g.n_unm = 0; return g; }
  g.n_bins = t.bins[e] - t.bins[f];
  g.n_chunks = t.chunks[e] - t.chunks[f];
  g.n_unm = t.unms[e] - t.unms[f];
  g.n_intv = (uint32_t)(t.gmax[e - 1] & 0x7FFFu) + 1u;
  return g;
}
__global__ __launch_bounds__(256) void k_bai_contig_sizes(uint64_t n_ref, BaiCols t, uint64_t *__restrict__ bytes) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_ref) return;
  const BaiContig g = bai_contig(t, r);
  bytes[r] = bai_contig_bytes(g.n, g.n_bins, g.n_chunks, g.n_intv);
}

// ---- the bytes.  `out` in 32-bit words: every field of the index stands at a multiple of 4 (not of 8: 64-bit values go out as two words)
__device__ __forceinline__ void bai_put64(uint32_t *__restrict__ out, uint64_t byte_at, uint64_t v) {
  out[byte_at >> 2] = (uint32_t)v;
  out[(byte_at >> 2) + 1] = (uint32_t)(v >> 32);
}
struct BaiPlace {
  const uint64_t *start;  // n_out + 1 stream positions
  const uint32_t *size;
  const uint64_t *coff;   // n_members + 1
  uint64_t base_coffset;
};
__device__ __forceinline__ uint64_t bai_S(const BaiPlace &p, uint64_t k) { return bai_voff(p.base_coffset, p.coff, p.start[k]); }
__device__ __forceinline__ uint64_t bai_E(const BaiPlace &p, uint64_t k) { return bai_voff(p.base_coffset, p.coff, p.start[k] + p.size[k]); }

// head, tail, and per contig: n_bin, the pseudo-bin, n_intv
__global__ __launch_bounds__(256) void k_bai_write_contigs(uint64_t n_ref, BaiCols t, BaiPlace p, const uint64_t *__restrict__ offset, uint64_t contig_bytes,
                                                           uint64_t n_no_coor, uint32_t *__restrict__ out) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r == 0) {
    out[0] = 0x01494142u;  // "BAI\1"
    out[1] = (uint32_t)n_ref;
    bai_put64(out, BAI_HEAD_BYTES + contig_bytes, n_no_coor);
  }
  if (r >= n_ref) return;
  const BaiContig g = bai_contig(t, r);
  const uint64_t at = BAI_HEAD_BYTES + offset[r];
  if (g.n == 0) {
    out[at >> 2] = 0;
    out[(at >> 2) + 1] = 0;
    return;
  }
  out[at >> 2] = g.n_bins + 1;
  const uint64_t ps = at + bai_bin_at(g.n_bins, g.n_chunks);
  out[ps >> 2] = BAI_PSEUDO_BIN;
  out[(ps >> 2) + 1] = 2;
  bai_put64(out, ps + 8, bai_S(p, g.first));
  bai_put64(out, ps + 16, bai_E(p, (uint64_t)g.first + g.n - 1));
  bai_put64(out, ps + 24, g.n - g.n_unm);
  bai_put64(out, ps + 32, g.n_unm);
  out[(at + bai_intv_at(g.n_bins, g.n_chunks)) >> 2] = g.n_intv;
}
// bins and chunks: sorted entry j writes its bin's number if it is the bin's first, the bin's chunk count if its last, its chunk's
// beginning if the chunk's first, its end if the chunk's last
__global__ __launch_bounds__(256) void k_bai_write_bins(uint64_t np, const uint64_t *__restrict__ ks, const uint32_t *__restrict__ vs, const uint32_t *__restrict__ head_bin,
                                                        const uint32_t *__restrict__ head_chunk, const uint32_t *__restrict__ bin_chunk0, BaiCols t, BaiPlace p,
                                                        const uint64_t *__restrict__ offset, uint32_t *__restrict__ out) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= np) return;
  const uint32_t hb = head_bin[j], hc = head_chunk[j], tb = head_bin[j + 1] || j + 1 == np, tc = head_chunk[j + 1] || j + 1 == np;
  if (!(hb | hc | tb | tc)) return;
  const uint64_t r = ks[j] >> 16;
  const uint32_t f = t.first[r], k = vs[j];
  const uint64_t at = BAI_HEAD_BYTES + offset[r];
  const uint32_t bin_g = t.bins[j + 1] - 1, chunk_g = t.chunks[j + 1] - 1;  // this entry's bin and chunk among all
  const uint32_t bin_c = bin_g - t.bins[f], chunk_c = chunk_g - t.chunks[f], c0 = bin_chunk0[bin_g];  // ... among the contig's; the chunks in front of the bin
  const uint64_t b_at = at + bai_bin_at(bin_c, c0 - t.chunks[f]);
  if (hb) out[b_at >> 2] = (uint32_t)(ks[j] & 0xFFFFu);
  if (tb) out[(b_at >> 2) + 1] = chunk_g + 1 - c0;
  const uint64_t c_at = at + bai_chunk_at((uint64_t)bin_c + 1, chunk_c);
  if (hc) bai_put64(out, c_at, bai_S(p, k));
  if (tc) bai_put64(out, c_at + 8, bai_E(p, k));
}
// the linear index: output record k writes its start into the windows its last window is the first to reach (the scheme at the top)
__global__ __launch_bounds__(256) void k_bai_write_windows(uint64_t np, BaiCols t, BaiPlace p, const uint64_t *__restrict__ offset, uint32_t *__restrict__ out) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= np) return;
  const uint64_t g = t.gmax[k], r = g >> 15;
  const uint32_t hi = (uint32_t)(g & 0x7FFFu), f = t.first[r];
  const uint32_t lo = k > f ? (uint32_t)(t.gmax[k - 1] & 0x7FFFu) + 1u : 0u;
  if (lo > hi) return;
  const BaiContig c = bai_contig(t, r);
  const uint64_t w_at = BAI_HEAD_BYTES + offset[r] + bai_intv_at(c.n_bins, c.n_chunks) + 4;
  const uint64_t s = bai_S(p, k);
  for (uint32_t w = lo; w <= hi && w < c.n_intv; w++) bai_put64(out, w_at + 8ull * w, s);
}

// ---- the call, for the stream of n_out output records (m, m2, src: as emit_stream takes them)
static int index_stream(elp_ctx *c, const BamOut &m, const BamOut &m2, const uint32_t *src, uint64_t n_out, uint64_t max_raw_rec, const uint8_t *bgzf, uint64_t n_bytes,
                        uint64_t base_coffset, uint8_t *bai_out, uint64_t cap, uint64_t *n_bytes_out, const char *who) {
  hipStream_t st = c->stream;
  if (n_bytes && !bgzf) return set_error(c, ELP_ERR_ARG, "%s: no bytes", who);
  if (n_out >= 0xFFFFFFFEull) return set_error(c, ELP_ERR_UNSUPPORTED, "%s: more than 2^32 - 2 output records", who);
  const BaiMembers mem = bai_members(bgzf, n_bytes);
  if (mem.error) return set_error(c, ELP_ERR_DATA, "%s", mem.text(who).c_str());
  if (!bai_coffsets_fit(base_coffset, n_bytes)) return set_error(c, ELP_ERR_ARG, "%s: base_coffset + n_bytes does not fit the 48 bits of a virtual offset", who);
  const uint64_t n_ref = (uint64_t)std::max<int32_t>(c->n_ref, 0), n_mem = mem.n_members();
  const BaiScratch0 l0(n_out);
  const BaiScratch1 l1(n_out);
  const BaiScratch2 l2(n_ref, n_mem, n_out);
  uint64_t *w0, *w1, *w2;
  ELP_TRY(scratch(c, 0, l0.words64, &w0));
  ELP_TRY(scratch(c, 1, l1.words64, &w1));
  ELP_TRY(scratch(c, 2, l2.words64, &w2));
  uint64_t *start = w0 + l0.start, *key = w0 + l0.key, *gmax = w0 + l0.gmax;
  auto u32_at = [](uint64_t *w, size_t at) { return reinterpret_cast<uint32_t *>(w + at); };
  uint32_t *size = u32_at(w0, l0.size), *val = u32_at(w0, l0.val), *head_bin = u32_at(w0, l0.head_bin), *head_chunk = u32_at(w0, l0.head_chunk),
           *bins = u32_at(w0, l0.bins), *chunks = u32_at(w0, l0.chunks), *unm = u32_at(w0, l0.unm), *unms = u32_at(w0, l0.unms), *bin_chunk0 = u32_at(w0, l0.bin_chunk0);
  BaiRes *res = reinterpret_cast<BaiRes *>(w2 + l2.res);
  uint64_t *coff = w2 + l2.coff, *bytes = w2 + l2.bytes, *offset = w2 + l2.offset, *partials = w2 + l2.partials;
  uint32_t *first = u32_at(w2, l2.first), *end = u32_at(w2, l2.end);

  // where the records stand: the emitters' own sizes, pass by pass as emit_stream takes them
  ELP_HIP(c, hipMemsetAsync(start, 0, 8, st));
  const uint32_t CHUNK = emit_pass_records(emit_rec_bound(OutFormat::BGZF, max_raw_rec, 0), c->tune.emit_pass);
  uint64_t stream_bytes = 0;
  for (uint64_t k0 = 0; k0 < n_out; k0 += CHUNK) {
    const uint32_t cnt = (uint32_t)std::min<uint64_t>(CHUNK, n_out - k0);
    const EmitScratch4 lay(cnt);
    uint32_t *wk;
    ELP_TRY(scratch(c, 4, lay.words, &wk));
    uint32_t *sizes = wk + lay.sizes, *offs = wk + lay.offs, *err = wk + lay.err;
    ELP_HIP(c, hipMemsetAsync(err, 0, 4, st));
    ELP_TRY(bam_sizes_launch(c, m, m2, src, k0, cnt, sizes, err));
    uint32_t chunk_bytes = 0, he = 0;
    ELP_TRY(exclusive_scan_u32(c, sizes, offs, cnt, &chunk_bytes));
    ELP_LAUNCH(c, "bai_place", k_bai_place, dim3(blocks_for(cnt, 256)), dim3(256), 0, cnt, k0, stream_bytes, (const uint32_t *)sizes, (const uint32_t *)offs, start, size);
    ELP_HIP(c, hipMemcpyAsync(&he, err, 4, hipMemcpyDeviceToHost, st));
    ELP_HIP(c, elp::stream_wait(st));  // (the next pass may move slot 4)
    if (he & 16u) return set_error(c, ELP_ERR_UNSUPPORTED, "%s: H-typed optional field", who);
    if (he) return set_error(c, ELP_ERR_DATA, "%s: malformed optional fields", who);
    stream_bytes += chunk_bytes;
  }
  if (!bai_is_the_stream(mem, stream_bytes))
    return set_error(c, ELP_ERR_ARG, "%s: these bytes are not this context's stream (%llu bytes in %llu members, the stream has %llu)", who,
                     (unsigned long long)mem.inflated, (unsigned long long)n_mem, (unsigned long long)stream_bytes);

  // per record and per contig
  ELP_HIP(c, hipMemsetAsync(res, 0, sizeof(BaiRes), st));
  ELP_HIP(c, hipMemcpyAsync(coff, mem.coff.data(), (n_mem + 1) * 8, hipMemcpyHostToDevice, st));
  ELP_HIP(c, hipMemsetAsync(first, 0, (n_ref + 1) * 4, st));
  ELP_HIP(c, hipMemsetAsync(end, 0, (n_ref + 1) * 4, st));
  ELP_HIP(c, hipMemsetAsync(unm, 0, (n_out + 1) * 4, st));
  if (n_out) {
    ELP_LAUNCH(c, "bai_records", k_bai_records, dim3(blocks_for(n_out, 256)), dim3(256), 0, m, m2, src, n_out, (int32_t)n_ref, key, gmax, val, unm, res);
    ELP_LAUNCH(c, "bai_contigs", k_bai_contigs, dim3(blocks_for(n_out, 256)), dim3(256), 0, n_out, (const uint64_t *)key, first, end, res);
  }
  BaiRes h;
  ELP_HIP(c, hipMemcpyAsync(&h, res, sizeof h, hipMemcpyDeviceToHost, st));
  ELP_HIP(c, elp::stream_wait(st));
  if (h.err & BAI_ERR_REFID) return set_error(c, ELP_ERR_DATA, "%s: a record's refid is outside the dictionary", who);
  if (h.err & BAI_ERR_ORDER) return set_error(c, ELP_ERR_DATA, "%s: records are not in coordinate order", who);
  if (h.err & BAI_ERR_END) return set_error(c, ELP_ERR_UNSUPPORTED, "%s: a record ends beyond position 2^29, which a BAM index cannot hold", who);
  const uint64_t np = h.n_placed;
  if (np > n_out) return set_error(c, ELP_ERR_HIP, "%s: the count of placed records is off", who);

  // bins and chunks from the sorted list
  uint64_t *ks = key;
  uint32_t *vs = val;
  ELP_TRY(radix_sort_pairs(c, key, val, w1 + l1.key, u32_at(w1, l1.val), np, &ks, &vs));
  ELP_LAUNCH(c, "bai_heads", k_bai_heads, dim3(blocks_for(np + 1, 256)), dim3(256), 0, np, (const uint64_t *)ks, (const uint32_t *)vs, (const uint64_t *)start,
             (const uint32_t *)size, head_bin, head_chunk);
  ELP_TRY(exclusive_scan_u32(c, head_bin, bins, np + 1, nullptr));
  ELP_TRY(exclusive_scan_u32(c, head_chunk, chunks, np + 1, nullptr));
  ELP_TRY(exclusive_scan_u32(c, unm, unms, np + 1, nullptr));
  if (np) ELP_LAUNCH(c, "bai_bin_first", k_bai_bin_first, dim3(blocks_for(np, 256)), dim3(256), 0, np, (const uint32_t *)head_bin, (const uint32_t *)bins, (const uint32_t *)chunks, bin_chunk0);
  ELP_TRY(bai_scan<true>(c, "bai_window_scan", gmax, gmax, np, partials, nullptr));
  // every contig's size and place
  const BaiCols cols{first, end, bins, chunks, unms, gmax};
  if (n_ref) ELP_LAUNCH(c, "bai_contig_sizes", k_bai_contig_sizes, dim3(blocks_for(n_ref, 256)), dim3(256), 0, n_ref, cols, bytes);
  ELP_TRY(bai_scan<false>(c, "bai_contig_scan", bytes, offset, n_ref, partials, &res->contig_bytes));
  ELP_HIP(c, hipMemcpyAsync(&h, res, sizeof h, hipMemcpyDeviceToHost, st));
  ELP_HIP(c, elp::stream_wait(st));
  ELP_TRY(radix_check(c));
  const uint64_t total = bai_total_bytes(h.contig_bytes);
  if (!bai_out) { *n_bytes_out = total; return 0; }  // size query: exact
  if (cap < total) return set_error(c, ELP_ERR_ARG, "%s: output buffer too small (%llu bytes needed)", who, (unsigned long long)total);

  // the bytes
  uint32_t *d_bai;
  ELP_TRY(scratch(c, 3, (size_t)(total / 4) + 16, &d_bai));
  const BaiPlace place{start, size, coff, base_coffset};
  ELP_LAUNCH(c, "bai_write_contigs", k_bai_write_contigs, dim3(blocks_for(std::max<uint64_t>(n_ref, 1), 256)), dim3(256), 0, n_ref, cols, place, (const uint64_t *)offset,
             h.contig_bytes, n_out - np, d_bai);
  if (np) {
    ELP_LAUNCH(c, "bai_write_bins", k_bai_write_bins, dim3(blocks_for(np, 256)), dim3(256), 0, np, (const uint64_t *)ks, (const uint32_t *)vs, (const uint32_t *)head_bin,
               (const uint32_t *)head_chunk, (const uint32_t *)bin_chunk0, cols, place, (const uint64_t *)offset, d_bai);
    ELP_LAUNCH(c, "bai_write_windows", k_bai_write_windows, dim3(blocks_for(np, 256)), dim3(256), 0, np, cols, place, (const uint64_t *)offset, d_bai);
  }
  ELP_HIP(c, hipMemcpyAsync(bai_out, d_bai, total, hipMemcpyDeviceToHost, st));
  ELP_HIP(c, elp::stream_wait(st));
  *n_bytes_out = total;
  return 0;
}

}  // namespace elp

using namespace elp;

extern "C" {

int elp_index_sorted_bgzf(elp_ctx *c, const uint8_t *bgzf, uint64_t n_bytes, uint64_t base_coffset, uint8_t *bai_out, uint64_t cap, uint64_t *n_bytes_out) {
  const char *who = "elp_index_sorted_bgzf";
  if (!c || !n_bytes_out) return ELP_ERR_ARG;
  ELP_HIP(c, hipSetDevice(c->device));
  if (!c->derived.sorted) return set_error(c, ELP_ERR_ARG, "%s: call elp_sort_coordinate first (or elp_order_keep with by_split = 0 on coordinate-sorted input)", who);
  if (c->derived.sorted_qname) return set_error(c, ELP_ERR_ARG, "%s: the context holds a queryname permutation; a BAM index is of a coordinate-sorted stream", who);
  if (c->derived.sorted_keep_by_split)
    return set_error(c, ELP_ERR_ARG, "%s: the context holds a keep permutation ordered by split id; a BAM index is of a coordinate-sorted stream", who);
  ELP_TRY(radix_check(c));
  if (c->raw_n != c->n) return set_error(c, ELP_ERR_ARG, "%s: records were not staged with elp_stage_bam", who);
  const uint64_t n_out = c->n - c->n_sr;
  if (c->derived.sorted_keep) {
    uint64_t *keys;
    ELP_TRY(scratch(c, 5, n_out + 2, &keys));
    bool in_order = true;
    ELP_TRY(keep_coordinate_order(c, n_out, keys, reinterpret_cast<uint32_t *>(keys + n_out), &in_order));
    if (!in_order)
      return set_error(c, ELP_ERR_DATA, "%s: records are not in coordinate order ((refid, POS) must not decrease in a context that holds its input order, "
                       "elp_order_keep; sort it with elp_sort_coordinate instead)", who);
  }
  const BamOut m = bam_out_of(c);
  return index_stream(c, m, m, nullptr, n_out, c->max_raw_rec + emit_out_growth(c), bgzf, n_bytes, base_coffset, bai_out, cap, n_bytes_out, who);
}

int elp_index_merged_bgzf(elp_ctx *groups, elp_ctx *spread, const uint8_t *bgzf, uint64_t n_bytes, uint64_t base_coffset, uint8_t *bai_out, uint64_t cap,
                          uint64_t *n_bytes_out) {
  const char *who = "elp_index_merged_bgzf";
  if (!groups || !spread || groups == spread || !n_bytes_out) return ELP_ERR_ARG;
  BamOut mg, ms;
  const uint32_t *src = nullptr;
  uint64_t n_out = 0;
  ELP_TRY(emit_merged_list(groups, spread, who, &mg, &ms, &src, &n_out));
  return index_stream(groups, mg, ms, src, n_out, std::max(groups->max_raw_rec, spread->max_raw_rec) + emit_out_growth(groups), bgzf, n_bytes, base_coffset, bai_out, cap,
                      n_bytes_out, who);
}

}  // extern "C"
