// sw.hip — the HaplotypeCaller's Smith-Waterman on the device: elp_sw_align and elp_sw_align_reads (runSmithWaterman, filters/sw.go:110-316;
// its call sites: filters/realign.go:310, filters/assemble-reads.go:1042,1152, filters/sw.go:401).  A batch is two pools of sequences and
// index pairs; every result is bit-equal to the reference's: all of its arithmetic is int32, and the limits of include/elprep_hip.h
// keep every one of them from wrapping.  The algorithm is sw_core.hpp's, sizes and layouts are sw_plan.hpp's; here are the kernels:
//   k_sw_shortcut   (softclip, ignore) a wave per problem looks for the LAST place at which the raw alternate stands in the normalised
//                   reference (lastIndex, :96-108), 64 candidate offsets at a time from the right; a hit is the whole answer
//   k_sw_dp         a wave per problem that missed: the systolic sweep over the tiles of the alternate, the end search, the traceback
//                   64 diagonal cells at a time, the strategy's tail - raw operations, their cleaned-up count and the alignment offset
//   k_sw_write      a thread per problem: the clean-up loop once more, now storing, behind an exclusive scan of the counts
//   k_sw_read_lens, k_sw_decode   (elp_sw_align_reads) the alternates from the SEQ of staged BAM records
// The host lists the problems that missed (one read-back of n words), cuts the list into chunks under the scratch budget and runs
// DP, scan and write chunk by chunk in problem order, a running base between them.
#include "common.hpp"
#include "sw_core.hpp"
#include "sw_plan.hpp"

namespace elp {

struct SwDev {  // a batch in HBM
  const uint8_t *a, *b;
  const uint64_t *a_off, *b_off;
  const uint32_t *ref_of, *alt_of;
};

// ---- the exact-substring shortcut, four problems per workgroup
__global__ __launch_bounds__(256) void k_sw_shortcut(SwDev d, uint64_t n, uint32_t *__restrict__ miss, uint32_t *__restrict__ n_ops, int32_t *__restrict__ offset) {
  const uint64_t k = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (k >= n) return;  // (the whole wave)
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t r0 = d.a_off[d.ref_of[k]], q0 = d.b_off[d.alt_of[k]];
  const uint32_t m = (uint32_t)(d.a_off[d.ref_of[k] + 1] - r0), len = (uint32_t)(d.b_off[d.alt_of[k] + 1] - q0);
  int32_t found = -1;
  for (int32_t top = (int32_t)m - (int32_t)len; top >= 0 && found < 0; top -= 64) {  // (wave-uniform)
    const int32_t r = top - (int32_t)lane;
    const bool hit = r >= 0 && sw_occurs_at(d.a + r0, d.b + q0, len, (uint32_t)r);
    const unsigned long long mask = __ballot(hit);
    if (mask) found = top - (int32_t)__builtin_ctzll(mask);  // the lowest lane holds the largest offset
  }
  if (lane == 0) {
    miss[k] = found < 0;
    n_ops[k] = found < 0 ? 0u : 1u;
    offset[k] = found < 0 ? 0 : found;
  }
}

// ---- the DP.  from_left: lane l receives lane l - 1's value (lane 0 its own, which it replaces)
__device__ __forceinline__ int32_t from_left(int32_t v) { return __shfl_up(v, 1, 64); }

__global__ __launch_bounds__(64) void k_sw_dp(SwDev d, SwParams p, const SwProb *__restrict__ probs, uint64_t first, int16_t *__restrict__ bt_all,
                                              uint32_t *__restrict__ raw_all, int32_t *__restrict__ edge_all, uint32_t *__restrict__ n_ops,
                                              int32_t *__restrict__ offset) {
  __shared__ uint8_t s_ref[SW_MAX_LEN + 1];
  const SwProb pr = probs[first + blockIdx.x];
  const uint32_t lane = threadIdx.x;
  const uint64_t r0 = d.a_off[d.ref_of[pr.k]], q0 = d.b_off[d.alt_of[pr.k]];
  const uint32_t m = (uint32_t)(d.a_off[d.ref_of[pr.k] + 1] - r0), n = (uint32_t)(d.b_off[d.alt_of[pr.k] + 1] - q0);
  if (m == 0 || n == 0 || m > SW_MAX_LEN || n > SW_MAX_LEN) return;  // (refused by the host; the whole workgroup)
  const uint8_t *__restrict__ alt = d.b + q0;
  for (uint32_t i = lane; i < m; i += 64) s_ref[i] = d.a[r0 + i];
  __syncthreads();
  int16_t *__restrict__ bt = bt_all + pr.bt_at;
  int32_t *edge = edge_all + pr.edge_at;  // 3 words per row, used where n > SW_TILE
  uint32_t *__restrict__ raw = raw_all + pr.raw_at;
  const uint32_t raw_cap = m + n + 3;

  SwColumnBest col;
  int64_t bottom = SW_NO_KEY;
  const uint32_t nt = sw_tiles(n);
  for (uint32_t q = 0; q < nt; q++) {
    const uint32_t width = n - q * SW_TILE < SW_TILE ? n - q * SW_TILE : SW_TILE, L = (width + SW_COLS - 1) / SW_COLS;
    const uint32_t j0 = q * SW_TILE + lane * SW_COLS;
    uint32_t bases = 0;
    for (uint32_t c = 0; c < SW_COLS; c++)
      if (j0 + c < n) bases |= (uint32_t)alt[j0 + c] << (8 * c);
    SwLane s;
    sw_lane_init(p, s, j0, bases);
    const bool owns_last = q + 1 == nt && lane == (width - 1) / SW_COLS;
    const uint32_t c_last = (width - 1) % SW_COLS;
    const bool writes_edge = q + 1 < nt && lane == 63;
    int16_t *__restrict__ bt_tile = bt + (uint64_t)q * sw_full_tile_cells(m);
    SwLeft out{0, 0, 0};
    // lane 0's input of the next step, fetched one step ahead: the first column, or the edge the tile before wrote
    SwLeft ahead = q == 0 ? sw_first_column(p, 1) : SwLeft{edge[0], edge[1], edge[2]};
    uint8_t a_ahead = s_ref[0];  // this lane's reference byte of the next row it computes
    const uint32_t steps = m + L - 1;
    for (uint32_t t = 0; t < steps; t++) {
      SwLeft in{from_left(out.cur), from_left(out.gap), from_left(out.size)};
      const int32_t i = (int32_t)t - (int32_t)lane + 1;  // this lane's row
      if (lane == 0) {
        in = ahead;
        if (t + 1 < m) ahead = q == 0 ? sw_first_column(p, t + 2) : SwLeft{edge[3 * (t + 1)], edge[3 * (t + 1) + 1], edge[3 * (t + 1) + 2]};
      }
      if (lane < L && i >= 1 && i <= (int32_t)m) {
        const uint8_t a_base = a_ahead;
        if ((uint32_t)i < m) a_ahead = s_ref[i];
        int16_t b4[SW_COLS];
        out = sw_strip_row(p, s, a_base, in, b4);
        short4 v;
        v.x = b4[0]; v.y = b4[1]; v.z = b4[2]; v.w = b4[3];
        *reinterpret_cast<short4 *>(bt_tile + ((uint64_t)t * L + lane) * SW_COLS) = v;
        if (writes_edge) {
          edge[3 * (i - 1)] = out.cur;
          edge[3 * (i - 1) + 1] = out.gap;
          edge[3 * (i - 1) + 2] = out.size;
        }
        if (owns_last)  // (no runtime index into the lane's registers)
          sw_column_step(col, c_last == 0 ? s.last[0] : c_last == 1 ? s.last[1] : c_last == 2 ? s.last[2] : s.last[3], (uint32_t)i);
        if ((uint32_t)i == m) {
          for (uint32_t c = 0; c < SW_COLS; c++)
            if (j0 + c < n) {
              const int64_t key = sw_bottom_key(s.last[c], m, j0 + c + 1);
              bottom = key > bottom ? key : bottom;
            }
        }
      }
    }
    __syncthreads();  // the edge and the backtrack cells are read by other lanes than wrote them
  }

  // the end search: the last column's choice from its owner, the bottom row's largest key over the lanes
  const uint32_t owner = ((n - 1) % SW_TILE) / SW_COLS;
  col.score = __shfl(col.score, owner, 64);
  col.p1 = __shfl(col.p1, owner, 64);
  for (int w = 32; w >= 1; w >>= 1) {
    const int64_t o = __shfl_xor(bottom, w, 64);
    bottom = o > bottom ? o : bottom;
  }
  // the traceback, the same in every lane; lane 0 stores.  Each turn fetches the 64 cells (p1 - k, p2 - k) and jumps to the first
  // that is not 0.  p1 + p2 falls in every turn, and the bound holds whatever the scratch contains.
  uint32_t *store = lane == 0 ? raw : nullptr;
  const uint32_t cap = lane == 0 ? raw_cap : 0;
  SwTrace t = sw_trace_begin(p, m, n, col, bottom, store, cap);
  for (uint32_t turns = 0; turns < m + n + 2; turns++) {
    if (t.p1 < 1 || t.p2 < 1 || t.p1 > (int32_t)m || t.p2 > (int32_t)n) break;
    const int32_t lim = t.p1 < t.p2 ? t.p1 : t.p2;
    int32_t v = 1;
    if ((int32_t)lane < lim) v = bt[sw_bt_index(m, n, (uint32_t)t.p1 - lane, (uint32_t)t.p2 - lane)];
    const unsigned long long mask = __ballot(v != 0);
    const int32_t run = mask ? (int32_t)__builtin_ctzll(mask) : 64;
    if (run > 0) sw_trace_diagonal(t, run, store, cap);
    else sw_trace_gap(t, __shfl(v, 0, 64), store, cap);
    if (sw_trace_done(t)) break;
  }
  sw_trace_end(p, t, store, cap);
  if (lane == 0) {
    const uint32_t n_raw = t.n_raw < raw_cap ? t.n_raw : raw_cap;
    n_ops[pr.k] = sw_clean(raw, n_raw, SwCountOnly{});
    offset[pr.k] = t.offset;
    raw[raw_cap] = n_raw;  // behind the list, for k_sw_write (sw_need counts the word)
  }
}

// ---- the results in their places: problems k0 .. k1, `base` operations in front of them, scan[k] those of k0 .. k
__global__ __launch_bounds__(256) void k_sw_write(SwDev d, uint64_t k0, uint64_t k1, uint64_t base, const uint32_t *__restrict__ miss, const uint32_t *__restrict__ scan,
                                                  const uint32_t *__restrict__ slot /* per problem: its entry of probs, where miss */, const SwProb *__restrict__ probs,
                                                  const uint32_t *__restrict__ raw_all, uint32_t *__restrict__ cigar, uint64_t cigar_cap, uint64_t *__restrict__ cigar_off) {
  const uint64_t k = k0 + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= k1) return;
  const uint64_t at = base + scan[k];
  cigar_off[k] = at;
  const uint32_t n = (uint32_t)(d.b_off[d.alt_of[k] + 1] - d.b_off[d.alt_of[k]]);
  if (!miss[k]) {
    if (at < cigar_cap) cigar[at] = (n << 4) | SW_OP_M;
    return;
  }
  const uint32_t m = (uint32_t)(d.a_off[d.ref_of[k] + 1] - d.a_off[d.ref_of[k]]);
  const SwProb pr = probs[slot[k]];
  const uint32_t *raw = raw_all + pr.raw_at, raw_cap = m + n + 3;
  const uint32_t n_raw = raw[raw_cap] < raw_cap ? raw[raw_cap] : raw_cap;
  if (n_raw) (void)sw_clean(raw, n_raw, SwStore{cigar, at, cigar_cap});
}

// ---- elp_sw_align_reads: the alternates from staged BAM records (block_size, 32 fixed bytes, name, CIGAR, SEQ: SAM specification 4.2)
__global__ __launch_bounds__(256) void k_sw_read_lens(uint64_t n, const uint32_t *__restrict__ read_idx, const uint32_t *__restrict__ l_seq, uint32_t *__restrict__ lens) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) lens[k] = l_seq[read_idx[k]];
}
__global__ __launch_bounds__(64) void k_sw_decode(const uint32_t *__restrict__ read_idx, const uint8_t *__restrict__ rawrec, const uint64_t *__restrict__ raw_off,
                                                  const uint64_t *__restrict__ b_off, uint8_t *__restrict__ b) {
  const uint64_t k = blockIdx.x;
  const uint32_t i = read_idx[k];
  const uint8_t *rec = rawrec + raw_off[i];
  const uint32_t l_name = rec[12], n_cigar = (uint32_t)rec[16] | ((uint32_t)rec[17] << 8);
  const uint8_t *seq = rec + 36 + l_name + 4 * n_cigar;
  const uint64_t at = b_off[k];
  const uint32_t len = (uint32_t)(b_off[k + 1] - at);  // the l_seq column's value, checked by the host
  for (uint32_t x = threadIdx.x; x < len; x += 64) {
    const uint32_t nib = (seq[x >> 1] >> ((x & 1) ? 0 : 4)) & 15u;
    b[at + x] = (uint8_t)"=ACMGRSVTWYHKDBN"[nib];
  }
}

// ---- the call behind both entry points: the batch is in HBM, its lengths are on the host and checked
static int sw_run(elp_ctx *c, const char *who, const SwDev &d, uint64_t n, const uint32_t *len_ref, const uint32_t *len_alt, uint64_t ops_bound, const SwParams &p,
                  uint32_t *cigar_out, uint64_t cigar_cap, uint64_t *cigar_off_out, int32_t *offset_out, uint64_t *n_ops_out) {
  hipStream_t st = c->stream;
  const bool shortcut = p.strategy == SW_SOFTCLIP || p.strategy == SW_IGNORE;
  // per problem; the descriptors' place is sized for every problem (who misses is known after the first kernel)
  const SwPerProblem lay(n, n);
  uint8_t *w1;
  ELP_TRY(scratch(c, 1, lay.bytes, &w1));
  uint32_t *miss = reinterpret_cast<uint32_t *>(w1 + lay.miss), *n_ops = reinterpret_cast<uint32_t *>(w1 + lay.n_ops), *scan = reinterpret_cast<uint32_t *>(w1 + lay.scan);
  int32_t *offset = reinterpret_cast<int32_t *>(w1 + lay.offset);
  uint64_t *cigar_off = reinterpret_cast<uint64_t *>(w1 + lay.cigar_off);
  SwProb *probs = reinterpret_cast<SwProb *>(w1 + lay.probs);
  const uint64_t dev_cap = std::min(cigar_cap, ops_bound);
  uint32_t *cigar;
  ELP_TRY(scratch(c, 3, dev_cap + 2, &cigar));

  ELP_HIP(c, hipMemsetAsync(n_ops, 0, 4 * (n + 1), st));
  ELP_HIP(c, hipMemsetAsync(offset, 0, 4 * n, st));
  std::vector<uint32_t> h_miss(n, 1u);
  if (shortcut) {
    ELP_LAUNCH(c, "sw_shortcut", k_sw_shortcut, dim3(blocks_for(n, 4)), dim3(256), 0, d, n, miss, n_ops, offset);
    ELP_HIP(c, hipMemcpyAsync(h_miss.data(), miss, 4 * n, hipMemcpyDeviceToHost, st));
    ELP_HIP(c, elp::stream_wait(st));
  } else {
    ELP_HIP(c, hipMemcpyAsync(miss, h_miss.data(), 4 * n, hipMemcpyHostToDevice, st));
  }
  // the list, its chunks, and for every problem that missed its entry of the list (slot 5)
  std::vector<SwProb> list;
  std::vector<uint32_t> h_slot(n, 0u);
  for (uint64_t k = 0; k < n; k++)
    if (h_miss[k]) {
      h_slot[k] = (uint32_t)list.size();
      list.push_back(SwProb{(uint32_t)k, 0, 0, 0, 0});
    }
  const uint64_t budget = c->tune.sw_scratch_bytes > 0 ? (uint64_t)c->tune.sw_scratch_bytes : SW_SCRATCH_DEFAULT;
  const std::vector<SwChunkCut> cuts = sw_chunks(list, len_ref, len_alt, budget);
  uint32_t *slot;
  ELP_TRY(scratch(c, 5, n + 2, &slot));
  ELP_HIP(c, hipMemcpyAsync(slot, h_slot.data(), 4 * n, hipMemcpyHostToDevice, st));
  if (!list.empty()) ELP_HIP(c, hipMemcpyAsync(probs, list.data(), sizeof(SwProb) * list.size(), hipMemcpyHostToDevice, st));
  ELP_HIP(c, elp::stream_wait(st));  // (the vectors above are pageable: their copies are done before they go)

  uint64_t base = 0, k0 = 0;
  const size_t n_chunks = std::max<size_t>(cuts.size(), 1);
  for (size_t ci = 0; ci < n_chunks; ci++) {
    uint64_t k1 = n;
    if (!cuts.empty()) {
      const SwChunkCut &cut = cuts[ci];
      const SwChunk ch(cut);
      uint8_t *w2;
      ELP_TRY(scratch(c, 2, ch.bytes + 16, &w2));
      ELP_LAUNCH(c, "sw_dp", k_sw_dp, dim3((unsigned)(cut.end - cut.first)), dim3(64), 0, d, p, (const SwProb *)probs, cut.first, reinterpret_cast<int16_t *>(w2 + ch.bt_at),
                 reinterpret_cast<uint32_t *>(w2 + ch.raw_at), reinterpret_cast<int32_t *>(w2 + ch.edge_at), n_ops, offset);
      if (ci + 1 < cuts.size()) k1 = list[cuts[ci + 1].first].k;  // the problems in front of the next chunk's first are this chunk's
      uint32_t total = 0;
      ELP_TRY(exclusive_scan_u32(c, n_ops + k0, scan + k0, k1 - k0, &total));
      ELP_LAUNCH(c, "sw_write", k_sw_write, dim3(blocks_for(k1 - k0, 256)), dim3(256), 0, d, k0, k1, base, (const uint32_t *)miss, (const uint32_t *)scan,
                 (const uint32_t *)slot, (const SwProb *)probs, (const uint32_t *)reinterpret_cast<uint32_t *>(w2 + ch.raw_at), cigar, dev_cap, cigar_off);
      base += total;
    } else {
      uint32_t total = 0;
      ELP_TRY(exclusive_scan_u32(c, n_ops, scan, n, &total));
      ELP_LAUNCH(c, "sw_write", k_sw_write, dim3(blocks_for(n, 256)), dim3(256), 0, d, (uint64_t)0, n, (uint64_t)0, (const uint32_t *)miss, (const uint32_t *)scan,
                 (const uint32_t *)slot, (const SwProb *)probs, (const uint32_t *)nullptr, cigar, dev_cap, cigar_off);
      base = total;
    }
    k0 = k1;
  }
  ELP_HIP(c, elp::stream_wait(st));
  *n_ops_out = base;
  if (base > cigar_cap)
    return set_error(c, ELP_ERR_ARG, "%s: cigar_cap is %llu operations, the results have %llu", who, (unsigned long long)cigar_cap, (unsigned long long)base);
  ELP_HIP(c, hipMemcpyAsync(cigar_off_out, cigar_off, 8 * n, hipMemcpyDeviceToHost, st));
  ELP_HIP(c, hipMemcpyAsync(offset_out, offset, 4 * n, hipMemcpyDeviceToHost, st));
  if (base) ELP_HIP(c, hipMemcpyAsync(cigar_out, cigar, 4 * base, hipMemcpyDeviceToHost, st));
  ELP_HIP(c, elp::stream_wait(st));
  cigar_off_out[n] = base;
  return 0;
}

static int sw_refused(elp_ctx *c, const char *who, const SwCheck &r) {
  return set_error(c, r.code == SW_REFUSE_UNSUPPORTED ? ELP_ERR_UNSUPPORTED : ELP_ERR_ARG, "%s: %s", who, r.text.c_str());
}

}  // namespace elp

using namespace elp;

extern "C" {

int elp_sw_align(elp_ctx *c, uint64_t n_a, const uint8_t *a, const uint64_t *a_off, uint64_t n_b, const uint8_t *b, const uint64_t *b_off, uint64_t n, const uint32_t *ref_of,
                 const uint32_t *alt_of, int32_t match, int32_t mismatch, int32_t gap_open, int32_t gap_extend, int strategy, uint32_t *cigar_out, uint64_t cigar_cap,
                 uint64_t *cigar_off_out, int32_t *offset_out, uint64_t *n_ops_out) {
  const char *who = "elp_sw_align";
  if (!c) return ELP_ERR_ARG;
  if (!cigar_off_out || !n_ops_out || (n && !offset_out) || (cigar_cap && !cigar_out)) return set_error(c, ELP_ERR_ARG, "%s: an output pointer is NULL", who);
  *n_ops_out = 0;
  SwCheck r = sw_check_params(match, mismatch, gap_open, gap_extend, strategy);
  if (r.code) return sw_refused(c, who, r);
  std::vector<uint32_t> len_ref(n), len_alt(n);
  r = sw_check_batch(n_a, a_off, n_b, b_off, n, ref_of, alt_of, len_ref.data(), len_alt.data());
  if (r.code) return sw_refused(c, who, r);
  if (n == 0) { cigar_off_out[0] = 0; return 0; }
  if (!a || !b) return set_error(c, ELP_ERR_ARG, "%s: a pool is NULL", who);
  ELP_HIP(c, hipSetDevice(c->device));
  hipStream_t st = c->stream;
  const SwInputs la(a_off[n_a], n_a, n), lb(b_off[n_b], n_b, 0);
  uint8_t *w0, *w4;
  ELP_TRY(scratch(c, 0, la.bytes, &w0));
  ELP_TRY(scratch(c, 4, lb.bytes, &w4));
  ELP_HIP(c, hipMemcpyAsync(w0 + la.seq, a, a_off[n_a], hipMemcpyHostToDevice, st));
  ELP_HIP(c, hipMemcpyAsync(w0 + la.off, a_off, 8 * (n_a + 1), hipMemcpyHostToDevice, st));
  ELP_HIP(c, hipMemcpyAsync(w0 + la.idx0, ref_of, 4 * n, hipMemcpyHostToDevice, st));
  ELP_HIP(c, hipMemcpyAsync(w0 + la.idx1, alt_of, 4 * n, hipMemcpyHostToDevice, st));
  ELP_HIP(c, hipMemcpyAsync(w4 + lb.seq, b, b_off[n_b], hipMemcpyHostToDevice, st));
  ELP_HIP(c, hipMemcpyAsync(w4 + lb.off, b_off, 8 * (n_b + 1), hipMemcpyHostToDevice, st));
  const SwDev d{w0 + la.seq, w4 + lb.seq, reinterpret_cast<const uint64_t *>(w0 + la.off), reinterpret_cast<const uint64_t *>(w4 + lb.off),
                reinterpret_cast<const uint32_t *>(w0 + la.idx0), reinterpret_cast<const uint32_t *>(w0 + la.idx1)};
  return sw_run(c, who, d, n, len_ref.data(), len_alt.data(), r.ops_bound, SwParams{match, mismatch, gap_open, gap_extend, strategy}, cigar_out, cigar_cap, cigar_off_out,
                offset_out, n_ops_out);
}

int elp_sw_align_reads(elp_ctx *c, uint64_t n_a, const uint8_t *a, const uint64_t *a_off, uint64_t n, const uint32_t *ref_of, const uint32_t *read_idx, int32_t match,
                       int32_t mismatch, int32_t gap_open, int32_t gap_extend, int strategy, uint32_t *cigar_out, uint64_t cigar_cap, uint64_t *cigar_off_out,
                       int32_t *offset_out, uint64_t *n_ops_out) {
  const char *who = "elp_sw_align_reads";
  if (!c) return ELP_ERR_ARG;
  if (!cigar_off_out || !n_ops_out || (n && !offset_out) || (cigar_cap && !cigar_out)) return set_error(c, ELP_ERR_ARG, "%s: an output pointer is NULL", who);
  *n_ops_out = 0;
  SwCheck r = sw_check_params(match, mismatch, gap_open, gap_extend, strategy);
  if (r.code) return sw_refused(c, who, r);
  if (n >= SW_MAX_PROBLEMS) return set_error(c, ELP_ERR_UNSUPPORTED, "%s: more than 2^31 - 1 problems", who);
  r = sw_check_pool("a", n_a, a_off);
  if (r.code) return sw_refused(c, who, r);
  if (n && (!ref_of || !read_idx)) return set_error(c, ELP_ERR_ARG, "%s: an index array is NULL", who);
  for (uint64_t k = 0; k < n; k++) {
    if (ref_of[k] >= n_a) return set_error(c, ELP_ERR_ARG, "%s: ref_of[%llu] = %u is outside the reference pool", who, (unsigned long long)k, ref_of[k]);
    if (read_idx[k] >= c->n) return set_error(c, ELP_ERR_ARG, "%s: read_idx[%llu] = %u is not a staged record (%llu staged)", who, (unsigned long long)k, read_idx[k], (unsigned long long)c->n);
  }
  if (n == 0) { cigar_off_out[0] = 0; return 0; }
  if (!a) return set_error(c, ELP_ERR_ARG, "%s: the reference pool is NULL", who);
  // the SEQ column keeps A, C, G, T and "other" (ctx.hip: k_recode_seq); the bases as the reference's strings hold them are in the BAM records
  if (c->raw_n != c->n)
    return set_error(c, ELP_ERR_ARG, "%s: records were not staged with elp_stage_bam, elp_stage_bgzf or elp_stage_sam (the SEQ column of column staging keeps A, C, G, T only)", who);
  ELP_HIP(c, hipSetDevice(c->device));
  hipStream_t st = c->stream;
  const SwInputs la(a_off[n_a], n_a, n);
  uint8_t *w0;
  ELP_TRY(scratch(c, 0, la.bytes, &w0));
  ELP_HIP(c, hipMemcpyAsync(w0 + la.seq, a, a_off[n_a], hipMemcpyHostToDevice, st));
  ELP_HIP(c, hipMemcpyAsync(w0 + la.off, a_off, 8 * (n_a + 1), hipMemcpyHostToDevice, st));
  ELP_HIP(c, hipMemcpyAsync(w0 + la.idx0, ref_of, 4 * n, hipMemcpyHostToDevice, st));
  ELP_HIP(c, hipMemcpyAsync(w0 + la.idx2, read_idx, 4 * n, hipMemcpyHostToDevice, st));
  const uint32_t *d_read_idx = reinterpret_cast<const uint32_t *>(w0 + la.idx2);
  uint32_t *d_lens;
  ELP_TRY(scratch(c, 1, n + 2, &d_lens));
  ELP_LAUNCH(c, "sw_read_lens", k_sw_read_lens, dim3(blocks_for(n, 256)), dim3(256), 0, n, d_read_idx, (const uint32_t *)c->l_seq.p, d_lens);
  std::vector<uint32_t> len_ref(n), len_alt(n), iota(n);
  ELP_HIP(c, hipMemcpyAsync(len_alt.data(), d_lens, 4 * n, hipMemcpyDeviceToHost, st));
  ELP_HIP(c, elp::stream_wait(st));
  std::vector<uint64_t> b_off(n + 1, 0);
  uint64_t bound = 0;
  for (uint64_t k = 0; k < n; k++) {
    const uint64_t m = a_off[ref_of[k] + 1] - a_off[ref_of[k]];
    r = sw_check_length(k, m, true);
    if (!r.code) r = sw_check_length(k, len_alt[k], false);
    if (r.code) return sw_refused(c, who, r);
    len_ref[k] = (uint32_t)m;
    iota[k] = (uint32_t)k;
    b_off[k + 1] = b_off[k] + len_alt[k];
    bound += m + len_alt[k] + 2;
  }
  const SwInputs lb(b_off[n], n, 0);
  uint8_t *w4;
  ELP_TRY(scratch(c, 4, lb.bytes, &w4));
  ELP_HIP(c, hipMemcpyAsync(w4 + lb.off, b_off.data(), 8 * (n + 1), hipMemcpyHostToDevice, st));
  ELP_HIP(c, hipMemcpyAsync(w0 + la.idx1, iota.data(), 4 * n, hipMemcpyHostToDevice, st));
  ELP_LAUNCH(c, "sw_decode", k_sw_decode, dim3((unsigned)n), dim3(64), 0, d_read_idx, (const uint8_t *)c->raw.p, (const uint64_t *)c->raw_off.p,
             reinterpret_cast<const uint64_t *>(w4 + lb.off), w4 + lb.seq);
  ELP_HIP(c, elp::stream_wait(st));
  const SwDev d{w0 + la.seq, w4 + lb.seq, reinterpret_cast<const uint64_t *>(w0 + la.off), reinterpret_cast<const uint64_t *>(w4 + lb.off),
                reinterpret_cast<const uint32_t *>(w0 + la.idx0), reinterpret_cast<const uint32_t *>(w0 + la.idx1)};
  return sw_run(c, who, d, n, len_ref.data(), len_alt.data(), bound, SwParams{match, mismatch, gap_open, gap_extend, strategy}, cigar_out, cigar_cap, cigar_off_out, offset_out,
                n_ops_out);
}

}  // extern "C"
