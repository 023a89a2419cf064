// bgzf_records.hip — BGZF on the device: where the alignment records start in the inflated stream.
#include "bgzf.hpp"

namespace elp {

// A reader walks the block_size chain record by record (sam/bam-files.go: one record after the other from the stream); that is one
// dependent load per record - 50 M of them.  Here every inflated block GUESSES its first record start (the first offset at which a
// well-formed record header stands and whose block_size chain stays well-formed for a few records), walks its own records from there
// and reports where its chain leaves the block; the guesses are then PROVEN: the chain that starts at the known first record of the
// stream enters every block exactly at that block's guess iff every block's exit equals the next block's guess - checked for all
// blocks at once.  Where a guess was wrong (a byte pattern that happened to look like a record), one thread repairs the entries in
// order.  The result is exact; the guessing only decides how much runs in parallel.
struct RecScan {
  const uint8_t *raw;
  uint64_t begin, end;  // the stream's bytes in c->raw: the first record of the piece starts at `begin`
  int32_t n_ref;
};
constexpr uint64_t REC_NONE = ~0ull;
__device__ __forceinline__ uint32_t ld32(const uint8_t *p) { uint32_t v; __builtin_memcpy(&v, p, 4); return v; }
// could a record start at p?  (fields of the fixed part, sam/bam-files.go:parseBamAlignment; everything that is checkable inside the data)
__device__ inline bool rec_plausible(const RecScan &r, uint64_t p) {
  if (p + 36 > r.end) return false;
  const uint8_t *q = r.raw + p;
  const uint32_t bs = ld32(q);
  if (bs < 32 || bs > (1u << 28)) return false;
  const int32_t refid = (int32_t)ld32(q + 4), pos = (int32_t)ld32(q + 8), next_refid = (int32_t)ld32(q + 24), next_pos = (int32_t)ld32(q + 28);
  if (refid < -1 || refid >= r.n_ref || next_refid < -1 || next_refid >= r.n_ref || pos < -1 || next_pos < -1) return false;
  const uint32_t l_name = q[12], n_cig = q[16] | ((uint32_t)q[17] << 8), l_seq = ld32(q + 20);
  if (l_name < 1 || l_seq > (1u << 28)) return false;
  const uint64_t need = 32ull + l_name + 4ull * n_cig + (l_seq + 1) / 2 + l_seq;
  if (need > bs) return false;
  const uint64_t nul = p + 36 + l_name - 1;
  if (nul < r.end && r.raw[nul] != 0) return false;
  return true;
}
// per inflated block: first / one-past-last byte in c->raw
__global__ __launch_bounds__(256) void k_rec_guess(RecScan r, const BgzfBlk *__restrict__ blk, uint64_t *__restrict__ guess, int weak) {
  __shared__ unsigned long long s_best;
  const BgzfBlk B = blk[blockIdx.x];
  // (the first block of a piece also owns the bytes in front of it: the record that was pending when the previous piece ended starts there)
  const uint64_t lo = (blockIdx.x == 0 || B.out_off < r.begin) ? r.begin : B.out_off, hi = B.out_off + B.out_len;
  if (threadIdx.x == 0) s_best = (weak && lo < hi) ? lo + (blockIdx.x % 3u) : REC_NONE;  // weak: a guess without a look at the bytes
  __syncthreads();
  for (uint64_t base = lo; !weak && base < hi; base += 256) {
    const uint64_t p = base + threadIdx.x;
    if (p < hi && rec_plausible(r, p)) {
      // the chain must stay plausible for up to three more records (as far as the data at hand goes)
      uint64_t q = p + 4ull + ld32(r.raw + p);
      bool ok = true;
      for (int k = 0; ok && k < 3 && q + 36 <= r.end; k++) {
        ok = rec_plausible(r, q);
        q += 4ull + ld32(r.raw + q);
      }
      if (ok) atomicMin(&s_best, (unsigned long long)p);
    }
    __syncthreads();
    if (s_best != REC_NONE) break;  // (uniform: read behind the barrier)
    __syncthreads();
  }
  if (threadIdx.x == 0) guess[blockIdx.x] = s_best;
}
// the record at p is not complete in the data at hand: it stays pending (the next piece brings the rest)
__device__ __forceinline__ bool rec_incomplete(const RecScan &r, uint64_t p) { return p + 4 > r.end || p + 4ull + ld32(r.raw + p) > r.end; }
// thread per block: the complete records that START in the block, from its entry; exit = where the chain leaves the block, or the first
// record that is not complete in the data.  fill: also writes the starts (second pass)
__device__ inline void rec_walk(const RecScan &r, uint64_t entry, uint64_t hi, uint64_t *exit_out, uint32_t *cnt_out, uint64_t *starts, uint32_t *max_rec) {
  uint64_t p = entry;
  uint32_t cnt = 0, mx = 0;
  while (p < hi) {
    if (rec_incomplete(r, p)) break;
    const uint64_t nx = p + 4ull + ld32(r.raw + p);
    if (starts) starts[cnt] = p;
    cnt++;
    const uint32_t sz = (uint32_t)(nx - p);
    mx = sz > mx ? sz : mx;
    p = nx;
  }
  *exit_out = p;
  *cnt_out = cnt;
  if (max_rec && mx) atomicMax(max_rec, mx);
}
__global__ __launch_bounds__(64) void k_rec_walk(RecScan r, const BgzfBlk *__restrict__ blk, uint32_t n_blk, const uint64_t *__restrict__ entry, uint64_t *__restrict__ exit_,
                                                 uint32_t *__restrict__ cnt) {
  const uint32_t b = blockIdx.x * 64 + threadIdx.x;
  if (b >= n_blk) return;
  const uint64_t hi = blk[b].out_off + blk[b].out_len;
  if (entry[b] == REC_NONE) { exit_[b] = REC_NONE; cnt[b] = 0; return; }
  rec_walk(r, entry[b], hi, &exit_[b], &cnt[b], nullptr, nullptr);
}
// the proof: block b's guess is the true entry iff the nearest block in front of it that has an entry leaves its records exactly there
// (blocks in between hold no record start: the chain jumps over them); the first entry must be the stream's known first record
__global__ __launch_bounds__(256) void k_rec_check(RecScan r, const BgzfBlk *__restrict__ blk, uint32_t n_blk, const uint64_t *__restrict__ entry,
                                                   const uint64_t *__restrict__ exit_, uint32_t *bad, uint32_t *__restrict__ bad_list) {
  const uint32_t b = blockIdx.x * 256 + threadIdx.x;
  if (b >= n_blk) return;
  const uint64_t lo = blk[b].out_off, hi = lo + blk[b].out_len;
  int64_t a = (int64_t)b - 1;
  while (a >= 0 && entry[a] == REC_NONE) a--;
  const uint64_t came = a >= 0 ? exit_[a] : r.begin;  // where the true chain stands when it reaches this block (if everything in front is right)
  bool ok;
  if (entry[b] == REC_NONE) ok = came >= hi || rec_incomplete(r, came);  // no complete record starts here: the chain jumps over the block, or stands at the pending record
  else ok = came == entry[b];
  if (hi <= r.begin) ok = true;  // a block of the header prefix
  (void)lo;
  if (!ok) {
    const uint32_t k = atomicAdd(bad, 1u);
    if (k < REC_BAD_CAP) bad_list[k] = b;
  }
}
// one thread, in order: entries that the proof rejected are replaced by where the chain really arrives.  Only the rejected blocks are
// visited (round 6: the loop over all blocks - a dependent load each - took 15 ms for 19 k blocks because of one wrong guess), each followed
// by the blocks behind it for as long as the repaired chain arrives somewhere else than they assumed.
__device__ inline uint64_t rec_repair_block(const RecScan &r, const BgzfBlk *blk, uint32_t b, uint64_t came, uint64_t *entry, uint64_t *exit_, uint32_t *cnt) {
  const uint64_t hi = blk[b].out_off + blk[b].out_len;
  if (hi <= r.begin) return came;
  const uint64_t want = (came < hi && !rec_incomplete(r, came)) ? came : REC_NONE;
  if (entry[b] != want && !(want == REC_NONE && entry[b] == came)) {  // (an entry at the pending record itself is as good as none)
    entry[b] = want;
    if (want == REC_NONE) { exit_[b] = REC_NONE; cnt[b] = 0; }
    else rec_walk(r, want, hi, &exit_[b], &cnt[b], nullptr, nullptr);
  }
  return entry[b] != REC_NONE ? exit_[b] : came;
}
__global__ void k_rec_repair(RecScan r, const BgzfBlk *__restrict__ blk, uint32_t n_blk, uint64_t *entry, uint64_t *exit_, uint32_t *cnt, const uint32_t *bad,
                             uint32_t *bad_list) {
  const uint32_t n_bad = bad[0];
  if (n_bad > REC_BAD_CAP) {
    uint64_t came = r.begin;
    for (uint32_t b = 0; b < n_blk; b++) came = rec_repair_block(r, blk, b, came, entry, exit_, cnt);
    return;
  }
  for (uint32_t i = 1; i < n_bad; i++) {  // (the list is in the order of the atomics: sort it, it is short)
    const uint32_t v = bad_list[i];
    uint32_t j = i;
    for (; j > 0 && bad_list[j - 1] > v; j--) bad_list[j] = bad_list[j - 1];
    bad_list[j] = v;
  }
  uint32_t done = 0;  // blocks below are consistent with the repaired chain
  for (uint32_t i = 0; i < n_bad; i++) {
    uint32_t b = bad_list[i];
    if (b < done) continue;
    int64_t a = (int64_t)b - 1;
    while (a >= 0 && entry[a] == REC_NONE) a--;
    uint64_t came = a >= 0 ? exit_[a] : r.begin;
    for (;;) {
      came = rec_repair_block(r, blk, b, came, entry, exit_, cnt);
      if (++b >= n_blk) break;
      // does the next block stand as it is?  (k_rec_check's condition, with the chain as it is now)
      const uint64_t hi = blk[b].out_off + blk[b].out_len;
      const bool ok = hi <= r.begin || (entry[b] == REC_NONE ? (came >= hi || rec_incomplete(r, came)) : came == entry[b]);
      if (ok) break;
    }
    done = b;
  }
}
__global__ __launch_bounds__(64) void k_rec_fill(RecScan r, const BgzfBlk *__restrict__ blk, uint32_t n_blk, const uint64_t *__restrict__ entry,
                                                 const uint32_t *__restrict__ base, uint64_t *__restrict__ rec_off, uint32_t *max_rec) {
  const uint32_t b = blockIdx.x * 64 + threadIdx.x;
  if (b >= n_blk || entry[b] == REC_NONE) return;
  uint64_t ex;
  uint32_t cn;
  rec_walk(r, entry[b], blk[b].out_off + blk[b].out_len, &ex, &cn, rec_off + base[b], max_rec);
}
__global__ void k_rec_tail(const uint64_t *__restrict__ entry, const uint64_t *__restrict__ exit_, uint32_t n_blk, uint64_t begin, uint64_t *__restrict__ out /* [0] = end of the last complete record */) {
  uint64_t e = begin;
  for (int64_t b = (int64_t)n_blk - 1; b >= 0; b--)
    if (entry[b] != REC_NONE) { e = exit_[b]; break; }
  out[0] = e;
}

// what the decoder reported for the inflate piece, from the result words as read back (once per inflate piece)
static int inflate_verdict(elp_ctx *c, BgzfPiece &piece, const BgzfRes &hr) {
  if (hr.inflate & INFLATE_BAD_DATA) return set_error(c, ELP_ERR_DATA, "elp_stage_bgzf: a block does not inflate (corrupt DEFLATE data or wrong ISIZE)");
  if (hr.inflate & INFLATE_BAD_CRC) return set_error(c, ELP_ERR_DATA, "invalid CRC-32 value for a data block in a BGZF file");
  piece.inflate_checked = true;
  return 0;
}

// One scan piece: the records that start in the blocks [rel, rel + nb) of the inflate piece, the first of them at `begin` in c->raw.
// Guess, walk, check, (read-back: also what the decoder reported, once per inflate piece,) repair where a guess was rejected, the scan of
// the counts, the starts into c->raw_off behind the c->n that are there, the end of the last complete record.
int bgzf_scan_piece(elp_ctx *c, BgzfPiece &piece, size_t rel, uint32_t nb, uint64_t begin, BgzfScan *out) {
  hipStream_t st = c->stream;
  const BgzfBlk *d_blk = piece.blk + rel;
  uint64_t *entry = piece.entry + rel, *exit_ = piece.exit + rel;
  uint32_t *cnt = piece.cnt + rel, *base = piece.base + rel;
  BgzfRes *res = piece.res;
  ELP_HIP(c, hipMemsetAsync(res, 0, BgzfRes::CLEAR_SCAN, st));
  const BgzfBlk &last = piece.tb[rel + nb - 1];
  const uint64_t end = last.out_off + last.out_len;
  // a piece wholly in front of the first record (a header prefix longer than a scan piece) stages nothing and `begin` stands; its blocks
  // are inflated and checked all the same
  const bool in_front = end <= begin;
  const RecScan rs{c->raw.p, begin, end, c->n_ref};
  if (!in_front) {
    ELP_LAUNCH(c, "stage_bgzf_guess", k_rec_guess, dim3(nb), dim3(256), 0, rs, d_blk, entry, c->tune.bgzf_weak_guess);
    ELP_LAUNCH(c, "stage_bgzf_walk", k_rec_walk, dim3(blocks_for(nb, 64)), dim3(64), 0, rs, d_blk, nb, (const uint64_t *)entry, exit_, cnt);
    ELP_LAUNCH(c, "stage_bgzf_check", k_rec_check, dim3(blocks_for(nb, 256)), dim3(256), 0, rs, d_blk, nb, (const uint64_t *)entry, (const uint64_t *)exit_, &res->bad, piece.bad_list);
  }
  BgzfRes hr{};
  if (!in_front || !piece.inflate_checked) {
    ELP_HIP(c, hipMemcpyAsync(&hr, res, sizeof hr, hipMemcpyDeviceToHost, st));
    ELP_HIP(c, elp::stream_wait(st));
  }
  if (!piece.inflate_checked) ELP_TRY(inflate_verdict(c, piece, hr));
  if (in_front) {
    *out = BgzfScan{0, begin, 0};
    return 0;
  }
  if (hr.bad) ELP_LAUNCH(c, "stage_bgzf_repair", k_rec_repair, dim3(1), dim3(1), 0, rs, d_blk, nb, entry, exit_, cnt, (const uint32_t *)&res->bad, piece.bad_list);
  uint32_t n_rec = 0;
  ELP_TRY(exclusive_scan_u32(c, cnt, base, nb, &n_rec));
  if (c->n + n_rec > 0xFFFFFFF0ull) return set_error(c, ELP_ERR_UNSUPPORTED, "more than 2^32-16 records per context");
  ELP_TRY(ensure(c, c->raw_off, c->n + n_rec + 2, true, c->n + 1));
  ELP_LAUNCH(c, "stage_bgzf_fill", k_rec_fill, dim3(blocks_for(nb, 64)), dim3(64), 0, rs, d_blk, nb, (const uint64_t *)entry, (const uint32_t *)base,
             c->raw_off.p + c->n, &res->max_rec);
  ELP_LAUNCH(c, "stage_bgzf_tail", k_rec_tail, dim3(1), dim3(1), 0, (const uint64_t *)entry, (const uint64_t *)exit_, nb, begin, c->raw_off.p + c->n + n_rec);
  uint64_t rec_end = 0;
  ELP_HIP(c, hipMemcpyAsync(&rec_end, c->raw_off.p + c->n + n_rec, 8, hipMemcpyDeviceToHost, st));
  ELP_HIP(c, hipMemcpyAsync(&hr, res, sizeof hr, hipMemcpyDeviceToHost, st));
  ELP_HIP(c, elp::stream_wait(st));
  if (rec_end < begin || rec_end > end) return set_error(c, ELP_ERR_DATA, "elp_stage_bgzf: the alignment records do not chain (block_size fields)");
  *out = BgzfScan{n_rec, rec_end, hr.max_rec};
  return 0;
}

}  // namespace elp
