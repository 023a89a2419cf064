// sort.hip — the coordinate sort (its key column is the adapt stage's, adapt.hip).
//
// Reference: sam.CoordinateLess + modFlag (sam/sam-types.go:408-473), By.ParallelStableSort (:639-641).
//
// Sort = (1) 64-bit primary key {refid (unmapped last), POS, strand} sorted by the LSD radix sort of radix.hip,
//        (2) tie resolution inside runs of equal primary key with the comparator tail
//            {QNAME bytes, modFlag, MAPQ, [NextREFID, PNEXT if paired], TLEN}, ties keep staging order:
//            runs <= TIE_SMALL records: every record computes its rank in the run directly (all-pairs);
//            larger runs (the unmapped block, pile-ups): LSD radix over the live bytes of the zero-padded comparator string,
//            8 bytes per round, then one stable round on the run id.
// The host's part - key format, run bounds, scratch layout, rank tables, the packing of the rounds' keys - is sort_plan.hpp's: the
// phases at the end of this file launch and copy, and compute no size, offset, width or cut themselves.
#include <algorithm>
#include <cstdlib>

#include "common.hpp"
#include "sort_plan.hpp"  // TIE_SMALL, TIE_MAX_PACKED

namespace elp {

// ------------------------------------------------------------------ tie-break
struct TieCols {
  const uint64_t *qname_off;
  const uint8_t *qname;
  const uint16_t *flag;
  const uint8_t *mapq;
  const int32_t *next_refid, *pnext, *tlen;
  const uint8_t *rows = nullptr;  // the radix tie-break's comparator strings written out (k_material_rows): rows[m * rw + j] = byte j of member m
  uint32_t rw = 0;
};

// comparator tail of CoordinateLess (:439-472) for two records with equal (refid, pos, strand)
__device__ inline bool tie_less(const TieCols &t, uint32_t a, uint32_t b) {
  const uint32_t la = (uint32_t)(t.qname_off[a + 1] - t.qname_off[a]), lb = (uint32_t)(t.qname_off[b + 1] - t.qname_off[b]);
  if (la != 0 && lb != 0) {
    int c = qname_cmp(t.qname, t.qname_off, a, b);
    if (c < 0) return true;
    if (c > 0) return false;
  }
  const uint16_t fa = mod_flag(t.flag[a]), fb = mod_flag(t.flag[b]);
  if (fa < fb) return true;
  if (fa > fb) return false;
  const uint8_t ma = t.mapq[a], mb = t.mapq[b];
  if (ma < mb) return true;
  if (ma > mb) return false;
  if ((t.flag[a] & F_MULTIPLE) && (t.flag[b] & F_MULTIPLE)) {
    const int32_t na = t.next_refid[a], nb = t.next_refid[b];
    if (na < nb) return true;
    if (na > nb) return false;
    const int32_t pa = t.pnext[a], pb = t.pnext[b];
    if (pa < pb) return true;
    if (pa > pb) return false;
  }
  return t.tlen[a] < t.tlen[b];
}

__global__ __launch_bounds__(256) void k_iota(uint32_t *v, uint64_t n) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) v[i] = (uint32_t)i;
}

// the sorted array: (key, index) pairs in two arrays, or - idx_bits > 0 - words key << idx_bits | index (radix_sort_fused)
struct SortedView {
  const uint64_t *__restrict__ keys;
  const uint32_t *__restrict__ vals;
  uint32_t idx_bits;
  __device__ __forceinline__ uint64_t key(uint64_t i) const { return idx_bits ? keys[i] >> idx_bits : keys[i]; }
  __device__ __forceinline__ uint32_t val(uint64_t i) const { return idx_bits ? (uint32_t)(keys[i] & ((1ull << idx_bits) - 1ull)) : vals[i]; }
};

// Runs of equal primary key.  k_tie_scan (every record, three loads issued together): a record whose neighbours both differ is
// final; members of runs go to a compact list.  k_tie_small (list members only, all lanes busy with the same kind of work): runs of
// <= TIE_SMALL records are ranked by all-pairs comparison, members of longer runs are flagged for the radix tie-break.
constexpr int TS_TILES = 32;  // (16: 12 K workgroups queue at the one list counter for 0.15 ms of the kernel's 0.30)
__global__ __launch_bounds__(256) void k_tie_scan(uint64_t n, SortedView sv, uint32_t *__restrict__ perm_out, uint32_t *__restrict__ list, uint32_t *list_n,
                                                  uint32_t *__restrict__ bounds) {
  if (blockIdx.x == 0 && threadIdx.x < 4) bounds[threadIdx.x] = 0;  // the counters of k_tie_small's lists (it runs behind this kernel)
  // a workgroup handles TS_TILES * 256 consecutive records and collects its run members in LDS: ONE global atomic per workgroup
  // (a global atomic per wave on the single list counter serialises at ~12 ns each: 9 ms for 50 M records, measured)
  __shared__ uint32_t lq[TS_TILES * 256];
  __shared__ uint32_t lcount, gbase;
  if (threadIdx.x == 0) lcount = 0;
  __syncthreads();
#pragma unroll 1
  for (int tile = 0; tile < TS_TILES; tile++) {
    const uint64_t i = ((uint64_t)blockIdx.x * TS_TILES + (uint64_t)tile) * 256 + threadIdx.x;
    bool in_run = false;
    if (i < n) {
      const uint64_t w = sv.keys[i], wp = i > 0 ? sv.keys[i - 1] : 0ull, wn = i + 1 < n ? sv.keys[i + 1] : 0ull;
      const uint64_t k = w >> sv.idx_bits, kp = i > 0 ? wp >> sv.idx_bits : ~k, kn = i + 1 < n ? wn >> sv.idx_bits : ~k;
      const uint32_t me = sv.idx_bits ? (uint32_t)(w & ((1ull << sv.idx_bits) - 1ull)) : sv.vals[i];
      in_run = kp == k || kn == k;
      if (!in_run) perm_out[i] = me;
    }
    const unsigned long long mask = __ballot(in_run);
    if (mask) {
      const int lane = threadIdx.x & 63, leader = __ffsll((long long)mask) - 1;
      uint32_t base = 0;
      if (lane == leader) base = atomicAdd(&lcount, (uint32_t)__popcll(mask));
      base = __shfl(base, leader, 64);
      if (in_run) lq[base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = (uint32_t)i;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) gbase = lcount ? atomicAdd(list_n, lcount) : 0u;
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < lcount; k += 256) list[gbase + k] = lq[k];
}
__global__ __launch_bounds__(256) void k_tie_small(uint64_t n, SortedView sv, uint32_t *__restrict__ perm_out, uint32_t *__restrict__ bounds /* [0] starts, [1] ends counted; [4 + k] / [4 + cap + k] the positions */,
                                                   uint32_t bounds_cap, const uint32_t *__restrict__ list, const uint32_t *__restrict__ list_n, TieCols t) {
  const uint64_t j0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j0 >= (uint64_t)*list_n) return;
  const uint64_t i = list[j0];
  const uint64_t k = sv.key(i);
  const uint32_t me = sv.val(i);
  uint64_t s = i, e = i + 1;  // run [s, e)
  bool large = false;
  while (s > 0 && sv.key(s - 1) == k) {
    s--;
    if (i - s >= (uint64_t)TIE_SMALL) { large = true; break; }
  }
  if (!large) {
    while (e < n && sv.key(e) == k) {
      e++;
      if (e - s > (uint64_t)TIE_SMALL) { large = true; break; }
    }
  }
  if (large) {
    // a run of more than TIE_SMALL records goes to the radix tie-break as a RANGE of the sorted array: its first member reports where
    // it starts, its last one where it ends (two short lists the host pairs up) - no flag per record, no scan over all records
    perm_out[i] = me;
    if (i == 0 || sv.key(i - 1) != k) { const uint32_t at = atomicAdd(&bounds[0], 1u); if (at < bounds_cap) bounds[4 + at] = (uint32_t)i; }
    if (i + 1 == n || sv.key(i + 1) != k) { const uint32_t at = atomicAdd(&bounds[1], 1u); if (at < bounds_cap) bounds[4 + bounds_cap + at] = (uint32_t)i; }
    return;
  }
  if (e - s == 2) {
    // a run of two (nine runs in ten): its first member places both with ONE comparison, the second has nothing to do
    if (i != s) return;
    const uint32_t other = sv.val(s + 1);
    const bool swap = tie_less(t, other, me);  // `me` came first: it stays in front unless the other one is strictly less
    perm_out[s] = swap ? other : me;
    perm_out[s + 1] = swap ? me : other;
    return;
  }
  uint32_t rank = 0;
  for (uint64_t j = s; j < e; j++) {
    if (j == i) continue;
    const uint32_t other = sv.val(j);
    // other precedes me iff other < me, or neither is less and other came first (radix sort is stable: j < i <=> earlier staging index)
    if (tie_less(t, other, me)) rank++;
    else if (j < i && !tie_less(t, me, other)) rank++;
  }
  perm_out[s + rank] = me;
}

// members of the large runs, compacted: run r = positions [start[r], start[r] + (first[r + 1] - first[r])) of the sorted array, its members are
// numbers first[r] .. first[r + 1] - 1; u_seg = 1 + r (the key of the last, stable round: runs stay apart and in order)
__global__ __launch_bounds__(256) void k_large_fill(uint32_t nu, uint32_t nr, const uint32_t *__restrict__ start, const uint32_t *__restrict__ first,
                                                    SortedView sv, uint32_t *__restrict__ u_pos, uint32_t *__restrict__ u_read,
                                                    uint32_t *__restrict__ u_seg) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nu) return;
  uint32_t lo = 0, hi = nr;  // the run with first[r] <= j < first[r + 1]
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (first[mid] <= j) lo = mid; else hi = mid;
  }
  const uint32_t pos = start[lo] + (j - first[lo]);
  u_pos[j] = pos;
  u_read[j] = sv.val(pos);
  u_seg[j] = lo + 1u;
}

// comparator byte string of record r: QNAME zero-padded to maxq, then modFlag(2, BE), MAPQ(1), NextREFID^msb(4, BE), PNEXT^msb(4, BE)
// (both zero when unpaired; paired-ness is part of modFlag so it is constant within equal prefixes), TLEN^msb(4, BE).
__device__ inline uint32_t material_byte(const TieCols &t, uint32_t r, uint32_t j, uint32_t maxq, uint32_t m = 0) {
  if (t.rows) return t.rows[(size_t)m * t.rw + j];  // m = the member's number
  if (j < maxq) {
    const uint64_t o = t.qname_off[r];
    const uint32_t l = (uint32_t)(t.qname_off[r + 1] - o);
    return j < l ? t.qname[o + j] : 0u;
  }
  const uint32_t f = j - maxq;
  const uint16_t fl = t.flag[r];
  if (f < 2) { const uint16_t m = mod_flag(fl); return f == 0 ? (m >> 8) : (m & 0xFF); }
  if (f == 2) return t.mapq[r];
  if (f < 11) {
    if (!(fl & F_MULTIPLE)) return 0u;
    const uint32_t v = (f < 7 ? (uint32_t)t.next_refid[r] : (uint32_t)t.pnext[r]) ^ 0x80000000u;
    const uint32_t b = (f < 7) ? (f - 3) : (f - 7);
    return (v >> (8 * (3 - b))) & 0xFF;
  }
  if (f < 15) {
    const uint32_t v = (uint32_t)t.tlen[r] ^ 0x80000000u;
    return (v >> (8 * (3 - (f - 11)))) & 0xFF;
  }
  return 0u;
}

// The comparator strings of the large runs' members written out once, `rw` bytes per member (a thread writes eight bytes): the kernels
// of the LSD rounds then read a member's bytes from one or two cache lines instead of chasing QNAME offsets, names and four columns per
// byte (k_material_values and the key kernels took 0.5 ms for the 500 K unmapped reads of the bench workload).
__global__ __launch_bounds__(256) void k_material_rows(uint32_t nu, const uint32_t *__restrict__ u_read, uint32_t maxq, uint32_t nbytes, uint32_t rw,
                                                       uint8_t *__restrict__ rows, TieCols t /* t.rows == nullptr */) {
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t per = rw >> 3;
  const uint64_t m = g / per;
  if (m >= nu) return;
  const uint32_t k = (uint32_t)(g - m * per) * 8u, r = u_read[m];
  uint64_t v = 0;
  for (uint32_t i = 0; i < 8; i++)
    if (k + i < nbytes) v |= (uint64_t)material_byte(t, r, k + i, maxq) << (8 * i);
  reinterpret_cast<uint64_t *>(rows + m * rw)[k >> 3] = v;
}

// bit j of live[]: byte j of the comparator string is not the same for all members of large runs (compared with member 0's).
// QNAME bytes are compared eight at a time (zero-padded behind the name's end, as material_byte pads them).
__global__ __launch_bounds__(256) void k_material_live(uint32_t nu, const uint32_t *__restrict__ u_read, uint32_t maxq, uint32_t nbytes,
                                                       uint32_t *live, TieCols t) {
  __shared__ uint32_t acc[elp_ctx::TIE_LIVE_WORDS];
  if (threadIdx.x < elp_ctx::TIE_LIVE_WORDS) acc[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m < nu && t.rows) {
    // the strings are written out: member m's row against member 0's, eight bytes at a time
    const uint64_t *a8 = reinterpret_cast<const uint64_t *>(t.rows + (size_t)m * t.rw), *b8 = reinterpret_cast<const uint64_t *>(t.rows);
    for (uint32_t k = 0; k < nbytes; k += 8) {
      uint64_t x = a8[k >> 3] ^ b8[k >> 3];
      if (x) {
        x |= x >> 4; x |= x >> 2; x |= x >> 1;
        x &= 0x0101010101010101ull;
        const uint32_t bits = (uint32_t)((x * 0x0102040810204080ull) >> 56);
        for (uint32_t i = 0; i < 8 && k + i < nbytes; i++)
          if ((bits >> i) & 1u) atomicOr(&acc[(k + i) >> 5], 1u << ((k + i) & 31));
      }
    }
  } else if (m < nu) {
    const uint32_t r = u_read[m], r0 = u_read[0];
    const uint64_t oa = t.qname_off[r], ob = t.qname_off[r0];
    const uint32_t la = (uint32_t)(t.qname_off[r + 1] - oa), lb = (uint32_t)(t.qname_off[r0 + 1] - ob);
    for (uint32_t k = 0; k < maxq; k += 8) {
      const uint64_t a = k < la ? low_bytes(load8(t.qname + oa + k), la - k) : 0ull;
      const uint64_t b = k < lb ? low_bytes(load8(t.qname + ob + k), lb - k) : 0ull;
      uint64_t x = a ^ b;
      if (x) {
        x |= x >> 4; x |= x >> 2; x |= x >> 1;  // bit 0 of every byte: the byte is not zero
        x &= 0x0101010101010101ull;
        const uint32_t bits = (uint32_t)((x * 0x0102040810204080ull) >> 56);  // bit i: byte i differs
        for (uint32_t i = 0; i < 8 && k + i < maxq; i++)
          if ((bits >> i) & 1u) atomicOr(&acc[(k + i) >> 5], 1u << ((k + i) & 31));
      }
    }
    for (uint32_t j = maxq; j < nbytes; j++)
      if (material_byte(t, r, j, maxq) != material_byte(t, r0, j, maxq)) atomicOr(&acc[j >> 5], 1u << (j & 31));
  }
  __syncthreads();
  if (threadIdx.x < elp_ctx::TIE_LIVE_WORDS && acc[threadIdx.x]) atomicOr(&live[threadIdx.x], acc[threadIdx.x]);
}

// which byte values occur at every live position (bitmap of 256 bits per position, collected in LDS); TIE_MAX_PACKED (sort_plan.hpp):
// live positions up to which the packed keys below are used
struct TiePosList { uint16_t pos[TIE_MAX_PACKED]; uint32_t n; };
__global__ __launch_bounds__(256) void k_material_values(uint32_t nu, const uint32_t *__restrict__ u_read, TiePosList lp, uint32_t maxq,
                                                         uint32_t *vals /* [n][8] */, TieCols t) {
  __shared__ uint32_t acc[TIE_MAX_PACKED * 8];
  for (uint32_t k = threadIdx.x; k < lp.n * 8; k += blockDim.x) acc[k] = 0;
  __syncthreads();
  for (uint32_t m = blockIdx.x * blockDim.x + threadIdx.x; m < nu; m += gridDim.x * blockDim.x) {
    const uint32_t r = u_read[m];
    for (uint32_t k = 0; k < lp.n; k++) {
      const uint32_t v = material_byte(t, r, lp.pos[k], maxq, m);
      const uint32_t bit = 1u << (v & 31u);
      uint32_t *w = &acc[k * 8 + (v >> 5)];
      if (!(*w & bit)) atomicOr(w, bit);
    }
  }
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < lp.n * 8; k += blockDim.x)
    if (acc[k]) atomicOr(&vals[k], acc[k]);
}
// key of a member = the RANKS of its bytes (among the values that occur at the position: same order, fewer bits) at up to 64
// positions, most significant first: pos[j] is shifted to bit `shift[j]`; rank = lut[slot[j] * 256 + byte]
struct TiePacked { uint16_t pos[64]; uint8_t shift[64]; uint8_t slot[64]; uint32_t n; };
__global__ __launch_bounds__(256) void k_material_keys_packed(uint32_t nu, const uint32_t *__restrict__ vals, const uint32_t *__restrict__ u_read,
                                                              TiePacked sel, const uint8_t *__restrict__ lut, uint32_t maxq, uint64_t *__restrict__ keys,
                                                              TieCols t, const uint32_t *__restrict__ u_seg, uint32_t seg_shift) {
  uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nu) return;
  const uint32_t mem = vals[j], r = u_read[mem];
  uint64_t k = u_seg ? (uint64_t)u_seg[mem] << seg_shift : 0ull;  // the run id in front: runs stay apart and in order
  for (uint32_t b = 0; b < sel.n; b++) k |= (uint64_t)lut[(uint32_t)sel.slot[b] * 256u + material_byte(t, r, sel.pos[b], maxq, mem)] << sel.shift[b];
  keys[j] = k;
}

// key of a member = the bytes of its comparator string at the (up to eight) positions pos[0] < pos[1] < ..., most significant first
struct TieSel { uint16_t pos[8]; uint32_t n; };
__global__ __launch_bounds__(256) void k_material_keys_sel(uint32_t nu, const uint32_t *__restrict__ vals, const uint32_t *__restrict__ u_read,
                                                           TieSel sel, uint32_t maxq, uint64_t *__restrict__ keys, TieCols t) {
  uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nu) return;
  const uint32_t mem = vals[j], r = u_read[mem];
  uint64_t k = 0;
  for (uint32_t b = 0; b < sel.n; b++) k = (k << 8) | material_byte(t, r, sel.pos[b], maxq, mem);
  keys[j] = k;
}

__global__ __launch_bounds__(256) void k_seg_keys(uint32_t nu, const uint32_t *__restrict__ vals, const uint32_t *__restrict__ u_seg_incl,
                                                  uint64_t *__restrict__ keys) {
  uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < nu) keys[j] = (uint64_t)u_seg_incl[vals[j]];
}


// The comparator strings of two members, all positions (the order the LSD rounds over every live position give).
__device__ inline int material_cmp(const TieCols &t, uint32_t ma, uint32_t ra, uint32_t mb, uint32_t rb, uint32_t nbytes, uint32_t maxq) {
  if (t.rows) {
    const uint64_t *a8 = reinterpret_cast<const uint64_t *>(t.rows + (size_t)ma * t.rw), *b8 = reinterpret_cast<const uint64_t *>(t.rows + (size_t)mb * t.rw);
    for (uint32_t k = 0; k < nbytes; k += 8) {  // bytes behind nbytes are zero in every row
      const uint64_t x = a8[k >> 3], y = b8[k >> 3];
      if (x != y) return __builtin_bswap64(x) < __builtin_bswap64(y) ? -1 : 1;
    }
    return 0;
  }
  for (uint32_t j = 0; j < nbytes; j++) {
    const uint32_t x = material_byte(t, ra, j, maxq), y = material_byte(t, rb, j, maxq);
    if (x != y) return x < y ? -1 : 1;
  }
  return 0;
}
// Members of the large runs sorted on ONE key: the run id and the ranks of the most significant live positions that fit 64 bits
// (read names differ early: nearly every key is unique or shared by the two mates of a pair).  What the key leaves open is settled
// here: a member whose neighbours have other keys is final; the members of a group of equal keys rank themselves by comparing the
// whole strings (equal strings: the earlier member first, as the stable rounds leave them).  A group of more than LT_CAP members
// raises `over`: the host then runs the LSD rounds over all positions instead.
constexpr uint32_t LT_CAP = 1024;
__global__ __launch_bounds__(256) void k_large_ties(uint32_t nu, const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals,
                                                    uint32_t *__restrict__ vals_out, const uint32_t *__restrict__ u_read, uint32_t nbytes, uint32_t maxq,
                                                    uint32_t *over, TieCols t) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nu) return;
  const uint64_t k = keys[j];
  const uint32_t me = vals[j];
  const bool eq_prev = j > 0 && keys[j - 1] == k, eq_next = j + 1 < nu && keys[j + 1] == k;
  if (!eq_prev && !eq_next) { vals_out[j] = me; return; }
  uint32_t s = j, e = j + 1;  // group [s, e)
  bool large = false;
  while (s > 0 && keys[s - 1] == k) {
    s--;
    if (j - s >= LT_CAP) { large = true; break; }
  }
  while (!large && e < nu && keys[e] == k) {
    e++;
    if (e - s > LT_CAP) large = true;
  }
  if (large) {
    vals_out[j] = me;
    if (!eq_prev) atomicOr(over, 1u);
    return;
  }
  const uint32_t rme = u_read[me];
  uint32_t rank = 0;
  for (uint32_t i = s; i < e; i++) {
    if (i == j) continue;
    const uint32_t other = vals[i];
    const int c = material_cmp(t, other, u_read[other], me, rme, nbytes, maxq);
    if (c < 0 || (c == 0 && other < me)) rank++;
  }
  vals_out[s + rank] = me;
}

__global__ __launch_bounds__(256) void k_large_scatter(uint32_t nu, const uint32_t *__restrict__ vals_sorted, const uint32_t *__restrict__ u_pos,
                                                       const uint32_t *__restrict__ u_read, uint32_t *__restrict__ perm_out) {
  uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < nu) perm_out[u_pos[j]] = u_read[vals_sorted[j]];
}

// ------------------------------------------------------------------ the sort's phases, in the order they run
// What one sort's phases hand on.  Every size, offset, width and cut comes from sort_plan.hpp.
struct TieWork {
  uint64_t n;
  SortScratch sc;
  TieScratch lay{0, 0, 0};
  SortedView sv{nullptr, nullptr, 0};
  TieCols t{};
  uint32_t *list = nullptr, *bounds = nullptr;  // the half of `vbuf` the key passes left free; scratch slot 2
  uint32_t nr = 0, nu = 0, maxq = 0;            // long runs, their members; the longest name
  uint32_t *u_pos = nullptr, *u_read = nullptr, *u_seg = nullptr, *uv0 = nullptr, *uv1 = nullptr;
  uint64_t *uk0 = nullptr, *uk1 = nullptr;
  uint32_t *vcur = nullptr, *vtmp = nullptr;  // the members' order so far and the rounds' second buffer
  const uint8_t *d_lut = nullptr;
  explicit TieWork(uint64_t records) : n(records), sc(records) {}
};

// the key column holds key_bits live bits (adapt packs it): that many digit passes, no histogram read-back; the first pass reads
// the column itself and numbers the records as it goes (no copy, no index array)
static int sort_key_passes(elp_ctx *c, uint64_t *presorted, TieWork &w) {
  const uint64_t n = w.n;
  uint64_t *kbuf;
  uint32_t *vbuf;
  ELP_TRY(scratch(c, 0, w.sc.keys, &kbuf));
  ELP_TRY(scratch(c, 1, w.sc.vals, &vbuf));
  ELP_TRY(scratch(c, 2, w.sc.flags, &w.bounds));
  uint64_t *k0 = kbuf, *k1 = kbuf + n;
  uint32_t *v0 = vbuf, *v1 = vbuf + n;
  uint64_t *ks;
  uint32_t *vs = nullptr;
  // where key << b | index fits one word (a genome's coordinate key has ~31-34 live bits), the passes move words, not pairs
  const int idx_bits = index_bits(n);
  const bool words = sort_words(c->key_bits, idx_bits, c->tune.sort_pairs);
  if (words && presorted) ks = presorted;
  else if (words) ELP_TRY(radix_sort_fused(c, c->key.p, n, c->key_bits, idx_bits, k0, k1, &ks));
  else {
    ProfScope ps(c, "sort_pairs_");  // (the pair form's passes are booked apart from the word form's: tests see which one ran)
    ELP_TRY(radix_sort_pairs_low(c, k0, v0, k1, v1, n, key_digits(c->key_bits), &ks, &vs, c->key.p, true));
  }
  w.sv = SortedView{ks, vs, words ? (uint32_t)idx_bits : 0u};
  w.t = TieCols{c->qname_off.p, c->qname.p, c->flag.p, c->mapq.p, c->next_refid.p, c->pnext.p, c->tlen.p};
  w.list = (vs == v0) ? v1 : v0;  // (sorted words: `vbuf` is free altogether)
  return 0;
}

// run members -> compact list; runs up to TIE_SMALL records ranked; bounds of the longer ones -> two short lists in `bounds`
static int tie_short_runs(elp_ctx *c, TieWork &w) {
  const uint64_t n = w.n;
  uint32_t *list_n = c->err_flag.p + 3;  // the scan-total mailbox
  ELP_HIP(c, hipMemsetAsync(list_n, 0, 4, c->stream));
  ELP_LAUNCH(c, "tie_scan", k_tie_scan, dim3(blocks_for(n, 256 * TS_TILES)), dim3(256), 0, n, w.sv, c->perm.p, w.list, list_n, w.bounds);
  // sized for the worst case; workgroups beyond the list's end leave at once
  ELP_LAUNCH(c, "tie_small", k_tie_small, dim3(blocks_for(n, 256)), dim3(256), 0, n, w.sv, c->perm.p, w.bounds, w.sc.cap, (const uint32_t *)w.list, (const uint32_t *)list_n, w.t);
  ELP_HIP(c, hipMemsetAsync(list_n, 0, 4, c->stream));
  return 0;
}

// ONE read-back: the two counts and the first run bounds (all of them unless there are more than TIE_HEAD runs: then a second copy)
static int tie_read_bounds(elp_ctx *c, TieWork &w, LongRuns *runs) {
  const uint32_t head = bounds_head(w.sc.cap);
  std::vector<uint32_t> hs(w.sc.starts + head), he(head);
  ELP_HIP(c, hipMemcpyAsync(hs.data(), w.bounds, hs.size() * 4, hipMemcpyDeviceToHost, c->stream));
  ELP_HIP(c, hipMemcpyAsync(he.data(), w.bounds + w.sc.ends, (size_t)head * 4, hipMemcpyDeviceToHost, c->stream));
  ELP_HIP(c, elp::stream_wait(c->stream));
  const uint32_t nr = hs[0];
  if (!run_counts_ok(hs[0], hs[1], w.sc.cap)) return set_error(c, ELP_ERR_HIP, "coordinate sort: %u starts and %u ends of long runs (internal)", hs[0], hs[1]);
  std::vector<uint32_t> starts(nr), ends(nr);
  if (nr > 0 && bounds_in_head(nr)) {
    std::copy(hs.begin() + w.sc.starts, hs.begin() + w.sc.starts + nr, starts.begin());
    std::copy(he.begin(), he.begin() + nr, ends.begin());
  } else if (nr > 0) {
    ELP_HIP(c, hipMemcpyAsync(starts.data(), w.bounds + w.sc.starts, (size_t)nr * 4, hipMemcpyDeviceToHost, c->stream));
    ELP_HIP(c, hipMemcpyAsync(ends.data(), w.bounds + w.sc.ends, (size_t)nr * 4, hipMemcpyDeviceToHost, c->stream));
    ELP_HIP(c, elp::stream_wait(c->stream));
  }
  if (!long_runs(std::move(starts), std::move(ends), runs)) return set_error(c, ELP_ERR_HIP, "coordinate sort: long runs overlap (internal)");
  w.nr = runs->nr;
  w.nu = runs->nu;
  return 0;
}

// The long runs' members, compacted (+ their comparator strings written out, TieScratch::use_rows), and which positions of the string
// differ at all among them: one kernel, one read-back; the rounds then run over live positions only (no histogram read-back per
// round, no rounds over constant bytes)
static int tie_members(elp_ctx *c, TieWork &w, const LongRuns &runs, std::vector<uint16_t> *lp) {
  const uint32_t nu = w.nu, nr = w.nr, maxq = w.maxq = c->max_qname_len;
  const TieScratch &lay = w.lay = TieScratch(nu, nr, maxq);  // (m_bytes <= MAX_QNAME + 15: elp_stage enforces the QNAME limit)
  uint32_t *u;
  ELP_TRY(scratch(c, 3, lay.words3, &u));
  w.u_pos = u + lay.u_pos; w.u_read = u + lay.u_read; w.u_seg = u + lay.u_seg; w.uv0 = u + lay.uv0; w.uv1 = u + lay.uv1;
  uint32_t *d_start = u + lay.d_start, *d_first = u + lay.d_first;
  uint64_t *uk;
  ELP_TRY(scratch(c, 4, lay.words4, &uk));
  w.uk0 = uk + lay.uk0; w.uk1 = uk + lay.uk1;
  ELP_HIP(c, hipMemcpyAsync(d_start, runs.starts.data(), (size_t)nr * 4, hipMemcpyHostToDevice, c->stream));
  ELP_HIP(c, hipMemcpyAsync(d_first, runs.first.data(), ((size_t)nr + 1) * 4, hipMemcpyHostToDevice, c->stream));
  ELP_LAUNCH(c, "large_fill", k_large_fill, dim3(blocks_for(nu, 256)), dim3(256), 0, nu, nr, (const uint32_t *)d_start, (const uint32_t *)d_first, w.sv, w.u_pos, w.u_read, w.u_seg);
  ELP_LAUNCH(c, "iota", k_iota, dim3(blocks_for(nu, 256)), dim3(256), 0, w.uv0, (uint64_t)nu);
  static_assert(elp_ctx::MAX_QNAME + 15 <= 32 * elp_ctx::TIE_LIVE_WORDS, "live-position bitmap too small");
  ELP_TRY(ensure(c, c->tie_live, elp_ctx::TIE_LIVE_WORDS));
  ELP_HIP(c, hipMemsetAsync(c->tie_live.p, 0, elp_ctx::TIE_LIVE_WORDS * sizeof(uint32_t), c->stream));
  if (lay.use_rows) {
    uint8_t *rows = reinterpret_cast<uint8_t *>(u + lay.u_words);
    ELP_LAUNCH(c, "material_rows", k_material_rows, dim3(blocks_for((uint64_t)nu * (lay.rw >> 3), 256)), dim3(256), 0, nu, (const uint32_t *)w.u_read, maxq, lay.m_bytes, lay.rw,
               rows, w.t);
    w.t.rows = rows;
    w.t.rw = lay.rw;
  }
  ELP_LAUNCH(c, "material_live", k_material_live, dim3(blocks_for(nu, 256)), dim3(256), 0, nu, (const uint32_t *)w.u_read, maxq, lay.m_bytes,
             c->tie_live.p, w.t);
  uint32_t live[elp_ctx::TIE_LIVE_WORDS];
  ELP_HIP(c, hipMemcpyAsync(live, c->tie_live.p, sizeof live, hipMemcpyDeviceToHost, c->stream));
  ELP_HIP(c, elp::stream_wait(c->stream));
  *lp = live_positions(live, lay.m_bytes);
  w.vcur = w.uv0;
  w.vtmp = w.uv1;
  return 0;
}

// Few distinct byte values per live position (read names: digits and ':'): the rounds sort on their ranks instead of the bytes, as
// many positions per 64-bit key as fit - typically two LSD rounds of ~10 passes instead of five rounds of eight.
static int tie_rank_tables(elp_ctx *c, TieWork &w, const std::vector<uint16_t> &lp, RankFields *f) {
  TiePosList pl;
  pl.n = (uint32_t)lp.size();
  for (size_t k = 0; k < lp.size(); k++) pl.pos[k] = lp[k];
  uint32_t *s5;
  ELP_TRY(scratch(c, 5, w.lay.words5, &s5));
  uint32_t *d_vals = s5 + w.lay.d_vals;
  uint8_t *d_lut = reinterpret_cast<uint8_t *>(s5 + w.lay.d_lut);
  ELP_HIP(c, hipMemsetAsync(d_vals, 0, (size_t)pl.n * 8 * 4, c->stream));
  ELP_LAUNCH(c, "material_values", k_material_values, dim3(std::min(blocks_for(w.nu, 256), 1024u)), dim3(256), 0, w.nu, (const uint32_t *)w.u_read, pl, w.maxq, d_vals, w.t);
  std::vector<uint32_t> hv((size_t)pl.n * 8);
  ELP_HIP(c, hipMemcpyAsync(hv.data(), d_vals, hv.size() * 4, hipMemcpyDeviceToHost, c->stream));
  ELP_HIP(c, elp::stream_wait(c->stream));
  *f = tie_fields(lp, hv.data());
  ELP_HIP(c, hipMemcpyAsync(d_lut, f->lut.data(), f->lut.size(), hipMemcpyHostToDevice, c->stream));
  w.d_lut = d_lut;
  return 0;
}

static TiePacked tie_packed(const RankFields &f, FieldCut cut) {
  TiePacked sel;
  memset(&sel, 0, sizeof sel);
  for (int k = cut.lo; k < cut.hi; k++, sel.n++) { sel.pos[sel.n] = f.pos[k]; sel.slot[sel.n] = (uint8_t)f.slot[k]; }
  field_shifts(f.bits, cut, sel.shift);
  return sel;
}
// one stable round of the members on the low `digits` bytes of the keys in uk0
static int tie_round_sort(elp_ctx *c, TieWork &w, int digits, uint64_t **ko) {
  uint32_t *vo;
  ELP_TRY(radix_sort_pairs_low(c, w.uk0, w.vcur, w.uk1, w.vtmp, w.nu, digits, ko, &vo));
  if (vo != w.vcur) { w.vtmp = w.vcur; w.vcur = vo; }
  return 0;
}
static int tie_scatter(elp_ctx *c, TieWork &w) {
  ELP_LAUNCH(c, "large_scatter", k_large_scatter, dim3(blocks_for(w.nu, 256)), dim3(256), 0, w.nu, (const uint32_t *)w.vcur, (const uint32_t *)w.u_pos,
             (const uint32_t *)w.u_read, c->perm.p);
  return 0;
}

// ONE round if everything fits a key, or on the most significant positions that do, with the rest settled by comparison inside the
// groups of equal keys (k_large_ties); the run id rides in front of the key (no last round on it).  *settled = the permutation is
// written; else a group of > LT_CAP equal keys was found: the rounds over all positions follow, from the members' first order.
static int tie_key_round(elp_ctx *c, TieWork &w, const RankFields &f, bool *settled) {
  const uint32_t nu = w.nu;
  const int sb = segbits(w.nr);
  const FieldCut cut = pack_prefix(f.bits, sb);
  const TiePacked sel = tie_packed(f, cut);
  ELP_LAUNCH(c, "material_keys", k_material_keys_packed, dim3(blocks_for(nu, 256)), dim3(256), 0, nu, (const uint32_t *)w.vcur, (const uint32_t *)w.u_read,
             sel, w.d_lut, w.maxq, w.uk0, w.t, (const uint32_t *)(w.nr > 1 ? w.u_seg : nullptr), (uint32_t)cut.total);
  uint64_t *ko;
  ELP_TRY(tie_round_sort(c, w, key_digits(sb + cut.total), &ko));
  *settled = cut.hi == f.n();  // every live position is in the key: equal keys are equal strings, the stable passes kept their order
  if (*settled) return tie_scatter(c, w);
  uint32_t *over = c->err_flag.p + 3;  // the scan-total mailbox (zero here)
  ELP_LAUNCH(c, "large_ties", k_large_ties, dim3(blocks_for(nu, 256)), dim3(256), 0, nu, (const uint64_t *)ko, (const uint32_t *)w.vcur, w.vtmp,
             (const uint32_t *)w.u_read, w.lay.m_bytes, w.maxq, over, w.t);
  std::swap(w.vcur, w.vtmp);
  ELP_TRY(tie_scatter(c, w));
  uint32_t h_over = 0;
  ELP_HIP(c, hipMemcpyAsync(&h_over, over, 4, hipMemcpyDeviceToHost, c->stream));
  ELP_HIP(c, elp::stream_wait(c->stream));
  *settled = h_over == 0;
  if (!*settled) {
    ELP_HIP(c, hipMemsetAsync(over, 0, 4, c->stream));
    ELP_LAUNCH(c, "iota", k_iota, dim3(blocks_for(nu, 256)), dim3(256), 0, w.uv0, (uint64_t)nu);
    w.vcur = w.uv0; w.vtmp = w.uv1;
  }
  return 0;
}

// rounds on the ranks from the least significant position upwards, each filling at most 64 bits / 64 positions
static int tie_packed_rounds(elp_ctx *c, TieWork &w, const RankFields &f) {
  for (const FieldCut &cut : lsd_cuts(f.bits)) {
    const TiePacked sel = tie_packed(f, cut);
    ELP_LAUNCH(c, "material_keys", k_material_keys_packed, dim3(blocks_for(w.nu, 256)), dim3(256), 0, w.nu, (const uint32_t *)w.vcur, (const uint32_t *)w.u_read,
               sel, w.d_lut, w.maxq, w.uk0, w.t, (const uint32_t *)nullptr, 0u);
    uint64_t *ko;
    ELP_TRY(tie_round_sort(c, w, key_digits(cut.total), &ko));
  }
  return 0;
}

// more live positions than the rank keys take (or none at all: no round): rounds on the bytes, least significant positions first
static int tie_byte_rounds(elp_ctx *c, TieWork &w, const std::vector<uint16_t> &lp) {
  for (const FieldCut &cut : byte_cuts(lp.size())) {
    TieSel sel;
    sel.n = (uint32_t)(cut.hi - cut.lo);
    for (size_t b = 0; b < 8; b++) sel.pos[b] = b < sel.n ? lp[cut.lo + b] : 0;
    ELP_LAUNCH(c, "material_keys", k_material_keys_sel, dim3(blocks_for(w.nu, 256)), dim3(256), 0, w.nu, (const uint32_t *)w.vcur,
               (const uint32_t *)w.u_read, sel, w.maxq, w.uk0, w.t);
    uint64_t *ko;
    ELP_TRY(tie_round_sort(c, w, (int)sel.n, &ko));
  }
  return 0;
}

// the last, stable round on the run id keeps the runs apart and in order - with ONE long run (the unmapped block of a file without
// pile-ups) there is nothing to keep apart
static int tie_run_id_round(elp_ctx *c, TieWork &w) {
  if (w.nr > 1) ELP_LAUNCH(c, "seg_keys", k_seg_keys, dim3(blocks_for(w.nu, 256)), dim3(256), 0, w.nu, (const uint32_t *)w.vcur, (const uint32_t *)w.u_seg, w.uk0);
  if (w.nr > 1) {
    uint64_t *ko;
    uint32_t *vo;
    ELP_TRY(radix_sort_pairs(c, w.uk0, w.vcur, w.uk1, w.vtmp, w.nu, &ko, &vo));
    if (vo != w.vcur) { w.vtmp = w.vcur; w.vcur = vo; }
  }
  return tie_scatter(c, w);
}

static int tie_long_runs(elp_ctx *c, TieWork &w, const LongRuns &runs) {
  std::vector<uint16_t> lp;
  ELP_TRY(tie_members(c, w, runs, &lp));
  if (rank_keys_apply(lp.size())) {
    RankFields f;
    ELP_TRY(tie_rank_tables(c, w, lp, &f));
    if (key_then_compare(c->tune.tie_rounds, segbits(w.nr), f.bits[0])) {
      bool settled = false;
      ELP_TRY(tie_key_round(c, w, f, &settled));
      if (settled) return 0;
    }
    ELP_TRY(tie_packed_rounds(c, w, f));
  } else {
    ELP_TRY(tie_byte_rounds(c, w, lp));
  }
  return tie_run_id_round(c, w);
}

static int sort_impl(elp_ctx *c, uint64_t *presorted = nullptr /* the key passes' result, made ahead (sort_presort) */) {
  const uint64_t n = c->n;
  ELP_TRY(ensure_keys(c));
  ELP_TRY(ensure(c, c->perm, n + 1));
  if (n == 0) { c->derived.set_sorted(false); return 0; }
  TieWork w(n);
  ELP_TRY(sort_key_passes(c, presorted, w));
  ELP_TRY(tie_short_runs(c, w));
  LongRuns runs;
  ELP_TRY(tie_read_bounds(c, w, &runs));
  if (runs.nr > 0) ELP_TRY(tie_long_runs(c, w, runs));
  // (a look-back that timed out leaves a wrong permutation: the bit is read by whoever reads the error words next - the following
  // stage, elp_sync, elp_get_permutation, the emit calls: fetch_err - instead of a synchronisation of its own here)
  c->radix_check_pending = true;
  c->derived.set_sorted(false);
  return 0;
}

// The sort on the context's side lane 1 (common.hpp): the shadow context sees the key column, the comparator's columns and the
// permutation's buffer as views for the duration of the call, runs on its own stream behind what the context's stream holds now, and
// before it returns the context's stream is made to wait for whatever the lane still has queued - later stages find the permutation.
static int sort_on_side(elp_ctx *c) {
  ELP_TRY(ensure_keys(c));  // (on the context: the shadow takes the key column as it is)
  ELP_TRY(ensure(c, c->perm, c->n + 1));
  elp_ctx *s = nullptr;
  ELP_TRY(side_lane(c, 1, &s));
  s->n = c->n; s->n_sr = c->n_sr; s->n_filtered = c->n_filtered; s->key_bits = c->key_bits; s->max_qname_len = c->max_qname_len; s->max_pos = c->max_pos;
  s->n_ref = c->n_ref;
  s->derived = elp::Derived{};
  s->derived.keys = true;  // (of what the context has derived the shadow sees the key column, nothing else)
  // the key passes may have been queued ahead (elp_sort_ahead, from inside elp_mark_duplicates): same keys, same length, same lane
  const bool pre_ok = c->presort_ks && c->derived.presorted && c->presort_n == c->n && c->presort_idx_bits == index_bits(c->n) && c->tune.sort_pairs != 1;
  uint64_t *pre = pre_ok ? c->presort_ks : nullptr;
  c->derived.drop_presort();  // (used once: the tie-break leaves its marks in the buffer's other half)
  int rc;
  {
    LaneViews views(s, c, &elp_ctx::key, &elp_ctx::flag, &elp_ctx::mapq, &elp_ctx::next_refid, &elp_ctx::pnext, &elp_ctx::tlen, &elp_ctx::qname_off,
                    &elp_ctx::qname, &elp_ctx::has_sr);
    views.view(s->perm, c->perm, true);
    rc = sort_impl(s, pre);
  }
  if (rc == 0) rc = radix_check(s);  // (the lane's own error words: nothing of the sort stays unread)
  if (rc != 0) {
    (void)elp::stream_wait(s->stream);
    c->err = s->err;
    return rc;
  }
  ELP_TRY(side_join(c, 1));
  c->derived.set_sorted(false);
  return 0;
}

int sort_presort(elp_ctx *c) {
  const uint64_t n = c->n;
  c->derived.drop_presort();
  if (!c->sort_ahead || n < 2 || !c->derived.keys) return 0;
  const int idx_bits = index_bits(n);
  if (!sort_words(c->key_bits, idx_bits, c->tune.sort_pairs)) return 0;  // (pairs, not words: the sort makes its passes itself)
  elp_ctx *s = nullptr;
  ELP_TRY(side_lane(c, 1, &s));
  s->n = n; s->key_bits = c->key_bits;
  const int tile_saved = s->tune.radix_tile;
  if (!s->tune.radix_tile) s->tune.radix_tile = c->tune.presort_tile >= 1 && c->tune.presort_tile <= 3 ? c->tune.presort_tile : 2;
  uint64_t *kbuf, *ks = nullptr;
  int rc = scratch(s, 0, SortScratch(n).keys, &kbuf);
  if (rc == 0) rc = radix_sort_fused(s, c->key.p, n, c->key_bits, idx_bits, kbuf, kbuf + n, &ks);
  s->tune.radix_tile = tile_saved;
  if (rc != 0) { c->err = s->err; return rc; }
  c->presort_ks = ks; c->presort_n = n; c->presort_idx_bits = idx_bits; c->derived.presorted = true;
  return 0;
}
}  // namespace elp

extern "C" int elp_sort_ahead(elp_ctx *c, int on) {
  if (!c) return ELP_ERR_ARG;
  c->sort_ahead = on != 0;
  if (!on) c->derived.drop_presort();
  return 0;
}

extern "C" int elp_sort_coordinate(elp_ctx *c) {
  if (!c) return ELP_ERR_ARG;
  ELP_HIP(c, hipSetDevice(c->device));
  c->derived.drop_sorted();
  return elp::sort_on_side(c);
}
