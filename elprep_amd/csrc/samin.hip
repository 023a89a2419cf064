// samin.hip — SAM text IN on the device (elp_stage_sam): parseSamAlignment (sam/sam-files.go:386-410) + AddREFID
// (filters/simple-filters.go:208-231) + formatBamAlignment (sam/bam-files.go:635-737) as kernels.  Every alignment line becomes the BAM
// record the reference would write for it, in c->raw with its offset in c->raw_off; stage_bam_columns (bam_in.hip) then cuts the records
// into the columns as it does for elp_stage_bam and elp_stage_bgzf - whatever reads staged records reads these.
//
// Per piece of text (whole lines, at most PIECE bytes):
//   line starts   newlines counted per tile of 4096 bytes, scanned, the starts scattered (k_sam_count_nl, k_sam_starts)
//   size pass     one wavefront per line (k_sam_lines<false>): the tabs are found by ballots over 64-byte chunks and kept in LDS, the
//                 line is validated and its record's exact size computed; the first refusal of the piece is kept as one word
//                 (line << 8 | reason) by atomic minimum.  Nothing of a piece is committed before its size pass has passed.
//   write pass    the same walk (k_sam_lines<true>) writes the record behind the exclusive scan of the sizes.
// Who does what in the wave: the five mandatory numbers and the two name look-ups each by a lane of their own; the CIGAR by one lane per
// operation character (its digits lie in front of it; the lane that begins a run of equal operations adds the run up); QNAME, SEQ
// nibble pairs and QUAL lane-parallel; one lane per optional field for its frame and scalar value; Z values and B arrays by the whole
// wave, a B array with one lane per entry (an entry begins behind a comma found by ballot).  The token parsers are samparse.hpp's.
#include <algorithm>

#include "common.hpp"
#include "bamtag.hpp"
#include "bamout.hpp"
#include "samparse.hpp"

namespace elp {

using namespace samparse;

constexpr uint32_t NL_TILE = 4096;  // bytes per workgroup of the line-start kernels (256 threads x 16 rounds)

__global__ __launch_bounds__(256) void k_sam_count_nl(const uint8_t *__restrict__ text, uint32_t n, uint32_t *__restrict__ cnt) {
  __shared__ uint32_t total;
  if (threadIdx.x == 0) total = 0;
  __syncthreads();
  const uint32_t t0 = blockIdx.x * NL_TILE;
  uint32_t mine = 0;
  for (uint32_t r = 0; r < NL_TILE / 256; r++) {
    const uint32_t p = t0 + r * 256 + threadIdx.x;
    mine += (p < n && text[p] == '\n') ? 1u : 0u;
  }
  if (mine) atomicAdd(&total, mine);
  __syncthreads();
  if (threadIdx.x == 0) cnt[blockIdx.x] = total;
}
// starts[k + 1] = the byte behind the k-th newline of the piece; starts[0] = 0 (the host sets the entry behind a last line without one)
__global__ __launch_bounds__(256) void k_sam_starts(const uint8_t *__restrict__ text, uint32_t n, const uint32_t *__restrict__ base, uint32_t *__restrict__ starts) {
  __shared__ uint32_t wave_cnt[4];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t t0 = blockIdx.x * NL_TILE;
  uint32_t running = base[blockIdx.x];
  if (blockIdx.x == 0 && threadIdx.x == 0) starts[0] = 0;
  for (uint32_t r = 0; r < NL_TILE / 256; r++) {
    const uint32_t p = t0 + r * 256 + threadIdx.x;
    const bool nl = p < n && text[p] == '\n';
    const unsigned long long b = __ballot(nl);
    if (lane == 0) wave_cnt[wave] = (uint32_t)__popcll(b);
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (uint32_t w = 0; w < 4; w++) {
      const uint32_t c = wave_cnt[w];
      before += w < wave ? c : 0u;
      all += c;
    }
    if (nl) starts[1 + running + before + (uint32_t)__popcll(b & ((1ull << lane) - 1ull))] = p + 1;
    running += all;
    __syncthreads();
  }
}

// FNV-1a over a reference name: the host fills the table with it, the kernels probe with it
__host__ __device__ inline uint32_t name_hash(const uint8_t *s, uint32_t n) {
  uint32_t h = 2166136261u;
  for (uint32_t k = 0; k < n; k++) h = (h ^ s[k]) * 16777619u;
  return h;
}

struct SamIn {
  const uint8_t *text;       // the piece (device copy)
  const uint32_t *starts;    // line k of the piece = text[starts[k] .. starts[k + 1] - 1), a carriage return in front of the newline dropped
  uint32_t line0, n_lines;   // the lines of this launch: line0 .. line0 + n_lines
  uint32_t *sizes;           // size pass: per line of the piece, the record's bytes (block_size field included); 0 for a refused line
  unsigned long long *err;   // size pass: min over the refused lines of (line << 8 | reason); starts as ~0
  uint32_t *max_size;        // size pass: the largest record
  const uint32_t *offs;      // write pass: exclusive scan of sizes[line0 ..]
  uint8_t *out;              // write pass: where the pass's records go (c->raw + its fill level)
  uint64_t *raw_off;         // write pass: c->raw_off + c->n
  uint64_t raw_base;         // write pass: the fill level of c->raw in front of the pass
  const uint8_t *names;      // the dictionary: names, offsets, the look-up table (slot = refid + 1, 0 = empty)
  const uint32_t *name_off, *slots;
  uint32_t slot_mask;
  int32_t n_ref;
};

constexpr int32_t REF_SAME = 0x7FFFFFFE;  // RNEXT "=": RNAME's refid, taken once both lanes are back
__device__ inline int32_t name_lookup(const SamIn &m, const uint8_t *s, uint32_t n, bool is_next, uint32_t *err) {
  if (n == 1 && s[0] == '*') return -1;
  if (n == 1 && s[0] == '=') return is_next ? REF_SAME : -1;  // (RNAME "=": AddREFID finds no such contig)
  if (m.n_ref > 0) {
    for (uint32_t h = name_hash(s, n) & m.slot_mask;; h = (h + 1u) & m.slot_mask) {
      const uint32_t slot = m.slots[h];
      if (!slot) break;
      const uint32_t o = m.name_off[slot - 1u];
      if (m.name_off[slot] - o != n) continue;
      bool eq = true;
      for (uint32_t k = 0; k < n; k++) eq &= m.names[o + k] == s[k];
      if (eq) return (int32_t)(slot - 1u);
    }
  }
  *err = R_NAME_UNKNOWN;
  return -1;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

// one wavefront (= one workgroup) per line; WRITE = false: the size pass, true: the write pass
template <bool WRITE>
__global__ __launch_bounds__(64) void k_sam_lines(SamIn m) {
  __shared__ uint32_t tabs[MAX_TABS];   // positions of the line's tabs
  __shared__ uint16_t keys[MAX_TABS];   // keys of the optional fields seen so far
  const uint32_t lane = threadIdx.x;
  const unsigned long long lt = (1ull << lane) - 1ull;
  for (uint32_t j = blockIdx.x; j < m.n_lines; j += gridDim.x) {
    const uint32_t li = m.line0 + j;
    const uint32_t at = m.starts[li];
    uint32_t len = m.starts[li + 1] - 1u - at;
    const uint8_t *L = m.text + at;
    if (len && L[len - 1] == '\r') len--;
    uint32_t err = 0;    // this lane's first refusal; the lowest lane's decides the line's
    uint32_t size = 0;   // the record's bytes (wave-uniform)
    uint8_t *o = nullptr;
    if constexpr (WRITE) o = m.out + m.offs[j];
    __syncthreads();  // (the lanes of the line before have read what this one overwrites)
    do {
      if (len > MAX_LINE) { err = R_LINE_LONG; break; }
      // ---- tabs
      uint32_t ntabs = 0, n_nul = 0;
      for (uint32_t base = 0; base < len; base += 64) {
        const uint32_t p = base + lane;
        const uint8_t ch = p < len ? L[p] : (uint8_t)'x';
        const unsigned long long b = __ballot(ch == '\t');
        n_nul += (uint32_t)__popcll(__ballot(p < len && ch == 0));
        if (ch == '\t') {
          const uint32_t idx = ntabs + (uint32_t)__popcll(b & lt);
          if (idx < MAX_TABS) tabs[idx] = p;
        }
        ntabs += (uint32_t)__popcll(b);
      }
      __syncthreads();
      if (ntabs < 10) { err = R_MISSING_TAB; break; }
      if (ntabs >= MAX_TABS) { err = R_FIELDS_MANY; break; }
      auto fstart = [&](uint32_t f) { return f ? tabs[f - 1] + 1u : 0u; };
      auto fend = [&](uint32_t f) { return f < ntabs ? tabs[f] : len; };
      uint32_t nfields = ntabs + 1;
      if (nfields > 11 && tabs[ntabs - 1] + 1u == len) nfields--;  // a tab behind the last field: the scanner is at its end, no field follows
      // ---- the mandatory numbers and names: a lane each
      uint32_t val = 0;
      if (lane < 11) {
        const uint32_t a = fstart(lane), n = fend(lane) - a;
        int64_t v = 0;
        switch (lane) {
          case 1: if (!parse_int(L + a, n, 16, false, &v)) err = R_FLAG; break;
          case 3: if (!parse_int(L + a, n, 32, true, &v)) err = R_POS; break;
          case 4: if (!parse_int(L + a, n, 8, false, &v)) err = R_MAPQ; break;
          case 7: if (!parse_int(L + a, n, 32, true, &v)) err = R_PNEXT; break;
          case 8: if (!parse_int(L + a, n, 32, true, &v)) err = R_TLEN; break;
          case 2: v = name_lookup(m, L + a, n, false, &err); break;
          case 6: v = name_lookup(m, L + a, n, true, &err); break;
          default: break;
        }
        val = (uint32_t)v;
      }
      const uint32_t flag = __shfl(val, 1), mapq = __shfl(val, 4);
      const int32_t refid = (int32_t)__shfl(val, 2), pos = (int32_t)__shfl(val, 3), pnext = (int32_t)__shfl(val, 7), tlen = (int32_t)__shfl(val, 8);
      int32_t next_refid = (int32_t)__shfl(val, 6);
      if (next_refid == REF_SAME) next_refid = refid;
      // ---- QNAME
      const uint32_t lq = fend(0);
      if (lq > 254) { err = R_QNAME_LONG; break; }
      if (n_nul)
        for (uint32_t k = lane; k < lq; k += 64)
          if (L[k] == 0 && !err) err = R_QNAME_NUL;
      if constexpr (WRITE)
        for (uint32_t k = lane; k <= lq; k += 64) o[36 + k] = k < lq ? L[k] : (uint8_t)0;
      // ---- CIGAR: a lane per operation character
      const uint32_t c0 = fstart(5), c1 = fend(5);
      uint32_t n_ops = 0, ref_span = 0;
      if (c1 > c0 && !(c1 - c0 == 1 && L[c0] == '*')) {
        uint32_t prev_end = c0, prev_op = 0xFFu;  // behind the last operation character of the chunks in front, and its operation
        for (uint32_t base = c0; base < c1; base += 64) {
          const uint32_t p = base + lane;
          const bool in = p < c1;
          const uint8_t ch = in ? L[p] : (uint8_t)'0';
          const bool opc = in && !is_digit(ch);
          const unsigned long long b = __ballot(opc);
          bool begins = false;
          uint32_t merged = 0, op = 0xFFu;
          if (opc) {
            const unsigned long long below = b & lt;
            const uint32_t q = below ? base + 64u - (uint32_t)__builtin_clzll(below) : prev_end;  // where this token's digits begin
            const uint32_t before = below ? cigar_op_code(L[q - 1]) : prev_op;
            uint32_t tl = 0;
            uint32_t r = cigar_token(L, q, p, &tl, &op);
            if (!r && op != before) {
              begins = true;
              r = cigar_run(L, p, c1, op, tl, &merged);
            }
            if (r && !err) err = r;
          }
          const unsigned long long bb = __ballot(begins);
          if constexpr (WRITE) {
            if (begins) {
              st_u32(o + 36 + lq + 1 + 4 * (n_ops + (uint32_t)__popcll(bb & lt)), (merged << 4) | op);
              if (op_consumes_ref(op)) ref_span += merged;
            }
          }
          n_ops += (uint32_t)__popcll(bb);
          if (b) {
            prev_end = base + 64u - (uint32_t)__builtin_clzll(b);
            prev_op = cigar_op_code(L[prev_end - 1]);
          }
        }
        if (prev_end != c1) { err = R_CIGAR; break; }  // digits without an operation
        if (n_ops > 65535u) { err = R_CIGAR_OPS; break; }
        if constexpr (WRITE) ref_span = wave_sum(ref_span);
      }
      // ---- SEQ and QUAL
      const uint32_t s0 = fstart(9), l_seq = fend(9) - s0, q0 = fstart(10);
      if (fend(10) - q0 != l_seq) { err = R_QUAL_LENGTH; break; }
      const uint32_t seqb = (l_seq + 1) >> 1;
      const uint32_t fixed = 36 + lq + 1 + 4 * n_ops + seqb + l_seq;
      if constexpr (WRITE) {
        uint8_t *w = o + 36 + lq + 1 + 4 * n_ops;
        for (uint32_t k = lane; k < seqb; k += 64) {
          const uint32_t hi = base_nibble(L[s0 + 2 * k]), lo = 2 * k + 1 < l_seq ? base_nibble(L[s0 + 2 * k + 1]) : 0u;
          w[k] = (uint8_t)((hi << 4) | lo);
        }
        w += seqb;
        for (uint32_t k = lane; k < l_seq; k += 64) w[k] = (uint8_t)(L[q0 + k] - 33u);
      }
      // ---- optional fields: a lane per field, 64 fields a round
      const uint32_t nopt = nfields - 11;
      uint32_t tag_off = fixed;  // where the round's first field goes
      for (uint32_t r0 = 0; r0 < nopt; r0 += 64) {
        const uint32_t fi = r0 + lane;
        const bool act = fi < nopt;
        uint32_t a = 0, e = 0, v0 = 0, vn = 0, fsz = 0, key = 0, fbits = 0, es = 0, bcnt = 0;
        uint8_t ty = 0, ity = 0;
        int64_t iv = 0;
        if (act) {
          a = fstart(11 + fi);
          e = fend(11 + fi);
          uint32_t r = 0;
          if (e - a < 5 || L[a] == ':' || L[a + 1] == ':' || L[a + 2] != ':' || L[a + 4] != ':') {
            r = R_FIELD;
          } else {
            ty = L[a + 3];
            v0 = a + 5;
            vn = e - v0;
            key = (uint32_t)L[a] | ((uint32_t)L[a + 1] << 8);
            keys[fi] = (uint16_t)key;
            switch (ty) {
              case 'A': if (vn != 1) r = R_FIELD_A; fsz = 4; break;
              case 'i':
                if (!parse_int(L + v0, vn, 64, true, &iv)) r = R_FIELD_INT;
                else if (iv < -2147483648ll || iv > 4294967295ll) r = R_FIELD_INT_RANGE;
                else fsz = 3 + int_store(iv, &ity);
                break;
              case 'f': r = parse_f32(L + v0, vn, &fbits); fsz = 7; break;
              case 'Z': fsz = 4 + vn; break;
              case 'H': r = R_FIELD_H; break;
              case 'B':
                es = vn >= 2 && L[v0 + 1] == ',' ? elem_size(L[v0]) : 0u;
                if (!es) r = R_FIELD_B;
                break;
              default: r = R_FIELD_TYPE; break;
            }
          }
          if (r) { ty = 0; fsz = 0; if (!err) err = r; }
        }
        __syncthreads();
        if (act && ty) {
          for (uint32_t k = 0; k < fi; k++)
            if (keys[k] == (uint16_t)key) { if (!err) err = R_FIELD_TWICE; break; }
        }
        // B arrays: the entries are the commas (the first stands behind the subtype)
        for (unsigned long long bm = __ballot(act && ty == 'B'); bm; bm &= bm - 1) {
          const int owner = __builtin_ctzll(bm);
          const uint32_t fa = __shfl(v0, owner) + 1u, fe = __shfl(e, owner);
          uint32_t cnt = 0;
          for (uint32_t base = fa; base < fe; base += 64) {
            const uint32_t p = base + lane;
            cnt += (uint32_t)__popcll(__ballot(p < fe && L[p] == ','));
          }
          if ((int)lane == owner) { bcnt = cnt; fsz = 8 + cnt * es; }
        }
        // where each field goes: exclusive prefix sum of the sizes
        uint32_t incl = fsz;
        for (uint32_t d = 1; d < 64; d <<= 1) {
          const uint32_t up = __shfl_up(incl, d);
          if (lane >= d) incl += up;
        }
        const uint32_t my_off = tag_off + incl - fsz;
        tag_off += __shfl(incl, 63);
        if constexpr (WRITE) {
          if (act && ty) {
            uint8_t *w = o + my_off;
            w[0] = L[a]; w[1] = L[a + 1]; w[2] = ty == 'i' ? ity : ty;
            if (ty == 'A') w[3] = L[v0];
            else if (ty == 'i') { for (uint32_t b = 0; b + 3 < fsz; b++) w[3 + b] = (uint8_t)((uint64_t)iv >> (8 * b)); }
            else if (ty == 'f') st_u32(w + 3, fbits);
            else if (ty == 'Z') w[3 + vn] = 0;
            else { w[3] = L[v0]; st_u32(w + 4, bcnt); }
          }
        }
        // Z values (write pass; size pass only where the line holds a NUL) and the entries of B arrays: the whole wave on one field
        for (unsigned long long cm = __ballot(act && (ty == 'B' || (ty == 'Z' && (WRITE || n_nul)))); cm; cm &= cm - 1) {
          const int owner = __builtin_ctzll(cm);
          const uint32_t fty = __shfl((uint32_t)ty, owner), fv = __shfl(v0, owner), fe = __shfl(e, owner), foff = __shfl(my_off, owner);
          if (fty == 'Z') {
            bool nul = false;
            for (uint32_t k = lane; k < fe - fv; k += 64) {
              const uint8_t ch = L[fv + k];
              nul |= ch == 0;
              if constexpr (WRITE) o[foff + 3 + k] = ch;
            }
            if (__ballot(nul) && (int)lane == owner && !err) err = R_FIELD_Z_NUL;
          } else {
            const uint8_t sub = L[fv];
            const uint32_t esz = elem_size(sub);
            uint32_t cnt = 0;
            for (uint32_t base = fv + 1; base < fe; base += 64) {
              const uint32_t p = base + lane;
              const bool comma = p < fe && L[p] == ',';
              const unsigned long long b = __ballot(comma);
              if (comma) {
                uint32_t q = p + 1;
                while (q < fe && L[q] != ',') q++;
                uint32_t v = 0;
                const uint32_t r = parse_entry(sub, L + p + 1, q - p - 1, &v);
                if (r) { if (!err) err = r; }
                else if constexpr (WRITE) {
                  uint8_t *w = o + foff + 8 + (cnt + (uint32_t)__popcll(b & lt)) * esz;
                  for (uint32_t k = 0; k < esz; k++) w[k] = (uint8_t)(v >> (8 * k));
                }
              }
              cnt += (uint32_t)__popcll(b);
            }
          }
        }
        __syncthreads();
      }
      size = tag_off;
      if constexpr (WRITE) {
        if (lane == 0) {
          st_u32(o, size - 4);
          st_u32(o + 4, (uint32_t)refid);
          st_u32(o + 8, (uint32_t)pos - 1u);
          o[12] = (uint8_t)(lq + 1);
          o[13] = (uint8_t)mapq;
          st_u16(o + 14, record_bin((uint16_t)flag, (int32_t)((uint32_t)pos - 1u), ref_span));
          st_u16(o + 16, n_ops);
          st_u16(o + 18, flag);
          st_u32(o + 20, l_seq);
          st_u32(o + 24, (uint32_t)next_refid);
          st_u32(o + 28, (uint32_t)pnext - 1u);
          st_u32(o + 32, (uint32_t)tlen);
          m.raw_off[j] = m.raw_base + m.offs[j];
        }
      }
    } while (false);
    if constexpr (!WRITE) {
      const unsigned long long eb = __ballot(err != 0);
      const uint32_t reason = eb ? __shfl(err, __builtin_ctzll(eb)) : 0u;
      if (lane == 0) {
        m.sizes[li] = reason ? 0u : size;
        if (reason) atomicMin(m.err, ((unsigned long long)li << 8) | reason);
        else if (size > *(volatile uint32_t *)m.max_size) atomicMax(m.max_size, size);  // (a look first: one atomic per line on ONE word is a queue)
      }
    }
  }
}

// the look-up table of the names in force, made once per set of names
static int ensure_name_table(elp_ctx *c) {
  if (c->have_ref_name_table) return 0;
  uint32_t slots = 2;
  while (slots < 2u * (uint32_t)c->n_ref + 2u) slots <<= 1;
  std::vector<uint32_t> table(slots, 0u);
  const uint8_t *names = reinterpret_cast<const uint8_t *>(c->h_ref_names.data());
  for (int32_t r = 0; r < c->n_ref; r++) {
    const uint32_t o = c->h_ref_names_off[(size_t)r], n = c->h_ref_names_off[(size_t)r + 1] - o;
    uint32_t h = name_hash(names + o, n) & (slots - 1);
    while (table[h]) h = (h + 1u) & (slots - 1);  // (the names are distinct: elp_set_reference_names_flat)
    table[h] = (uint32_t)r + 1u;
  }
  ELP_TRY(ensure(c, c->ref_name_slots, slots));
  ELP_HIP(c, hipMemcpyAsync(c->ref_name_slots.p, table.data(), (size_t)slots * 4, hipMemcpyHostToDevice, c->stream));
  ELP_HIP(c, elp::stream_wait(c->stream));
  c->ref_name_mask = slots - 1;
  c->have_ref_name_table = true;
  return 0;
}

}  // namespace elp

using namespace elp;

extern "C" {

int elp_stage_sam(elp_ctx *c, const uint8_t *text, uint64_t n_bytes, uint16_t split_id) {
  if (!c || (!text && n_bytes)) return ELP_ERR_ARG;
  std::lock_guard<std::mutex> g(c->stage_mu);
  ELP_HIP(c, hipSetDevice(c->device));
  if (!c->have_header) return set_error(c, ELP_ERR_ARG, "elp_stage_sam: call elp_set_header first");
  if (c->dict_replaced) return staging_refused_after_replace(c, "elp_stage_sam");
  if (c->n_rg && !c->have_rg_ids && !c->replace_rg) return set_error(c, ELP_ERR_ARG, "elp_stage_sam: call elp_set_read_group_ids first");
  if (!c->have_ref_names) return set_error(c, ELP_ERR_ARG, "elp_stage_sam: call elp_set_reference_names_flat first (RNAME and RNEXT are looked up in the names)");
  if (c->n != c->raw_n) return set_error(c, ELP_ERR_ARG, "elp_stage_sam: the context already holds records staged with elp_stage");
  ELP_TRY(ensure_name_table(c));
  hipStream_t st = c->stream;
  // pieces are committed one at a time, as elp_stage_bam's: what was derived from the records staged so far is invalid from here on, also
  // if a later piece is refused (the pieces in front of it stay staged)
  c->derived.records_changed();
  if (!c->copy_stream) ELP_HIP(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
  hipPointerAttribute_t pa;
  const bool pinned = n_bytes && hipPointerGetAttributes(&pa, text) == hipSuccess && pa.type == hipMemoryTypeHost;
  (void)hipGetLastError();
  constexpr uint64_t PIECE = 256ull << 20;  // device work unit: <= 256 MiB of text + the line that crosses its end (u32 offsets and scans:
                                            // a record is at most twice its line + 40 bytes, a line that passes at least 21 bytes)
  constexpr size_t BOUNCE = 32ull << 20;
  if (!pinned && n_bytes && !c->bounce[0]) {
    for (int k = 0; k < 2; k++) {
      ELP_HIP(c, hipHostMalloc(&c->bounce[k], BOUNCE, hipHostMallocDefault));
      ELP_HIP(c, hipEventCreateWithFlags(&c->bounce_ev[k], hipEventDisableTiming));
    }
  }
  uint64_t at_byte = 0, lines_before = 0;
  while (at_byte < n_bytes) {
    // the piece ends behind the first newline at or behind PIECE bytes (a line is refused above 1 MiB, so the search is short)
    uint64_t end = n_bytes;
    if (n_bytes - at_byte > PIECE) {
      const void *nl = memchr(text + at_byte + PIECE - 1, '\n', (size_t)std::min<uint64_t>(n_bytes - (at_byte + PIECE - 1), (uint64_t)MAX_LINE + 2));
      if (nl) end = (uint64_t)(static_cast<const uint8_t *>(nl) - text) + 1;
      else if (n_bytes - (at_byte + PIECE - 1) > (uint64_t)MAX_LINE + 2) return set_error(c, ELP_ERR_DATA, "elp_stage_sam: line longer than 1 MiB near byte %llu", (unsigned long long)(at_byte + PIECE));
    }
    const uint32_t pb = (uint32_t)(end - at_byte);
    const bool open_end = text[end - 1] != '\n';  // a last line without a newline counts
    uint8_t *d_text;
    ELP_TRY(scratch(c, 5, (size_t)pb + 64, &d_text));
    if (pinned) {
      ELP_HIP(c, hipMemcpyAsync(d_text, text + at_byte, pb, hipMemcpyHostToDevice, st));
    } else {
      ELP_HIP(c, elp::stream_wait(st));  // (the kernels of the piece before read the buffer the copies overwrite)
      int k = 0;
      for (uint64_t o = 0; o < pb; o += BOUNCE, k ^= 1) {
        const size_t len = (size_t)std::min<uint64_t>(BOUNCE, pb - o);
        ELP_HIP(c, hipEventSynchronize(c->bounce_ev[k]));
        memcpy(c->bounce[k], text + at_byte + o, len);
        ELP_HIP(c, hipMemcpyAsync(d_text + o, c->bounce[k], len, hipMemcpyHostToDevice, c->copy_stream));
        ELP_HIP(c, hipEventRecord(c->bounce_ev[k], c->copy_stream));
      }
      ELP_HIP(c, elp::stream_wait(c->copy_stream));
    }
    // line starts
    const uint32_t tiles = blocks_for(pb, NL_TILE);
    uint32_t *tile_cnt;
    ELP_TRY(scratch(c, 6, (size_t)2 * (tiles + 8), &tile_cnt));
    uint32_t *tile_base = tile_cnt + tiles + 8;
    ELP_LAUNCH(c, "stage_sam_count", k_sam_count_nl, dim3(tiles), dim3(256), 0, (const uint8_t *)d_text, pb, tile_cnt);
    uint32_t n_nl = 0;
    ELP_TRY(exclusive_scan_u32(c, tile_cnt, tile_base, tiles, &n_nl));
    ELP_HIP(c, elp::stream_wait(st));  // (n_nl)
    const uint32_t n_lines = n_nl + (open_end ? 1u : 0u);
    if (c->n + n_lines > 0xFFFFFFF0ull) return set_error(c, ELP_ERR_UNSUPPORTED, "more than 2^32-16 records per context");
    // starts (n_lines + 1) | sizes | offsets, and the error and maximum words
    uint32_t *wk;
    ELP_TRY(scratch(c, 7, (size_t)3 * (n_lines + 8) + 8, &wk));
    uint32_t *starts = wk, *sizes = wk + n_lines + 8, *offs = sizes + n_lines + 8;
    unsigned long long *err = reinterpret_cast<unsigned long long *>(wk + (((size_t)3 * (n_lines + 8) + 1) & ~(size_t)1));
    uint32_t *max_size = reinterpret_cast<uint32_t *>(err + 1);
    ELP_LAUNCH(c, "stage_sam_starts", k_sam_starts, dim3(tiles), dim3(256), 0, (const uint8_t *)d_text, pb, (const uint32_t *)tile_base, starts);
    const uint32_t virtual_end = pb + 1;  // a last line without a newline: as if the newline stood behind the text
    if (open_end) ELP_HIP(c, hipMemcpyAsync(starts + n_lines, &virtual_end, 4, hipMemcpyHostToDevice, st));
    ELP_HIP(c, hipMemsetAsync(err, 0xFF, 8, st));
    ELP_HIP(c, hipMemsetAsync(max_size, 0, 4, st));
    SamIn in{d_text, starts, 0, n_lines, sizes, err, max_size, nullptr, nullptr, nullptr, 0, c->ref_names.p, c->ref_names_off.p, c->ref_name_slots.p, c->ref_name_mask, c->n_ref};
    const unsigned grid = std::min<unsigned>(n_lines, (unsigned)c->n_cu * 64);
    if (n_lines) ELP_LAUNCH(c, "stage_sam_sizes", k_sam_lines<false>, dim3(grid), dim3(64), 0, in);
    unsigned long long h_err = 0;
    uint32_t h_max = 0;
    ELP_HIP(c, hipMemcpyAsync(&h_err, err, 8, hipMemcpyDeviceToHost, st));
    ELP_HIP(c, hipMemcpyAsync(&h_max, max_size, 4, hipMemcpyDeviceToHost, st));
    ELP_HIP(c, elp::stream_wait(st));
    if (h_err != ~0ull) {
      const uint32_t reason = (uint32_t)(h_err & 0xFF);
      return set_error(c, reason >= R_UNSUPPORTED ? ELP_ERR_UNSUPPORTED : ELP_ERR_DATA, "elp_stage_sam: line %llu: %s", (unsigned long long)(lines_before + (h_err >> 8)),
                       reason_text(reason));
    }
    // write passes: all lines of the piece at once unless the tuning knob caps them
    const uint32_t pass = c->tune.sam_pass > 0 ? (uint32_t)c->tune.sam_pass : std::max(n_lines, 1u);
    for (uint32_t l0 = 0; l0 < n_lines; l0 += pass) {
      const uint32_t cnt = std::min(pass, n_lines - l0);
      uint32_t total = 0;
      ELP_TRY(exclusive_scan_u32(c, sizes + l0, offs, cnt, &total));
      ELP_HIP(c, elp::stream_wait(st));  // (total)
      ELP_TRY(ensure(c, c->raw, c->raw_bytes + total + 64, true, c->raw_bytes));
      ELP_TRY(ensure(c, c->raw_off, c->n + cnt + 2, true, c->n + 1));
      SamIn w = in;
      w.line0 = l0; w.n_lines = cnt; w.offs = offs; w.out = c->raw.p + c->raw_bytes; w.raw_off = c->raw_off.p + c->n; w.raw_base = c->raw_bytes;
      ELP_LAUNCH(c, "stage_sam_write", k_sam_lines<true>, dim3(std::min<unsigned>(cnt, (unsigned)c->n_cu * 64)), dim3(64), 0, w);
      const uint64_t raw_end = c->raw_bytes + total;
      ELP_HIP(c, hipMemcpyAsync(c->raw_off.p + c->n + cnt, &raw_end, 8, hipMemcpyHostToDevice, st));
      ELP_HIP(c, elp::stream_wait(st));  // (raw_end leaves scope; stage_bam_columns waits anyway)
      ELP_TRY(stage_bam_columns(c, cnt, total, raw_end, std::max<uint64_t>(c->max_raw_rec, h_max), split_id));
    }
    lines_before += n_lines;
    at_byte = end;
  }
  ELP_HIP(c, elp::stream_wait(st));
  c->derived.records_changed();
  return 0;
}

}  // extern "C"
