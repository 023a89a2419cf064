// sam.hip — SAM text out, on the device: FormatAlignment(parseBamAlignment(record)) (sam/sam-files.go:563-598, sam/bam-files.go:317-400)
// of the records the BAM emitters write, from the same columns and staged bytes (bamout.hpp), in the same chunked loop (emit_stream,
// emit.hip): a size pass of one thread per record, a scan, an emit pass of one wavefront per record.  The scalar pieces - decimal digits,
// the base table, the float form, a field's text - are samtext.hpp's, which the CPU tests run on the host.
//
// The line: QNAME FLAG RNAME POS MAPQ CIGAR RNEXT PNEXT TLEN SEQ QUAL separated by tabs, every optional field behind a tab, '\n'.
//   RNAME / RNEXT  the name of the refid, "*" below 0; RNEXT "=" where next_refid == refid (the reference compares the strings,
//                  bam-files.go:344-346: elp_set_reference_names_flat takes distinct names only, so the ids decide)
//   CIGAR          from the CIGAR column (so behind elp_clean_sam), "*" for none
//   SEQ            the staged 4-bit bases, one character each; none for l_seq 0 (the loop at :584-587 writes nothing, not "*")
//   QUAL           the QUAL column as it is now + 33, modulo 256 (BAM's 0xFF "missing" bytes leave as spaces, as the reference writes them)
//   fields         behind the tag filter and the read-group replacement, as the BAM emitter keeps them; every integer type as :i:
// No header lines: the host writes @HD, @SQ, @RG, @PG and then these bytes.
#include <algorithm>
#include <string>
#include <vector>

#include "common.hpp"
#include "bamtag.hpp"
#include "bamout.hpp"
#include "samtext.hpp"

namespace elp {

namespace st = samtext;

constexpr uint32_t SR_TEXT_LEN = 7;  // "\tsr:i:1"
// text size of output record k; the error bits of the BAM size pass (2 malformed fields, 16 an H field) and 32: a refid outside the names
// SR (the split emitters, split.hip), set_sr: as out_size's (bam_out.hip) - the tagged copy's first sr field goes out as "\tsr:i:1", a copy
// without one gets it behind its last field
template <bool OPT, bool SR = false>
__device__ inline uint32_t sam_out_size(const BamOut &m, const SamNames &nm, uint32_t i, uint32_t *err, bool set_sr = false) {
  static_assert(!(OPT && SR), "the split emitters run without a tag filter and a replacing read group");
  const uint8_t *p = m.raw + m.raw_off[i];
  const uint32_t bs = ld_u32(p);
  const uint8_t *rec = p + 4, *end = rec + bs;
  const uint32_t l_name = rec[8], n_cig = ld_u16(rec + 12), l_seq = ld_u32(rec + 16);
  const uint64_t fixed = 32ull + l_name + 4ull * n_cig + ((l_seq + 1) >> 1) + l_seq;
  const int32_t refid = m.refid[i], nref = m.next_refid[i];
  if (refid >= nm.n_ref || nref >= nm.n_ref) { *err |= 32u; return 0; }  // (staging checks refid alone)
  uint32_t size = 11;  // ten tabs and the newline
  size += (uint32_t)(m.qname_off[i + 1] - m.qname_off[i]);
  size += st::u32_width(m.flag[i]) + st::u32_width(m.mapq[i]);
  size += st::i64_width(m.pos[i]) + st::i64_width(m.pnext[i]) + st::i64_width(m.tlen[i]);
  size += refid < 0 ? 1u : nm.name_off[refid + 1] - nm.name_off[refid];
  size += (nref < 0 || nref == refid) ? 1u : nm.name_off[nref + 1] - nm.name_off[nref];
  const uint64_t c0 = m.cigar_off[i], c1 = m.cigar_off[i + 1];
  if (c0 == c1) size += 1;
  for (uint64_t k = c0; k < c1; k++) size += st::u32_width(m.cigar[k] >> 4) + 1u;
  size += 2u * m.l_seq[i];  // (the column, as the emit pass reads it; equal to the staged field)
  // the optional fields: out_size's walk (bam_out.hip), counting text
  const uint8_t *t = rec + fixed;
  bool rg_seen = false, sr_seen = false;
  while (t + 3 <= end) {
    const uint8_t ty = t[2];
    const uint8_t *v = t + 3;
    const uint32_t sz = tag_value_size(ty, v, end);
    if (!sz) { *err |= 2u; break; }
    if (ty == 'H') { *err |= 16u; break; }  // (refused, as by the BAM emitters)
    if constexpr (OPT) {
      const uint32_t key = tag_key(t);
      if (!tag_dropped(m.drop, key)) {
        if (m.rg_on && key == KEY_RG && !rg_seen) size += 6 + m.rg_len;  // "\tRG:Z:<id>" in place of the FIRST field of the key
        else size += st::put_field(nullptr, t, ty, v, sz);
      }
      rg_seen |= key == KEY_RG;
    } else if constexpr (SR) {
      const bool is_sr = tag_key(t) == KEY_SR;
      if (set_sr && is_sr && !sr_seen) size += SR_TEXT_LEN;
      else size += st::put_field(nullptr, t, ty, v, sz);
      sr_seen |= is_sr;
    } else {
      size += st::put_field(nullptr, t, ty, v, sz);
    }
    t = v + sz;
  }
  if constexpr (OPT)
    if (m.rg_on && !rg_seen && !tag_dropped(m.drop, KEY_RG)) size += 6 + m.rg_len;
  if constexpr (SR)
    if (set_sr && !sr_seen) size += SR_TEXT_LEN;
  return size;
}
template <bool OPT, bool SR = false>
__global__ __launch_bounds__(256) void k_sam_out_sizes(BamOut m, BamOut m2, SamNames nm, const uint32_t *__restrict__ src, uint64_t k0, uint32_t cnt,
                                                       uint32_t *__restrict__ sizes, uint32_t *err) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= cnt) return;
  uint32_t e = 0, i;
  bool set_sr;
  const BamOut &mm = out_source<SR>(m, m2, src, k0 + j, &i, &set_sr);
  sizes[j] = sam_out_size<OPT, SR>(mm, nm, i, &e, set_sr);
  if (e) atomicOr(err, e);
}

// inclusive prefix sum over the wavefront (all 64 lanes active)
__device__ __forceinline__ uint32_t wave_scan(uint32_t v, uint32_t lane) {
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint32_t up = __shfl_up(v, d);
    if (lane >= d) v += up;
  }
  return v;
}
// lane 0's count for the whole wave
__device__ __forceinline__ uint32_t from_lane0(uint32_t v) { return __shfl(v, 0); }
__device__ __forceinline__ uint32_t put_ref_name(uint8_t *w, const SamNames &nm, int32_t r, bool same, uint32_t lane) {
  if (r < 0 || same) {
    if (lane == 0) w[0] = same && r >= 0 ? '=' : '*';
    return 1;
  }
  const uint32_t o = nm.name_off[r], l = nm.name_off[r + 1] - o;
  for (uint32_t k = lane; k < l; k += 64) w[k] = nm.names[o + k];
  return l;
}
__device__ __forceinline__ uint32_t put_rg(uint8_t *w, const BamOut &m, uint32_t lane) {
  if (lane == 0) { w[0] = '\t'; w[1] = 'R'; w[2] = 'G'; w[3] = ':'; w[4] = 'Z'; w[5] = ':'; }
  for (uint32_t b = lane; b < m.rg_len; b += 64) w[6 + b] = m.rg_new[b];
  return 6 + m.rg_len;
}
__device__ __forceinline__ uint32_t put_sr(uint8_t *w, uint32_t lane) {
  if (lane == 0) { w[0] = '\t'; w[1] = 's'; w[2] = 'r'; w[3] = ':'; w[4] = 'i'; w[5] = ':'; w[6] = '1'; }
  return SR_TEXT_LEN;
}

// one wavefront per output line; `out` = this chunk's buffer, offs = exclusive scan of the chunk's sizes.  The lanes copy QNAME, the names,
// SEQ (a lane takes one staged byte: two bases), QUAL and Z values in strides of 64; the few numbers of the fixed columns and of scalar
// fields are lane 0's, which tells the wave how far it wrote.  CIGAR operations and B elements have texts of different widths: every
// lane formats one, a prefix sum over the wave places them, the running offset carries over the steps of 64.
template <bool OPT, bool SR = false>
__global__ __launch_bounds__(256) void k_sam_out_emit(BamOut m_first, BamOut m_second, SamNames nm, const uint32_t *__restrict__ src, uint64_t k0, uint32_t cnt,
                                                      const uint32_t *__restrict__ offs, uint8_t *__restrict__ out) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
  for (uint32_t j = wave; j < cnt; j += nwaves) {
    uint32_t i;
    bool set_sr;  // (wave-uniform, as i)
    const BamOut &m = out_source<SR>(m_first, m_second, src, k0 + j, &i, &set_sr);
    const uint8_t *p = m.raw + m.raw_off[i];
    const uint32_t bs = ld_u32(p);
    const uint8_t *rec = p + 4, *end = rec + bs;
    uint8_t *w = out + offs[j];
    const uint32_t l_name = rec[8], l_seq = m.l_seq[i];
    const int32_t refid = m.refid[i], nref = m.next_refid[i];
    // QNAME
    const uint64_t q0 = m.qname_off[i];
    const uint32_t lq = (uint32_t)(m.qname_off[i + 1] - q0);
    for (uint32_t k = lane; k < lq; k += 64) w[k] = m.qname[q0 + k];
    w += lq;
    // FLAG RNAME POS MAPQ
    uint32_t n = 0;
    if (lane == 0) { w[0] = '\t'; n = 1 + st::put_u32(w + 1, m.flag[i]); w[n++] = '\t'; }
    w += from_lane0(n);
    w += put_ref_name(w, nm, refid, false, lane);
    if (lane == 0) {
      w[0] = '\t'; n = 1 + st::put_i64(w + 1, m.pos[i]);
      w[n++] = '\t'; n += st::put_u32(w + n, m.mapq[i]);
      w[n++] = '\t';
    }
    w += from_lane0(n);
    // CIGAR
    const uint64_t c0 = m.cigar_off[i];
    const uint32_t n_cig = (uint32_t)(m.cigar_off[i + 1] - c0);
    if (n_cig == 0) {
      if (lane == 0) w[0] = '*';
      w += 1;
    }
    for (uint32_t base = 0; base < n_cig; base += 64) {
      const uint32_t k = base + lane;
      const bool in = k < n_cig;
      const uint32_t c = in ? m.cigar[c0 + k] : 0u;
      const uint32_t wd = in ? st::u32_width(c >> 4) + 1u : 0u;
      const uint32_t incl = wave_scan(wd, lane);
      if (in) {
        uint8_t *d = w + (incl - wd);
        st::put_u32(d, c >> 4);
        d[wd - 1] = st::cigar_op_char(c & 0xF);
      }
      w += __shfl(incl, 63);
    }
    // RNEXT PNEXT TLEN
    if (lane == 0) w[0] = '\t';
    w += 1;
    w += put_ref_name(w, nm, nref, nref == refid, lane);
    if (lane == 0) {
      w[0] = '\t'; n = 1 + st::put_i64(w + 1, m.pnext[i]);
      w[n++] = '\t'; n += st::put_i64(w + n, m.tlen[i]);
      w[n++] = '\t';
    }
    w += from_lane0(n);
    // SEQ: the original bases, QUAL: the qualities as they are now
    const uint32_t seqb = (l_seq + 1) >> 1;
    const uint8_t *seq_in = rec + 32 + l_name + 4 * ld_u16(rec + 12);
    for (uint32_t k = lane; k < seqb; k += 64) {
      const uint32_t b = seq_in[k];
      w[2 * k] = st::base_of(b >> 4);
      if (2 * k + 1 < l_seq) w[2 * k + 1] = st::base_of(b & 15u);
    }
    w += l_seq;
    if (lane == 0) w[0] = '\t';
    w += 1;
    const uint64_t l0 = m.qual_off[i];
    for (uint32_t k = lane; k < l_seq; k += 64) w[k] = (uint8_t)(m.qual[l0 + k] + 33u);
    w += l_seq;
    // the optional fields: the BAM emitter's wave-uniform walk (k_bam_out_emit), writing text
    const uint8_t *t = rec + (32ull + l_name + 4ull * ld_u16(rec + 12) + ((ld_u32(rec + 16) + 1) >> 1) + ld_u32(rec + 16));
    bool rg_seen = false, sr_seen = false;
    while (t + 3 <= end) {
      const uint8_t ty = t[2];
      const uint8_t *v = t + 3;
      uint32_t sz;
      if (ty == 'Z' || ty == 'H') {  // (tag_value_size's loop, 64 bytes a step)
        sz = 0;
        for (uint32_t at = 0;; at += 64) {
          const uint8_t *q = v + at + lane;
          const bool in = q < end;
          const unsigned long long zero = __ballot(in && *q == 0);
          if (zero) { sz = at + (uint32_t)__builtin_ctzll(zero) + 1u; break; }
          if (__ballot(!in)) break;
        }
      } else {
        sz = tag_value_size(ty, v, end);
      }
      if (!sz) break;
      bool dropped = false, is_rg = false, is_sr = false;
      if constexpr (OPT) {
        const uint32_t key = tag_key(t);
        dropped = tag_dropped(m.drop, key);
        is_rg = m.rg_on && key == KEY_RG && !rg_seen;
        rg_seen |= key == KEY_RG;
      }
      if constexpr (SR) {
        const bool key_sr = tag_key(t) == KEY_SR;
        is_sr = set_sr && key_sr && !sr_seen;
        sr_seen |= key_sr;
      }
      if (dropped) {
      } else if (is_rg) {
        w += put_rg(w, m, lane);
      } else if (SR && is_sr) {
        w += put_sr(w, lane);
      } else if (ty == 'Z' || ty == 'H') {
        if (lane == 0) { w[0] = '\t'; w[1] = t[0]; w[2] = t[1]; w[3] = ':'; w[4] = ty; w[5] = ':'; }
        for (uint32_t b = lane; b + 1 < sz; b += 64) w[6 + b] = v[b];
        w += 6 + sz - 1;
      } else if (ty == 'B') {
        const uint8_t sub = v[0];
        const uint32_t count = ld_u32(v + 1), es = st::elem_size(sub);
        if (lane == 0) { w[0] = '\t'; w[1] = t[0]; w[2] = t[1]; w[3] = ':'; w[4] = 'B'; w[5] = ':'; w[6] = sub; }
        w += 7;
        for (uint32_t base = 0; base < count; base += 64) {
          const uint32_t k = base + lane;
          const bool in = k < count;
          const uint8_t *e = v + 5 + (uint64_t)k * es;
          const uint32_t wd = in ? 1u + st::put_number(nullptr, sub, e) : 0u;
          const uint32_t incl = wave_scan(wd, lane);
          if (in) {
            uint8_t *d = w + (incl - wd);
            d[0] = ',';
            st::put_number(d + 1, sub, e);
          }
          w += __shfl(incl, 63);
        }
      } else {  // A, the six integer types, f
        n = 0;
        if (lane == 0) n = st::put_field(w, t, ty, v, sz);
        w += from_lane0(n);
      }
      t = v + sz;
    }
    if (OPT && m.rg_on && !rg_seen && !tag_dropped(m.drop, KEY_RG)) w += put_rg(w, m, lane);
    if (SR && set_sr && !sr_seen) w += put_sr(w, lane);
    if (lane == 0) w[0] = '\n';
  }
}

int sam_sizes_launch(elp_ctx *c, const BamOut &m, const BamOut &m2, const SamNames &nm, const uint32_t *src, uint64_t k0, uint32_t cnt, uint32_t *sizes, uint32_t *err) {
  const bool opt = m.drop != nullptr || m.rg_on;  // (m2 shares m's settings, as in the BAM emitters)
  if (m.sr_on) ELP_LAUNCH(c, "emit_split_sam_sizes", (k_sam_out_sizes<false, true>), dim3(blocks_for(cnt, 256)), dim3(256), 0, m, m2, nm, src, k0, cnt, sizes, err);
  else if (opt) ELP_LAUNCH(c, "emit_sam_sizes", k_sam_out_sizes<true>, dim3(blocks_for(cnt, 256)), dim3(256), 0, m, m2, nm, src, k0, cnt, sizes, err);
  else ELP_LAUNCH(c, "emit_sam_sizes", k_sam_out_sizes<false>, dim3(blocks_for(cnt, 256)), dim3(256), 0, m, m2, nm, src, k0, cnt, sizes, err);
  return 0;
}
int sam_emit_launch(elp_ctx *c, const BamOut &m, const BamOut &m2, const SamNames &nm, const uint32_t *src, uint64_t k0, uint32_t cnt, const uint32_t *offs, uint8_t *out) {
  const bool opt = m.drop != nullptr || m.rg_on;
  const unsigned grid = std::min<unsigned>(blocks_for((uint64_t)cnt * 64, 256), (unsigned)c->n_cu * 32);
  if (m.sr_on) ELP_LAUNCH(c, "emit_split_sam", (k_sam_out_emit<false, true>), dim3(grid), dim3(256), 0, m, m2, nm, src, k0, cnt, offs, out);
  else if (opt) ELP_LAUNCH(c, "emit_sam", k_sam_out_emit<true>, dim3(grid), dim3(256), 0, m, m2, nm, src, k0, cnt, offs, out);
  else ELP_LAUNCH(c, "emit_sam", k_sam_out_emit<false>, dim3(grid), dim3(256), 0, m, m2, nm, src, k0, cnt, offs, out);
  return 0;
}

}  // namespace elp

using namespace elp;

extern "C" {

int elp_set_reference_names_flat(elp_ctx *c, const uint8_t *names, const uint32_t *name_off) {
  if (!c) return ELP_ERR_ARG;
  if (!c->have_header) return set_error(c, ELP_ERR_ARG, "elp_set_reference_names_flat: call elp_set_header first");
  if (c->n_ref && (!names || !name_off)) return set_error(c, ELP_ERR_ARG, "elp_set_reference_names_flat: names and name_off must be given (%d references)", c->n_ref);
  const size_t n = (size_t)c->n_ref;
  std::vector<uint32_t> off(n + 1, 0u);
  std::vector<std::string> sorted(n);
  uint32_t longest = 0;
  for (size_t r = 0; r < n; r++) {
    if (name_off[r + 1] < name_off[r]) return set_error(c, ELP_ERR_ARG, "elp_set_reference_names_flat: name_off must not decrease");
    const uint32_t l = name_off[r + 1] - name_off[r];
    const char *s = reinterpret_cast<const char *>(names) + name_off[r];
    // "*" and "=" are what RNAME / RNEXT say without a name; the reference would read them back as such
    if (l == 0 || (l == 1 && (s[0] == '*' || s[0] == '='))) return set_error(c, ELP_ERR_ARG, "elp_set_reference_names_flat: name %zu is empty, \"*\" or \"=\"", r);
    sorted[r].assign(s, l);
    off[r + 1] = off[r] + l;
    longest = std::max(longest, l);
  }
  std::string cat;
  for (size_t r = 0; r < n; r++) cat += sorted[r];
  std::sort(sorted.begin(), sorted.end());
  // (distinct names: the emitters write RNEXT "=" where the refids are equal, the reference where the strings are)
  if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return set_error(c, ELP_ERR_ARG, "elp_set_reference_names_flat: two references have the same name");
  ELP_HIP(c, hipSetDevice(c->device));
  ELP_TRY(ensure(c, c->ref_names, cat.size() + 16));
  ELP_TRY(ensure(c, c->ref_names_off, off.size() + 4));
  if (!cat.empty()) ELP_HIP(c, hipMemcpyAsync(c->ref_names.p, cat.data(), cat.size(), hipMemcpyHostToDevice, c->stream));
  ELP_HIP(c, hipMemcpyAsync(c->ref_names_off.p, off.data(), off.size() * 4, hipMemcpyHostToDevice, c->stream));
  ELP_HIP(c, elp::stream_wait(c->stream));
  c->h_ref_names.swap(cat);
  c->h_ref_names_off.swap(off);
  c->max_ref_name = longest;
  c->have_ref_names = true;
  c->have_ref_name_table = false;  // (elp_stage_sam's look-up is made from the names the first time it is asked for)
  return 0;
}

}  // extern "C"
