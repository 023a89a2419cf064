// bam_out.hip — BAM records out: formatBamAlignment (sam/bam-files.go:635-737) for the output records of a stream (emit_stream,
// emit.hip: sorted, merged, concat or split, without the sr-tagged / filtered records): fixed fields from the columns with the
// duplicate flags of elp_mark_duplicates, bin() recomputed (:443-468), read name, CIGAR, the ORIGINAL 4-bit bases, the recalibrated
// qualities of elp_bqsr_apply, and the tags re-encoded as formatBamTag does (:481-632: integers in the smallest type that holds them,
// unsigned if >= 0; everything else as it came).  This is the "payload permutation" the reference does on pointers, done as one gather
// in HBM.  A size pass of one thread per record, emit_stream's scan, an emit pass of one wavefront per record; bam_sizes_launch and
// bam_emit_launch queue the two, as sam.hip's pair does for SAM lines.
#include "common.hpp"
#include "bamtag.hpp"
#include "bamout.hpp"

namespace elp {

// (BamOut, tag_dropped, out_source: bamout.hpp - sam.hip writes SAM text from the same columns)
// size of output record k (block_size field included); *tags_at = offset of the tags inside the input record
// OPT: a tag filter or a replacing read group is set.  The walks are bound by their chain of dependent loads and the per-field tests cost
// the emitter 8 % where nothing is set (measured), so a context without either runs the instantiation without them.
// SR: the split emitters (split.hip), an instantiation of its own for the same reason; set_sr = this output record is the tagged copy of a
// spread record and gets aln.TAGS.Set(sr, int64(1)) (sam/split-merge.go:290; SmallMap.Set, utils/small-map.go:59-67): the FIRST field with
// key sr, whatever its type, goes out as s r C 0x01 (formatBamTag, sam/bam-files.go:509-513: 1 is type C), a record without one gets it
// behind its last field.  elp_emit_split_* refuses a tag filter and a replacing read group, so SR never meets OPT.
template <bool OPT, bool SR = false>
__device__ inline uint32_t out_size(const BamOut &m, uint32_t i, uint32_t *err, bool set_sr = false) {
  static_assert(!(OPT && SR), "the split emitters run without a tag filter and a replacing read group");
  const uint8_t *p = m.raw + m.raw_off[i];
  const uint32_t bs = ld_u32(p);
  const uint8_t *rec = p + 4, *end = rec + bs;
  const uint32_t l_name = rec[8], n_cig = ld_u16(rec + 12), l_seq = ld_u32(rec + 16);
  const uint64_t fixed = 32ull + l_name + 4ull * n_cig + ((l_seq + 1) >> 1) + l_seq;
  // (the record goes out with the CIGAR column's operations - elp_clean_sam may have rewritten them -, the tags come from the staged bytes)
  const uint64_t n_cig_out = m.cigar_off[i + 1] - m.cigar_off[i];
  uint32_t size = 4 + (uint32_t)(fixed + 4ull * n_cig_out - 4ull * n_cig);
  const uint8_t *t = rec + fixed;
  bool rg_seen = false, sr_seen = false;
  while (t + 3 <= end) {
    const uint8_t ty = t[2];
    const uint8_t *v = t + 3;
    const uint32_t sz = tag_value_size(ty, v, end);
    if (!sz) { *err |= 2u; break; }
    if (ty == 'H') *err |= 16u;  // parseBamByteArray looks for the character '0' as the terminator (:203): not reproduced
    // (both errors also for a field the filter drops: the reference parses a record before it filters it)
    uint8_t ot;
    if constexpr (OPT) {
      const uint32_t key = tag_key(t);
      if (!tag_dropped(m.drop, key)) {
        if (m.rg_on && key == KEY_RG && !rg_seen) size += 4 + m.rg_len;  // SmallMap.Set (utils/small-map.go:59-67): the FIRST field of the key, whatever its type
        else size += 3 + (tag_is_int(ty) ? int_out(tag_int_value(ty, v), &ot) : sz);
      }
      rg_seen |= key == KEY_RG;
    } else if constexpr (SR) {
      const bool is_sr = tag_key(t) == KEY_SR;
      if (set_sr && is_sr && !sr_seen) size += 4;
      else size += 3 + (tag_is_int(ty) ? int_out(tag_int_value(ty, v), &ot) : sz);
      sr_seen |= is_sr;
    } else {
      size += 3 + (tag_is_int(ty) ? int_out(tag_int_value(ty, v), &ot) : sz);
    }
    t = v + sz;
  }
  if constexpr (OPT)
    if (m.rg_on && !rg_seen && !tag_dropped(m.drop, KEY_RG)) size += 4 + m.rg_len;  // ... else appended behind the last field
  if constexpr (SR)
    if (set_sr && !sr_seen) size += 4;
  return size;
}
template <bool OPT, bool SR = false>
__global__ __launch_bounds__(256) void k_bam_out_sizes(BamOut m, BamOut m2, const uint32_t *__restrict__ src, uint64_t k0, uint32_t cnt, uint32_t *__restrict__ sizes,
                                                       uint32_t *err) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= cnt) return;
  uint32_t e = 0, i;
  bool set_sr;
  const BamOut &mm = out_source<SR>(m, m2, src, k0 + j, &i, &set_sr);
  sizes[j] = out_size<OPT, SR>(mm, i, &e, set_sr);
  if (e) atomicOr(err, e);
}
// (Alignment.bin(): reg2bin / record_bin, bamout.hpp)
// one wavefront per output record; `out` = this chunk's buffer, offs = exclusive scan of the chunk's sizes
template <bool OPT, bool SR = false>
__global__ __launch_bounds__(256) void k_bam_out_emit(BamOut m_first, BamOut m_second, const uint32_t *__restrict__ src, uint64_t k0, uint32_t cnt,
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
    uint8_t *o = out + offs[j];
    const uint32_t l_name = rec[8], l_seq = m.l_seq[i];
    const uint64_t c0 = m.cigar_off[i];
    const uint32_t n_cig = (uint32_t)(m.cigar_off[i + 1] - c0), seqb = (l_seq + 1) >> 1;
    const uint32_t fixed = 32 + l_name + 4 * n_cig + seqb + l_seq;
    if (lane == 0) {
      const uint16_t f = m.flag[i];
      const int32_t beg = m.pos[i] - 1;
      uint32_t ref_span = 0;
      if (!(f & F_UNMAPPED)) {
        for (uint32_t k = 0; k < n_cig; k++) {
          const uint32_t c = m.cigar[c0 + k];
          if (op_consumes_ref(c & 0xF)) ref_span += c >> 4;
        }
      }
      st_u32(o + 4, (uint32_t)m.refid[i]);
      st_u32(o + 8, (uint32_t)beg);
      o[12] = (uint8_t)l_name;
      o[13] = m.mapq[i];
      st_u16(o + 14, record_bin(f, beg, ref_span));
      st_u16(o + 16, n_cig);
      st_u16(o + 18, f);
      st_u32(o + 20, l_seq);
      st_u32(o + 24, (uint32_t)m.next_refid[i]);
      st_u32(o + 28, (uint32_t)(m.pnext[i] - 1));
      st_u32(o + 32, (uint32_t)m.tlen[i]);
    }
    {
      // tags, re-encoded as formatBamTag does.  The WAVE walks them (round 6: lane 0 did, byte by byte - a dependent load per byte of
      // every string while 63 lanes waited): every lane reads the same tag header, a string's end is found by all lanes at once, a value
      // that stays as it is is copied by all lanes; only an integer's new form is written by lane 0.
      uint8_t *w = o + 4 + fixed;
      const uint8_t *t = rec + (32ull + l_name + 4ull * ld_u16(rec + 12) + ((ld_u32(rec + 16) + 1) >> 1) + ld_u32(rec + 16));
      // elp_set_tag_filter / elp_set_replace_read_group: the same walk - a dropped field is skipped by the whole wave together (the key
      // and the table's word are wave-uniform), the first RG field goes out as RG:Z:<id>, a record without one gets it behind its last field
      // elp_emit_split_* (SR): the tagged copy's first sr field goes out as sr:C:1 the same way, a copy without one gets it behind its last field
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
            if (__ballot(!in)) break;  // no NUL in front of the record's end: malformed, as tag_value_size says
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
          if (lane == 0) { w[0] = 'R'; w[1] = 'G'; w[2] = 'Z'; w[3 + m.rg_len] = 0; }
          for (uint32_t b = lane; b < m.rg_len; b += 64) w[3 + b] = m.rg_new[b];
          w += 4 + m.rg_len;
        } else if (SR && is_sr) {
          if (lane == 0) { w[0] = 's'; w[1] = 'r'; w[2] = 'C'; w[3] = 1; }
          w += 4;
        } else if (tag_is_int(ty)) {
          const long long val = tag_int_value(ty, v);
          uint8_t ot;
          const uint32_t os = int_out(val, &ot);
          if (lane == 0) {
            w[0] = t[0]; w[1] = t[1]; w[2] = ot;
            for (uint32_t b = 0; b < os; b++) w[3 + b] = (uint8_t)((unsigned long long)val >> (8 * b));
          }
          w += 3 + os;
        } else {
          for (uint32_t b = lane; b < 3 + sz; b += 64) w[b] = t[b];
          w += 3 + sz;
        }
        t = v + sz;
      }
      if (OPT && m.rg_on && !rg_seen && !tag_dropped(m.drop, KEY_RG)) {
        if (lane == 0) { w[0] = 'R'; w[1] = 'G'; w[2] = 'Z'; w[3 + m.rg_len] = 0; }
        for (uint32_t b = lane; b < m.rg_len; b += 64) w[3 + b] = m.rg_new[b];
        w += 4 + m.rg_len;
      }
      if (SR && set_sr && !sr_seen) {
        if (lane == 0) { w[0] = 's'; w[1] = 'r'; w[2] = 'C'; w[3] = 1; }
        w += 4;
      }
      if (lane == 0) st_u32(o, (uint32_t)(w - o - 4));  // block_size
    }
    // read name (+ NUL), CIGAR, the original bases, the qualities as they are now
    uint8_t *w = o + 36;
    const uint64_t q0 = m.qname_off[i];
    for (uint32_t k = lane; k < l_name; k += 64) w[k] = k + 1 < l_name ? m.qname[q0 + k] : (uint8_t)0;
    w += l_name;
    for (uint32_t k = lane; k < n_cig; k += 64) st_u32(w + 4 * k, m.cigar[c0 + k]);
    w += 4 * n_cig;
    const uint8_t *seq_in = rec + 32 + l_name + 4 * ld_u16(rec + 12);
    for (uint32_t k = lane; k < seqb; k += 64) w[k] = seq_in[k];
    w += seqb;
    const uint64_t l0 = m.qual_off[i];
    for (uint32_t k = lane; k < l_seq; k += 64) w[k] = m.qual[l0 + k];
  }
}

// the two passes of a BAM chunk (declared in bamout.hpp, beside sam.hip's): the instantiation by the stream's settings, the emit grid
int bam_sizes_launch(elp_ctx *c, const BamOut &m, const BamOut &m2, const uint32_t *src, uint64_t k0, uint32_t cnt, uint32_t *sizes, uint32_t *err) {
  const bool opt = m.drop != nullptr || m.rg_on;  // (m2 shares m's settings: two_context_checks, emit.hip)
  // (m.sr_on: the split emitters: never with `opt`, elp_emit_split_* refuses)
  if (m.sr_on) ELP_LAUNCH(c, "emit_split_bam_sizes", (k_bam_out_sizes<false, true>), dim3(blocks_for(cnt, 256)), dim3(256), 0, m, m2, src, k0, cnt, sizes, err);
  else if (opt) ELP_LAUNCH(c, "emit_bam_sizes", k_bam_out_sizes<true>, dim3(blocks_for(cnt, 256)), dim3(256), 0, m, m2, src, k0, cnt, sizes, err);
  else ELP_LAUNCH(c, "emit_bam_sizes", k_bam_out_sizes<false>, dim3(blocks_for(cnt, 256)), dim3(256), 0, m, m2, src, k0, cnt, sizes, err);
  return 0;
}
int bam_emit_launch(elp_ctx *c, const BamOut &m, const BamOut &m2, const uint32_t *src, uint64_t k0, uint32_t cnt, const uint32_t *offs, uint8_t *out) {
  const bool opt = m.drop != nullptr || m.rg_on;
  const unsigned grid = std::min<unsigned>(blocks_for((uint64_t)cnt * 64, 256), (unsigned)c->n_cu * 32);
  if (m.sr_on) ELP_LAUNCH(c, "emit_split_bam", (k_bam_out_emit<false, true>), dim3(grid), dim3(256), 0, m, m2, src, k0, cnt, offs, out);
  else if (opt) ELP_LAUNCH(c, "emit_bam", k_bam_out_emit<true>, dim3(grid), dim3(256), 0, m, m2, src, k0, cnt, offs, out);
  else ELP_LAUNCH(c, "emit_bam", k_bam_out_emit<false>, dim3(grid), dim3(256), 0, m, m2, src, k0, cnt, offs, out);
  return 0;
}

}  // namespace elp
