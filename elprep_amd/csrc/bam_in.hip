// bam_in.hip — inflated BAM records in (elp_stage_bam): parseBamAlignment (sam/bam-files.go:299-400) for the fields the path reads.
// The host hands over the bytes of inflated BGZF blocks (a run of whole alignment records: block_size, 32 fixed bytes, read_name,
// cigar, seq, qual, tags - SAMv1 4.2); they cross PCIe once, as they are (pinned double buffer, copy overlapped with the host's memcpy
// into it), and kernels cut them into the SoA columns: fixed fields by one thread per record (POS/PNEXT + 1, QNAME without its NUL,
// RG:Z looked up in the header's read-group ids, sr tag -> record state), variable-length parts by one wavefront per record.
// Only the walk along the block_size chain stays on the host (a pointer chase: 4 bytes read per record): bam_cut_piece, emit_plan.hpp.
// stage_bam_columns is shared with elp_stage_bgzf (bgzf.hip) and elp_stage_sam (samin.hip); the read-group ids are set here because
// k_bam_fixed is their only reader.  The way out: bam_out.hip, sam.hip and emit.hip.
#include <thread>

#include "common.hpp"
#include "bamtag.hpp"
#include "emit_plan.hpp"

namespace elp {

struct BamIn {
  const uint8_t *raw;        // records of this piece (device copy); rec_off are offsets from raw
  const uint64_t *rec_off;   // n + 1
  uint32_t n;
  uint64_t at;               // first staging index of the piece
  int32_t *refid, *pos, *next_refid, *pnext, *tlen;
  uint16_t *flag, *rgid, *split;
  uint8_t *mapq, *state;
  uint32_t *l_seq;
  uint32_t *len_q, *len_c, *len_s, *len_l;  // per record: QNAME bytes, CIGAR ops, SEQ bytes, QUAL bytes
  const uint8_t *rg_ids;     // header read-group ids, concatenated
  const uint32_t *rg_off;    // n_rg + 1
  int32_t n_rg, n_ref;
  int32_t replace_rg;        // elp_set_replace_read_group: every record is of read group 0, RG fields are not looked up
  uint16_t split_id;
  uint32_t *stats;           // [0] max QNAME length, [1] max l_seq, [2] max POS, [3] sr-tagged records, [4] error bits
};

__global__ __launch_bounds__(256) void k_bam_fixed(BamIn m) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  bool sr = false;
  if (r < m.n) {
    const uint8_t *p = m.raw + m.rec_off[r];
    const uint32_t bs = ld_u32(p);
    const uint8_t *rec = p + 4, *end = rec + bs;
    const uint64_t i = m.at + r;
    const int32_t refid = (int32_t)ld_u32(rec), pos0 = (int32_t)ld_u32(rec + 4);
    const uint32_t l_name = rec[8], n_cig = ld_u16(rec + 12), l_seq = ld_u32(rec + 16);
    const uint32_t seqb = (l_seq + 1) >> 1;
    const uint64_t fixed = 32ull + l_name + 4ull * n_cig + seqb + l_seq;
    uint32_t err = 0;
    if (bs < 32 || l_name == 0 || fixed > bs || refid >= m.n_ref || (uint64_t)bs + 4 != m.rec_off[r + 1] - m.rec_off[r]) err |= 1u;
    m.refid[i] = refid < 0 ? -1 : refid;                 // RNAME "*" (:322-326)
    m.pos[i] = pos0 + 1;                                 // :328
    m.mapq[i] = rec[9];
    m.flag[i] = (uint16_t)ld_u16(rec + 14);
    m.l_seq[i] = l_seq;
    const int32_t nref = (int32_t)ld_u32(rec + 20);
    m.next_refid[i] = nref < 0 ? -1 : nref;
    m.pnext[i] = (int32_t)ld_u32(rec + 24) + 1;
    m.tlen[i] = (int32_t)ld_u32(rec + 28);
    m.split[i] = m.split_id;
    m.len_q[r] = err ? 0 : l_name - 1;                   // QNAME without the NUL (:352)
    m.len_c[r] = err ? 0 : n_cig;
    m.len_s[r] = err ? 0 : seqb;
    m.len_l[r] = err ? 0 : l_seq;
    // optional fields: RG:Z -> dense id of the header's read groups, sr -> record state (:373-396)
    uint32_t rg = m.replace_rg ? 0u : ELP_NIL16;  // (aln.SetRG(id) runs on every alignment, with or without an RG field)
    if (!err) {
      const uint8_t *t = rec + fixed;
      while (t + 3 <= end) {
        const uint8_t k0 = t[0], k1 = t[1], ty = t[2];
        const uint8_t *v = t + 3;
        const uint32_t sz = tag_value_size(ty, v, end);
        if (!sz || v + sz > end) { err |= 2u; break; }
        if (k0 == 's' && k1 == 'r') sr = true;
        if (k0 == 'C' && k1 == 'G' && ty == 'B') err |= 4u;  // CIGAR in a tag (> 65535 operations): not supported
        if (k0 == 'R' && k1 == 'G' && ty == 'Z' && !m.replace_rg) {
          const uint32_t l = sz - 1;
          rg = 0xFFFEu;  // a read group the header does not know
          for (int g = 0; g < m.n_rg; g++) {
            const uint32_t o = m.rg_off[g], gl = m.rg_off[g + 1] - o;
            if (gl != l) continue;
            bool eq = true;
            for (uint32_t b = 0; b < l; b++) eq &= m.rg_ids[o + b] == v[b];
            if (eq) { rg = (uint32_t)g; break; }
          }
        }
        t = v + sz;
      }
      if (t != end && !(err & 2u)) err |= 2u;
    }
    if (rg == 0xFFFEu) { err |= 8u; rg = ELP_NIL16; }
    m.rgid[i] = (uint16_t)rg;
    m.state[i] = sr ? 1 : 0;
    atomicMax(&m.stats[0], err ? 0u : l_name - 1);
    atomicMax(&m.stats[1], l_seq);
    atomicMax(&m.stats[2], (uint32_t)(pos0 + 1));
    if (err) atomicOr(&m.stats[4], err);
  }
  const unsigned long long b = __ballot(sr);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(&m.stats[3], (uint32_t)__popcll(b));
}

struct BamPay {
  const uint8_t *raw;
  const uint64_t *rec_off;
  uint32_t n;
  uint64_t at;
  const uint32_t *sc_q, *sc_c, *sc_s, *sc_l;  // exclusive scans of the lengths
  const uint32_t *len_q, *len_c, *len_s, *len_l;
  uint64_t base_q, base_c, base_s, base_l;     // column fill levels in front of the piece
  uint64_t *qname_off, *cigar_off, *seq_off, *qual_off;
  uint8_t *qname, *seq4, *qual;
  uint32_t *cigar;
};
// one wavefront per record: lanes copy the variable-length parts byte by byte (coalesced)
__global__ __launch_bounds__(256) void k_bam_payload(BamPay m) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
  for (uint32_t r = wave; r < m.n; r += nwaves) {
    const uint8_t *rec = m.raw + m.rec_off[r] + 4;
    const uint32_t lq = m.len_q[r], lc = m.len_c[r], ls = m.len_s[r], ll = m.len_l[r];
    const uint64_t oq = m.base_q + m.sc_q[r], oc = m.base_c + m.sc_c[r], os = m.base_s + m.sc_s[r], ol = m.base_l + m.sc_l[r];
    if (lane == 0) {
      const uint64_t i = m.at + r;
      m.qname_off[i] = oq; m.cigar_off[i] = oc; m.seq_off[i] = os; m.qual_off[i] = ol;
      if (r + 1 == m.n) { m.qname_off[i + 1] = oq + lq; m.cigar_off[i + 1] = oc + lc; m.seq_off[i + 1] = os + ls; m.qual_off[i + 1] = ol + ll; }
    }
    const uint8_t *src = rec + 32;
    for (uint32_t k = lane; k < lq; k += 64) m.qname[oq + k] = src[k];
    src += lq + 1;
    for (uint32_t k = lane; k < lc; k += 64) m.cigar[oc + k] = ld_u32(src + 4 * k);
    src += 4 * lc;
    for (uint32_t k = lane; k < ls; k += 64) m.seq4[os + k] = src[k];
    src += ls;
    for (uint32_t k = lane; k < ll; k += 64) m.qual[ol + k] = src[k];
  }
}

int stage_reserve(elp_ctx *c, uint64_t n, uint64_t qb, uint64_t co, uint64_t sb, uint64_t lb);  // ctx.hip

// the columns of n_rec records whose inflated bytes lie in c->raw and whose offsets (n_rec + 1, into c->raw) lie at c->raw_off[c->n ..]:
// fixed fields, the four scans, payload copies, SEQ recoding, the commit.  piece_bytes bounds the variable-length columns of the piece;
// raw_end = the first byte of c->raw behind the last record.  Shared by elp_stage_bam and elp_stage_bgzf (bgzf.hip).
int stage_bam_columns(elp_ctx *c, uint32_t n_rec, uint64_t piece_bytes, uint64_t raw_end, uint64_t max_raw_rec, uint16_t split_id) {
  hipStream_t st = c->stream;
  // columns
  ELP_TRY(stage_reserve(c, c->n + n_rec, c->qname_bytes + piece_bytes, c->cigar_ops + piece_bytes / 4, c->seq_bytes + piece_bytes, c->qual_bytes + piece_bytes));
  uint32_t *wk;
  ELP_TRY(scratch(c, 4, (size_t)8 * (n_rec + 8) + 16, &wk));
  const size_t np = (size_t)n_rec + 8;
  uint32_t *len_q = wk, *len_c = wk + np, *len_s = wk + 2 * np, *len_l = wk + 3 * np, *sc_q = wk + 4 * np, *sc_c = wk + 5 * np, *sc_s = wk + 6 * np,
           *sc_l = wk + 7 * np, *stats = wk + 8 * np;
  ELP_HIP(c, hipMemsetAsync(stats, 0, 32, st));
  BamIn in{c->raw.p, c->raw_off.p + c->n, n_rec, c->n, c->refid.p, c->pos.p, c->next_refid.p, c->pnext.p, c->tlen.p, c->flag.p, c->rgid.p, c->split.p,
           c->mapq.p, c->has_sr.p, c->l_seq.p, len_q, len_c, len_s, len_l, c->rg_ids.p, c->rg_ids_off.p, c->n_rg, c->n_ref, c->replace_rg ? 1 : 0, split_id, stats};
  ELP_LAUNCH(c, "stage_bam_fixed", k_bam_fixed, dim3(blocks_for(n_rec, 256)), dim3(256), 0, in);
  uint32_t tq = 0, tc = 0, ts = 0, tl = 0;
  ELP_TRY(exclusive_scan_u32(c, len_q, sc_q, n_rec, &tq));
  ELP_TRY(exclusive_scan_u32(c, len_c, sc_c, n_rec, &tc));
  ELP_TRY(exclusive_scan_u32(c, len_s, sc_s, n_rec, &ts));
  ELP_TRY(exclusive_scan_u32(c, len_l, sc_l, n_rec, &tl));
  uint32_t hs[8];
  ELP_HIP(c, hipMemcpyAsync(hs, stats, 32, hipMemcpyDeviceToHost, st));
  ELP_HIP(c, elp::stream_wait(st));
  if (hs[4]) {
    if (hs[4] & 8u) return set_error(c, ELP_ERR_ARG, "elp_stage_bam: an RG:Z tag names a read group that is not in the header");
    if (hs[4] & 4u) return set_error(c, ELP_ERR_UNSUPPORTED, "elp_stage_bam: CIGAR in a CG:B tag (more than 65535 operations)");
    return set_error(c, ELP_ERR_DATA, "elp_stage_bam: malformed alignment record (bits %u)", hs[4]);
  }
  if (hs[0] > elp_ctx::MAX_QNAME) return set_error(c, ELP_ERR_UNSUPPORTED, "QNAME of %u bytes (limit %u)", hs[0], elp_ctx::MAX_QNAME);
  if (hs[1] > 0x3FFFFFu) return set_error(c, ELP_ERR_UNSUPPORTED, "record with more than 4194303 bases");
  BamPay pay{c->raw.p, c->raw_off.p + c->n, n_rec, c->n, sc_q, sc_c, sc_s, sc_l, len_q, len_c, len_s, len_l, c->qname_bytes, c->cigar_ops, c->seq_bytes,
             c->qual_bytes, c->qname_off.p, c->cigar_off.p, c->seq_off.p, c->qual_off.p, c->qname.p, c->seq4.p, c->qual.p, c->cigar.p};
  if (n_rec) {
    const unsigned grid = std::min<unsigned>(blocks_for((uint64_t)n_rec * 64, 256), (unsigned)c->n_cu * 32);
    ELP_LAUNCH(c, "stage_bam_payload", k_bam_payload, dim3(grid), dim3(256), 0, pay);
    if (ts) ELP_TRY(stage_recode_seq(c, c->seq_bytes, ts));
  }
  c->n += n_rec; c->raw_n += n_rec; c->raw_bytes = raw_end;
  c->qname_bytes += tq; c->cigar_ops += tc; c->seq_bytes += ts; c->qual_bytes += tl;
  c->n_sr += hs[3];
  c->max_qname_len = std::max(c->max_qname_len, hs[0]);
  c->max_l_seq = std::max(c->max_l_seq, hs[1]);
  c->max_pos = std::max(c->max_pos, hs[2]);
  c->max_split = std::max<uint32_t>(c->max_split, split_id);
  c->max_raw_rec = std::max(c->max_raw_rec, max_raw_rec);
  return 0;
}

}  // namespace elp

using namespace elp;

extern "C" {

int elp_set_read_group_ids(elp_ctx *c, const char *const *ids) {
  if (!c || !c->have_header || (c->n_rg && !ids)) return set_error(c, ELP_ERR_ARG, "elp_set_read_group_ids: call elp_set_header first");
  ELP_HIP(c, hipSetDevice(c->device));
  std::vector<uint8_t> cat;
  std::vector<uint32_t> off(1, 0);
  for (int g = 0; g < c->n_rg; g++) {
    const size_t l = strlen(ids[g]);
    cat.insert(cat.end(), ids[g], ids[g] + l);
    off.push_back((uint32_t)cat.size());
  }
  ELP_TRY(ensure(c, c->rg_ids, cat.size() + 16));
  ELP_TRY(ensure(c, c->rg_ids_off, off.size() + 4));
  if (!cat.empty()) ELP_HIP(c, hipMemcpyAsync(c->rg_ids.p, cat.data(), cat.size(), hipMemcpyHostToDevice, c->stream));
  ELP_HIP(c, hipMemcpyAsync(c->rg_ids_off.p, off.data(), off.size() * 4, hipMemcpyHostToDevice, c->stream));
  ELP_HIP(c, elp::stream_wait(c->stream));
  c->have_rg_ids = true;
  return 0;
}

// cgo-friendly form: the ids behind each other, id_off[g] .. id_off[g + 1] = the bytes of read group g (n_rg + 1 offsets)
int elp_set_read_group_ids_flat(elp_ctx *c, const uint8_t *ids, const uint32_t *id_off) {
  if (!c || !c->have_header || (c->n_rg && (!ids || !id_off))) return set_error(c, ELP_ERR_ARG, "elp_set_read_group_ids_flat: call elp_set_header first");
  std::vector<std::string> str((size_t)c->n_rg);
  std::vector<const char *> ptr((size_t)c->n_rg + 1, nullptr);
  for (int g = 0; g < c->n_rg; g++) {
    if (id_off[g + 1] < id_off[g]) return set_error(c, ELP_ERR_ARG, "elp_set_read_group_ids_flat: id_off must not decrease");
    str[g].assign(reinterpret_cast<const char *>(ids) + id_off[g], id_off[g + 1] - id_off[g]);
    ptr[g] = str[g].c_str();
  }
  return elp_set_read_group_ids(c, ptr.data());
}

void *elp_pinned_alloc(size_t bytes) {
  void *p = nullptr;
  if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) return nullptr;
  return p;
}
void elp_pinned_free(void *p) {
  if (p) (void)hipHostFree(p);
}

int elp_stage_bam(elp_ctx *c, const uint8_t *bytes, uint64_t n_bytes, const uint64_t *rec_off, uint64_t n_records, uint16_t split_id) {
  if (!c || (!bytes && n_bytes)) return ELP_ERR_ARG;
  if (rec_off && (n_records == 0 ? n_bytes != 0 : (rec_off[0] != 0 || rec_off[n_records] != n_bytes)))
    return set_error(c, ELP_ERR_ARG, "elp_stage_bam: rec_off must run from 0 to n_bytes");
  std::lock_guard<std::mutex> g(c->stage_mu);
  ELP_HIP(c, hipSetDevice(c->device));
  if (!c->have_header) return set_error(c, ELP_ERR_ARG, "elp_stage_bam: call elp_set_header first");
  if (c->dict_replaced) return staging_refused_after_replace(c, "elp_stage_bam");
  if (c->n_rg && !c->have_rg_ids && !c->replace_rg) return set_error(c, ELP_ERR_ARG, "elp_stage_bam: call elp_set_read_group_ids first");
  if (c->n != c->raw_n) return set_error(c, ELP_ERR_ARG, "elp_stage_bam: the context already holds records staged with elp_stage");
  hipStream_t st = c->stream;
  // pieces are committed one at a time: whatever was derived from the records staged so far is invalid from here on, also if a later
  // piece fails
  c->derived.records_changed();
  if (!c->copy_stream) ELP_HIP(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
  // is the caller's buffer page-locked (elp_pinned_alloc / hipHostRegister)?  then the DMA engine reads it directly
  hipPointerAttribute_t pa;
  const bool pinned = n_bytes && hipPointerGetAttributes(&pa, bytes) == hipSuccess && pa.type == hipMemoryTypeHost;
  (void)hipGetLastError();
  constexpr size_t BOUNCE = 32ull << 20;
  if (!pinned && n_bytes && !c->bounce[0]) {
    for (int k = 0; k < 2; k++) {
      ELP_HIP(c, hipHostMalloc(&c->bounce[k], BOUNCE, hipHostMallocDefault));
      ELP_HIP(c, hipEventCreateWithFlags(&c->bounce_ev[k], hipEventDisableTiming));
    }
  }
  uint64_t at_byte = 0, at_rec = 0;
  uint64_t max_raw_rec = c->max_raw_rec;
  while (at_byte < n_bytes) {
    // record starts of this piece (<= 256 MiB of records: the device work unit): given by the caller (a BAM reader knows where every
    // record it hands over begins), else by a walk along the block_size chain
    BamCut cut = bam_cut_piece(bytes, n_bytes, rec_off, n_records, at_byte, at_rec);
    if (cut.error) return set_error(c, ELP_ERR_DATA, "%s", cut.text().c_str());
    std::vector<uint64_t> &off = cut.off;
    const uint64_t p = cut.end, piece_bytes = p - at_byte;
    const uint32_t n_rec = (uint32_t)(off.size() - 1);
    at_rec = cut.next_rec;
    max_raw_rec = std::max(max_raw_rec, cut.max_raw_rec);
    if (c->n + n_rec > 0xFFFFFFF0ull) return set_error(c, ELP_ERR_UNSUPPORTED, "more than 2^32-16 records per context");
    // raw bytes + record offsets into HBM (kept: elp_emit_sorted_bam reads bases and tags from them)
    ELP_TRY(ensure(c, c->raw, c->raw_bytes + piece_bytes + 64, true, c->raw_bytes));
    ELP_TRY(ensure(c, c->raw_off, c->n + n_rec + 2, true, c->n + 1));
    uint8_t *d_raw = c->raw.p + c->raw_bytes;
    if (pinned) {
      ELP_HIP(c, hipMemcpyAsync(d_raw, bytes + at_byte, piece_bytes, hipMemcpyHostToDevice, st));
    } else {
      // bounce: while the DMA engine moves buffer k, this thread fills buffer 1 - k
      int k = 0;
      for (uint64_t o = 0; o < piece_bytes; o += BOUNCE, k ^= 1) {
        const size_t len = (size_t)std::min<uint64_t>(BOUNCE, piece_bytes - o);
        ELP_HIP(c, hipEventSynchronize(c->bounce_ev[k]));
        memcpy(c->bounce[k], bytes + at_byte + o, len);
        ELP_HIP(c, hipMemcpyAsync(d_raw + o, c->bounce[k], len, hipMemcpyHostToDevice, c->copy_stream));
        ELP_HIP(c, hipEventRecord(c->bounce_ev[k], c->copy_stream));
      }
      ELP_HIP(c, elp::stream_wait(c->copy_stream));
    }
    for (auto &o : off) o += c->raw_bytes;  // offsets into c->raw
    ELP_HIP(c, hipMemcpyAsync(c->raw_off.p + c->n, off.data(), (size_t)(n_rec + 1) * 8, hipMemcpyHostToDevice, st));
    ELP_TRY(stage_bam_columns(c, n_rec, piece_bytes, c->raw_bytes + piece_bytes, max_raw_rec, split_id));
    at_byte = p;
  }
  ELP_HIP(c, elp::stream_wait(st));
  c->derived.records_changed();
  return 0;
}

}  // extern "C"
