// bqsr_prologue.hip — the BQSR gather's per-record prologue: three passes, one thread per record, in front of either count kernel.
//
// Reference: recalibrateAln (filters/bqsr.go:225-244), hardClipAdaptorSequence / hardClipSoftClippedBases (filters/utils.go:149-548),
// calculateSkipSlice (bqsr.go:389-414), computeStrandedClippedSeq's mask bounds (bqsr.go:316-332); the device helpers are in bqsr_dev.hpp.
//
//   k_bqsr_prologue_fast   streams over every staged record: eligibility, and the whole prologue for CIGARs of the form
//                          [H] [S] <match> [S] [H] that need no adaptor clipping (about 5 of 6 reads); reads of match / insertion /
//                          deletion operations are listed for the second pass, everything else is queued for the third
//   k_bqsr_prologue_plain  the listed reads, densely: reference pieces and known-site read coordinates on the CIGAR as staged
//   k_bqsr_prologue        the queued reads: clipping on a working copy of the CIGAR, more than three pieces, adaptor clips
// A pass leaves, per record, the 32-byte descriptor of k_bqsr_count (bqsr_count.hip) or - RecOut.recs set - the 32-byte record of
// k_bqsr_count3 (count3.hip), and the record's known-site bits in the 1-bit-per-base skip column.  prologue_launch queues the three.
#include "bqsr_common.hpp"

namespace elp {

struct BqCols {
  uint64_t n;
  const int32_t *refid, *pos, *next_refid, *pnext, *tlen;
  const uint16_t *flag, *rgid;
  const uint8_t *mapq, *has_sr;
  const uint32_t *l_seq;
  const uint64_t *cigar_off, *seq_off, *qual_off;
  const uint32_t *cigar;
  const uint8_t *seq4;
  const uint8_t *qual;
  const int32_t *ref_len;
  const uint16_t *rg_cov;
  int32_t n_ref;
  uint8_t *const *ref_seq;
  const int64_t *ref_seq_len;
  int32_t *const *sites;
  const int64_t *n_sites;
  uint32_t *const *site_idx;  // per contig and 64-bp bucket: first site whose end is >= 64 * bucket (k_site_index)
  const uint64_t *qbounds;    // per record: low-quality-tail bounds of the full read (adapt_score)
};

// recalibrateAln, bqsr.go:225-244 (+ utils.go:121-139)
__device__ inline bool recalibrate_aln(const BqCols &m, uint64_t i) {
  if (m.has_sr[i]) return false;
  const uint8_t mq = m.mapq[i];
  if (!(mq > 0 && mq < 255)) return false;
  const uint16_t f = m.flag[i];
  if (f & (F_SECONDARY | F_DUPLICATE | F_QCFAILED)) return false;
  const int32_t r = m.refid[i], p = m.pos[i];
  if ((f & F_UNMAPPED) || r < 0 || p == 0) return false;
  if (!(p > 0)) return false;
  const uint32_t ls = m.l_seq[i];
  if (ls == 0) return false;
  if ((uint64_t)ls != m.qual_off[i + 1] - m.qual_off[i]) return false;
  if (m.rgid[i] == ELP_NIL16) return false;
  if (!(r < m.n_ref && p <= m.ref_len[r])) return false;
  int32_t rl = 0, refl = 0;
  for (uint64_t k = m.cigar_off[i]; k < m.cigar_off[i + 1]; k++) {
    const uint32_t c = m.cigar[k];
    if (c_op(c) == OP_N) return false;
    if (op_consumes_read(c_op(c))) rl += c_len(c);
    if (op_consumes_ref(c_op(c))) refl += c_len(c);
  }
  return refl >= 0 && (int32_t)ls == rl;
}

// pieces of the clipped CIGAR; false if it needs more than three
__device__ inline bool build_pieces(const uint32_t *cig, int ncig, int32_t pos, BqDesc &d) {
  int64_t val[3];
  bool noref[3];
  int start[3];
  int np = 0;
  int c = 0;
  int64_t delta = (int64_t)pos - 1;  // reference index minus clipped read index for the current match run
  for (int i = 0; i < ncig; i++) {
    const uint32_t op = c_op(cig[i]);
    const int ln = c_len(cig[i]);
    if (op == OP_M || op == OP_EQ || op == OP_X) {
      if (ln > 0 && (np == 0 || noref[np - 1] || val[np - 1] != delta)) {
        if (np == 3) return false;
        val[np] = delta; noref[np] = false; start[np] = c; np++;
      }
      c += ln;
    } else if (op == OP_I || op == OP_S) {
      if (ln > 0 && (np == 0 || !noref[np - 1])) {
        if (np == 3) return false;
        val[np] = 0; noref[np] = true; start[np] = c; np++;
      }
      c += ln;
      delta -= ln;
    } else if (op == OP_D || op == OP_N) {
      delta += ln;
    }
  }
  int32_t D[3] = {BQ_NOREF, BQ_NOREF, BQ_NOREF};
  for (int k = 0; k < np; k++) {
    if (noref[k]) continue;
    if (val[k] <= (int64_t)INT32_MIN + 70000 || val[k] >= (int64_t)INT32_MAX - 70000) return false;
    D[k] = (int32_t)val[k];
  }
  d.D0 = D[0]; d.D1 = D[1]; d.D2 = D[2];
  d.b1 = np > 1 ? (uint16_t)start[1] : (uint16_t)0xFFFF;
  d.b2 = np > 2 ? (uint16_t)start[2] : (uint16_t)0xFFFF;
  return true;
}

// marks bases [fs, fe] of the record whose first QUAL byte is at bit0 in the skip column
__device__ __forceinline__ void set_skip_bits(uint32_t *skipbits, uint64_t bit0, int fs, int fe) {
  for (int k = fs; k <= fe;) {  // word by word
    const uint64_t b = bit0 + (uint64_t)k;
    const int in_word = (int)(b & 31);
    int cnt = 32 - in_word;
    if (cnt > fe - k + 1) cnt = fe - k + 1;
    const uint32_t mask = (cnt == 32 ? 0xFFFFFFFFu : ((1u << cnt) - 1u)) << in_word;
    atomicOr(&skipbits[b >> 5], mask);
    k += cnt;
  }
}

// clears the bits of bases [0, nbits) of the record whose first QUAL byte is at bit0.  Round 6: when RECORDS are written (count3.hip) only the
// reads that put known-site bits into the column ever read it (RC_SKIPCOL), and only their own bits - such a read clears its range before
// it sets bits, and the fill of the whole column (a bit per staged base: 0.14 ms per 50 M reads) is made for the descriptor form only.
// Neighbouring reads share words, never bits: atomics on the words, in program order per thread.
__device__ __forceinline__ void clear_skip_bits(uint32_t *skipbits, uint64_t bit0, uint32_t nbits) {
  for (uint32_t k = 0; k < nbits;) {
    const uint64_t b = bit0 + (uint64_t)k;
    const uint32_t in_word = (uint32_t)(b & 31);
    uint32_t cnt = 32 - in_word;
    if (cnt > nbits - k) cnt = nbits - k;
    const uint32_t mask = (cnt == 32 ? 0xFFFFFFFFu : ((1u << cnt) - 1u)) << in_word;
    atomicAnd(&skipbits[b >> 5], ~mask);
    k += cnt;
  }
}

// Fast prologue, one thread per record.  Decides eligibility (recalibrateAln) for every record and finishes the records whose
// CIGAR is a single M/=/X operation and that need no adaptor clipping (≈ 5 of 6 reads): for those the clipped copy is the read
// itself, getReadCoordinateForReferenceCoordinate(ref) is ref - POS inside the read and fails outside (utils.go:267-349 with one
// match operation), and there is one reference piece.  Everything else is appended to `queue` for the general kernel, so that
// kernel's long divergent code runs with all lanes busy.  All column loads are issued before the first test (one latency, not 15).
// (PF_TILES: bqsr_plan.hpp)
// a record's columns (k_bqsr_prologue_fast loads them a tile ahead)
struct PfCols {
  uint8_t has_sr, mq;
  uint16_t f, rg;
  int32_t r, p, pnext, tlen, nrefid;
  uint32_t ls;
  uint64_t q0, q1, c0, c1, qb;
};
__device__ __forceinline__ PfCols pf_load_cols(const BqCols &m, uint64_t i) {
  PfCols c;
  c.has_sr = m.has_sr[i]; c.mq = m.mapq[i]; c.f = m.flag[i]; c.rg = m.rgid[i];
  c.r = m.refid[i]; c.p = m.pos[i]; c.pnext = m.pnext[i]; c.tlen = m.tlen[i]; c.nrefid = m.next_refid[i];
  c.ls = m.l_seq[i];
  c.q0 = m.qual_off[i]; c.q1 = m.qual_off[i + 1]; c.c0 = m.cigar_off[i]; c.c1 = m.cigar_off[i + 1];
  c.qb = m.qbounds[i];
  return c;
}
// per-contig facts in LDS (contig length, known-site array, its length, its bucket index): the walk over the known sites then depends on
// ONE global round trip (the bucket entry) instead of three (pointer tables first)
struct PfLds {
  int32_t ref_len[REF_LDS];
  const int32_t *sites[REF_LDS];
  int64_t nsites[REF_LDS];
  const uint32_t *sidx[REF_LDS];
};
__device__ __forceinline__ void pf_lds_fill(PfLds &L, const BqCols &m, int nt) {
  if (m.n_ref <= REF_LDS)
    for (int r = threadIdx.x; r < m.n_ref; r += nt) { L.ref_len[r] = m.ref_len[r]; L.sites[r] = m.sites[r]; L.nsites[r] = m.n_sites[r]; L.sidx[r] = m.site_idx[r]; }
}

// The prologue of ONE record.  PLAIN_PASS false: the first, streaming pass - finishes the reads whose CIGAR is [H] [S] <match> [S] [H], sends
// reads of match / insertion / deletion operations to the second pass (to_plain) and everything else to the general kernel (defer).
// PLAIN_PASS true: the second pass over the reads the first one listed; my_cig_w = five LDS words of the thread.
template <bool PLAIN_PASS>
__device__ __forceinline__ void pf_record(const BqCols &m, const uint64_t i, const PfCols &cur, const PfLds &L, const bool ref_lds, BqDesc *__restrict__ desc,
                                          uint32_t *skipbits, uint32_t *err, const bool recs /* records, not descriptors */, uint32_t *my_cig_w, bool &defer, bool &to_plain,
                                          BqRec &rc_out, int &rc_class, uint4 *__restrict__ plain_rec /* first pass: where a read of the second pass leaves its columns */,
                                          const uint32_t *pre_ops /* second pass: the read's five CIGAR operation slots, handed over */) {
    const uint8_t has_sr = cur.has_sr, mq = cur.mq;
    const uint16_t f = cur.f, rg = cur.rg;
    const int32_t r = cur.r, p = cur.p, pnext = cur.pnext, tlen = cur.tlen, nrefid = cur.nrefid;
    const uint32_t ls = cur.ls;
    const uint64_t q0 = cur.q0, q1 = cur.q1, c0 = cur.c0, c1 = cur.c1;
    const uint64_t qb = cur.qb;
    BqDesc d;
    d.D0 = d.D1 = d.D2 = BQ_NOREF; d.refid = 0; d.b1 = d.b2 = 0xFFFF; d.a = 0; d.len = 0; d.left = 0; d.right = 0; d.cov = 0; d.fl = 0; d.pad = 0;
    const uint8_t *rec_rp = nullptr;
    int64_t rec_rlen = 0;
    bool used_col = false, rec_skipped_walk = false;  // known-site bits of the read went into the skip column; no walk: they come with the reference window
    // recalibrateAln, bqsr.go:225-244 (+ utils.go:121-139), the part that needs no dependent load
    bool ok = !has_sr && mq > 0 && mq < 255 && !(f & (F_SECONDARY | F_DUPLICATE | F_QCFAILED)) && !(f & F_UNMAPPED) && r >= 0 && p > 0 && ls != 0 &&
              (uint64_t)ls == q1 - q0 && rg != ELP_NIL16 && r < m.n_ref;
    if (ok) {
      // CIGARs of the form [H] [S] <match> [S] [H] (one M/=/X operation, clips only at the ends: plain reads and soft-clipped ones):
      // hardClipSoftClippedBases (utils.go:519-548) leaves the match operation between hard clips, i.e. the clipped copy is bases
      // [aoff, aoff + len) of the read with ONE reference piece starting at POS, softStart = POS, softEnd = End, and
      // getReadCoordinateForReferenceCoordinate is ref - POS inside it.  All five operation slots are read at once.
      const uint64_t nop = c1 - c0;
      if (recs) { rec_rp = m.ref_seq[r]; rec_rlen = m.ref_seq_len[r]; }  // issued with the CIGAR loads: one round trip for both
      uint32_t opv[5];
#pragma unroll
      for (int k = 0; k < 5; k++) opv[k] = PLAIN_PASS ? pre_ops[k] : ((uint64_t)k < nop ? m.cigar[c0 + k] : 0u);
      const int32_t rl = ref_lds ? L.ref_len[r] : m.ref_len[r];
      // the same round trip: the read group's covariate index and - when descriptors are written - the known-site bucket entry (read
      // whether or not the tests below pass).  When RECORDS are written (count3.hip) a read that is one run of matches needs no walk over
      // the site list: its known-site bits come with the reference window (k_ref_mark_sites); the bucket entry is then fetched only by the
      // reads that do walk (indels; a window the record cannot describe)
      const uint16_t cov_rg = m.rg_cov[rg];
      const int32_t *sv = ref_lds ? L.sites[r] : m.sites[r];
      const int64_t ns = ref_lds ? L.nsites[r] : m.n_sites[r];
      auto bucket_entry = [&]() __attribute__((always_inline)) -> int64_t {
        const int64_t nbuck = ((int64_t)rl >> 6) + 1;
        int64_t bk = (int64_t)(p < rl ? p : rl) >> 6;
        bk = bk >= nbuck ? nbuck - 1 : bk;
        return (int64_t)(ref_lds ? L.sidx[r] : m.site_idx[r])[bk];
      };
      int64_t s_first = 0;
      if (!recs && ns > 0) s_first = bucket_entry();
      ok = p <= rl;
      bool simple = nop >= 1 && nop <= 5;
      uint32_t aoff = 0, mlen = 0, trail = 0;
      {
        uint32_t k = 0;
        if (simple && c_op(opv[0]) == OP_H) k = 1;
        // (select chains on purpose: opv[] indexed by a variable would move the array to scratch memory)
        auto at = [&](uint32_t j) { return j == 0 ? opv[0] : (j == 1 ? opv[1] : (j == 2 ? opv[2] : (j == 3 ? opv[3] : opv[4]))); };
        if (simple && k < nop && c_op(at(k)) == OP_S) { aoff = (uint32_t)c_len(at(k)); k++; }
        if (simple && k < nop && (c_op(at(k)) == OP_M || c_op(at(k)) == OP_EQ || c_op(at(k)) == OP_X)) { mlen = (uint32_t)c_len(at(k)); k++; }
        else simple = false;
        if (simple && k < nop && c_op(at(k)) == OP_S) { trail = (uint32_t)c_len(at(k)); k++; }
        if (simple && k < nop && c_op(at(k)) == OP_H) k++;
        simple = simple && k == nop && mlen != 0;
      }
      // CIGARs of match / insertion / deletion operations only (two to five of them: reads with an indel or two): nothing is clipped
      // unless the adaptor test says so, the window is the whole read; reference pieces and read coordinates of known sites come
      // from the same device functions the general kernel uses, on the CIGAR as staged
      bool plain = false;
      uint32_t plain_read = 0, plain_ref = 0;
      if (!simple && nop >= 2 && nop <= 5) {
        plain = true;
#pragma unroll
        for (int k = 0; k < 5; k++) {
          if ((uint64_t)k < nop) {
            const uint32_t o = c_op(opv[k]), ln = (uint32_t)c_len(opv[k]);
            if (o == OP_M || o == OP_EQ || o == OP_X) { plain_read += ln; plain_ref += ln; }
            else if (o == OP_I) plain_read += ln;
            else if (o == OP_D) plain_ref += ln;
            else plain = false;
          }
        }
      }
      if (!PLAIN_PASS) {
        // first pass: a read with indels goes to the second, dense pass (k_bqsr_prologue_plain) - a wave that holds one would otherwise
        // run the piece / read-coordinate code for all of its lanes (the kernel is bound by vector issue: 1250 instructions per wave and
        // tile with both paths in one kernel, profiles/round3 PMC)
        if (ok && plain && ls <= (uint32_t)MAX_DESC_READ) {
          // the columns this thread holds go along in ONE 64-byte line at the read's own place (round 6): the second pass gathered them
          // again from fifteen columns - 850 bytes of sectors per listed read, 0.52 ms for the 7.5 % of the reads that have an indel
          uint4 *pr = plain_rec + 4 * i;
          pr[0] = make_uint4(opv[0], opv[1], opv[2], opv[3]);
          pr[1] = make_uint4(opv[4], (uint32_t)f | ((uint32_t)rg << 16), (uint32_t)r, (uint32_t)p);
          pr[2] = make_uint4(ls | ((uint32_t)nop << 16) | (nrefid < 0 ? 1u << 19 : 0u), (uint32_t)c0, (uint32_t)q0, (uint32_t)(q0 >> 32));
          pr[3] = make_uint4((uint32_t)qb, (uint32_t)(qb >> 32), (uint32_t)pnext, (uint32_t)tlen);
          to_plain = true;
          return;
        }
        plain = false;
      } else if (plain) {
#pragma unroll
        for (int k = 0; k < 5; k++) my_cig_w[k] = opv[k];
      }
      const uint32_t *my_cig = my_cig_w;
      if (ok && !((simple || plain) && ls <= (uint32_t)MAX_DESC_READ)) { defer = true; ok = false; }  // the general kernel redoes the tests
      if (ok) ok = (plain ? plain_read : aoff + mlen + trail) == ls;  // SEQ length == CIGAR read length (utils.go:121-128)
      if (ok) {
        const int len = plain ? (int)ls : (int)mlen;
        const int32_t end = p + (plain ? (int)plain_ref : len) - 1;  // aln.End() (sam/sam-types.go:769-775)
        // hardClipAdaptorSequence (utils.go:149-180, 214-222) would clip?
        const bool rev = f & F_REVERSED;
        bool clip = false;
        if (tlen != 0 && (f & F_MULTIPLE) && !((f & F_NEXT_UNMAPPED) || nrefid < 0 || pnext == 0) && rev != (bool)(f & F_NEXT_REVERSED)) {
          const bool well = rev ? end > pnext : p <= pnext + tlen;
          if (well) {
            const int boundary = rev ? (int)pnext - 1 : (int)p + (tlen < 0 ? -(int)tlen : (int)tlen);
            clip = boundary >= (int)p && boundary <= (int)end;
          }
        }
        // computeStrandedClippedSeq mask bounds (bqsr.go:316-332) inside the window: adapt_score recorded the first / last quality > 2
        // of the whole read; where that lies outside the window the window's own end decides (if it does not: general kernel)
        const uint32_t hi1 = (uint32_t)qb;
        int left = len, right = len - 1;
        if (!clip && hi1) {
          const int f0 = (int)(qb >> 32) - (int)aoff, l0 = (int)hi1 - 1 - (int)aoff;  // relative to the window; f0 <= l0
          if (f0 < len && l0 >= 0) {
            if (f0 >= 0) left = f0;
            else if (m.qual[q0 + aoff] > 2) left = 0;
            else clip = true;
            if (l0 < len) right = l0;
            else if (m.qual[q0 + aoff + (uint32_t)len - 1] > 2) right = len - 1;
            else clip = true;
          }
        }
        if (clip) {
          defer = true;
        } else {
          // calculateSkipSlice (bqsr.go:389-414): softStart = POS, softEnd = End
          // (records: a plain run of matches whose window the record describes takes its known-site bits from the reference window)
          const bool rec_simple = recs && !plain && len <= 1022 && (int64_t)p - 1 - (int64_t)aoff >= 16 && (int64_t)p - 1 - (int64_t)aoff + (int64_t)ls <= rec_rlen + 32;
          rec_skipped_walk = ns > 0 && rec_simple;
          if (ns > 0 && !rec_simple) {
            if (recs) s_first = bucket_entry();
            // the first two candidate sites in one round trip (most reads touch none or one); any further ones from memory
            const int2 *sv2 = reinterpret_cast<const int2 *>(sv);
            int64_t s = s_first;
            const int2 cand0 = s < ns ? sv2[s] : make_int2(0, 0), cand1 = s + 1 < ns ? sv2[s + 1] : make_int2(0, 0);
            int sk_x = cand0.x, sk_y = cand0.y;  // site s
            auto fetch = [&]() __attribute__((always_inline)) {
              if (s == s_first + 1) { sk_x = cand1.x; sk_y = cand1.y; }
              else if (s < ns) { const int2 t = sv2[s]; sk_x = t.x; sk_y = t.y; }
            };
            while (s < ns && sk_y < p) { s++; fetch(); }
            for (; s < ns && sk_x <= end; s++, fetch()) {
              struct { int x, y; } sk = {sk_x, sk_y};
              int fs, fe;
              if (plain) {
                bool okc;
                fs = get_read_coord(my_cig, (int)nop, (int)p, sk.x, false, &okc);
                if (!okc || fs < 0) fs = 0;
                fe = get_read_coord(my_cig, (int)nop, (int)p, sk.y, false, &okc);
                if (!okc || fe > len - 1) fe = len - 1;
              } else {
                const int a0 = sk.x - p, a1 = sk.y - p;
                fs = (a0 < 0 || a0 >= len) ? 0 : a0;          // !ok || < 0 -> 0
                fe = (a1 < 0 || a1 >= len) ? len - 1 : a1;    // !ok || > len-1 -> len-1 (a1 < 0 cannot happen: End >= POS)
              }
              if (recs && !used_col) clear_skip_bits(skipbits, q0, ls);
              set_skip_bits(skipbits, q0 + aoff, fs, fe);
              used_col = true;
            }
          }
          d.D0 = p - 1;
          d.refid = r;
          d.a = (uint16_t)aoff;
          d.len = (uint16_t)len;
          uint8_t complex_fl = 0;
          if (plain && !build_pieces(my_cig, (int)nop, p, d)) {  // more than three pieces: the count kernel walks the CIGAR
            complex_fl = BQ_COMPLEX;
            d.D0 = (int32_t)c0;
            d.b1 = (uint16_t)nop;
            d.D2 = p - 1;
          }
          d.left = (uint16_t)left; d.right = (uint16_t)(right < 0 ? 0xFFFF : right);
          d.cov = (uint8_t)cov_rg;
          d.fl = BQ_ELIGIBLE | (rev ? BQ_REVERSED : 0) | ((f & F_LAST) ? BQ_LAST : 0) | complex_fl;
        }
      }
    }
    if (!defer) {
      if (recs) {  // the record count3.hip works from; BqDesc only for the reads the record cannot describe
        BqRec rc;
        rc.ref_lo = rc.ref_hi = rc.win = rc.ctxw = 0; rc.t0 = 0; rc.fl = rc.bpk = rc.dpk = 0;
        if (d.fl & BQ_ELIGIBLE) {
          Pieces4 P;
          if (d.fl & BQ_COMPLEX) pieces4(my_cig_w, (int)(c1 - c0), p, P);
          else if (d.b1 != 0xFFFFu) pieces4(my_cig_w, (int)(c1 - c0), p, P);
          else { P.v0 = (int64_t)d.D0; P.v1 = P.v2 = P.v3 = 0; P.s1 = P.s2 = P.s3 = 0; P.noref = d.D0 == BQ_NOREF ? 1u : 0u; P.np = 1; }
          rc = make_rec((int)d.a, (int)d.len, (int)d.left, d.right == 0xFFFFu ? -1 : (int)d.right, d.cov, (d.fl & BQ_REVERSED) != 0, (d.fl & BQ_LAST) != 0, P,
                        P.np < 0, rec_rp, rec_rlen, (int64_t)ls);
          if (used_col) rc.fl |= RC_SKIPCOL;
          else if ((rc.fl & RC_GENERAL) && rec_skipped_walk) atomicOr(&err[0], 1024u);  // (cannot happen: rec_simple restates make_rec's tests)
        }
        if (rc.fl & RC_GENERAL) desc[i] = d;
        rc_class = rec_class(rc);
        rec_pack_idx(rc, (uint32_t)i);
        rc_out = rc;
      } else {
        desc[i] = d;
      }
    }
}

// First pass, one thread per record; all column loads are issued before the first test (one latency, not 15), a tile ahead.
__global__ __launch_bounds__(256) void k_bqsr_prologue_fast(BqCols m, BqDesc *__restrict__ desc, uint32_t *skipbits, uint32_t *__restrict__ queue,
                                                            uint32_t *queue_n, uint32_t *err, RecOut ro, uint32_t *__restrict__ plist, uint4 *__restrict__ plain_rec) {
  // a workgroup handles PF_TILES * 256 consecutive records and collects the deferred ones in LDS - the general kernel's from the front of
  // the list, the second pass's from its end: one global atomic per workgroup and list (a global atomic per wave on a single counter
  // serialises at ~12 ns each: 9 ms for 50 M reads)
  __shared__ uint32_t lq[PF_TILES * 256];
  __shared__ uint32_t lcount, gbase, pcount, pbase;
  __shared__ uint32_t seg_n[C3_MAXSEG], seg_at[C3_MAXSEG];  // covariate-split segments: the tile's class-1 records per covariate, their first place
  __shared__ PfLds L;
  const bool ref_lds = m.n_ref <= REF_LDS;
  pf_lds_fill(L, m, 256);
  if (threadIdx.x == 0) { lcount = 0; pcount = 0; }
  seg_n[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t i_first = (uint64_t)blockIdx.x * PF_TILES * 256 + threadIdx.x;
  PfCols nxt = {};
  if (i_first < m.n) nxt = pf_load_cols(m, i_first);
#pragma unroll 1
  for (int tile = 0; tile < PF_TILES; tile++) {
    const uint64_t i = i_first + (uint64_t)tile * 256;
    bool defer = false, to_plain = false;
    const PfCols cur = nxt;
    if (tile + 1 < PF_TILES && i + 256 < m.n) nxt = pf_load_cols(m, i + 256);
    BqRec rc;
    int rcl = 0;
    if (i < m.n) pf_record<false>(m, i, cur, L, ref_lds, desc, skipbits, err, ro.recs != nullptr, nullptr, defer, to_plain, rc, rcl, plain_rec, nullptr);
    if (ro.recs) {  // the tile's records, compacted: class 1 into this wave's segment, the rare class 2 ones (windows the record cannot describe) behind
      if (!ro.ncs) {
        const uint32_t seg = (blockIdx.x * 4u + (threadIdx.x >> 6)) % ro.nseg;  // the wave's segment
        const uint32_t at1 = wave_append(rcl == 1, &ro.cnt[seg * C3_CSTRIDE]);
        if (rcl == 1) rec_store(ro.recs, (uint64_t)ro.seg_base[seg] + at1, rc);
      } else {
        // segments by covariate: the workgroup's class-1 records of this tile take their rank among those of their covariate from a
        // returning LDS atomic, then ONE global atomic per covariate that occurs reserves the places in segment (workgroup % groups, covariate)
        // (measured with the reservation taken out: the global atomics WERE the cost of many read groups - one per wave and covariate,
        // 4 M / 7 M of them at 16 / 32 read groups and 16 M reads, 0.74 / 0.98 ms against 0.41 / 0.43 without)
        const uint32_t cov = rc.fl & 0xFFu, seg = (blockIdx.x % (ro.nseg / ro.ncs)) * ro.ncs + cov;
        uint32_t rank = 0;
        if (rcl == 1) rank = atomicAdd(&seg_n[cov], 1u);
        __syncthreads();
        if (threadIdx.x < ro.ncs) {
          const uint32_t t = seg_n[threadIdx.x];
          if (t) {
            seg_at[threadIdx.x] = atomicAdd(&ro.cnt[((blockIdx.x % (ro.nseg / ro.ncs)) * ro.ncs + threadIdx.x) * C3_CSTRIDE], t);
            seg_n[threadIdx.x] = 0;
          }
        }
        __syncthreads();
        if (rcl == 1) rec_store(ro.recs, (uint64_t)ro.seg_base[seg] + seg_at[cov] + rank, rc);
      }
      const uint32_t at2 = wave_append(rcl == 2, &ro.cnt[ro.nseg * C3_CSTRIDE]);
      if (rcl == 2) rec_store(ro.recs, ro.other_at + at2, rc);
    }
    const int lane = threadIdx.x & 63;
    const unsigned long long mask = __ballot(defer);
    if (mask) {  // one LDS atomic per wave
      const int leader = __ffsll((long long)mask) - 1;
      uint32_t base = 0;
      if (lane == leader) base = atomicAdd(&lcount, (uint32_t)__popcll(mask));
      base = __shfl(base, leader, 64);
      if (defer) lq[base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = (uint32_t)i;
    }
    const unsigned long long pmask = __ballot(to_plain);
    if (pmask) {
      const int leader = __ffsll((long long)pmask) - 1;
      uint32_t base = 0;
      if (lane == leader) base = atomicAdd(&pcount, (uint32_t)__popcll(pmask));
      base = __shfl(base, leader, 64);
      if (to_plain) lq[PF_TILES * 256 - 1 - (base + (uint32_t)__popcll(pmask & ((1ull << lane) - 1ull)))] = (uint32_t)i;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    gbase = lcount ? atomicAdd(queue_n, lcount) : 0u;
    pbase = pcount ? atomicAdd(queue_n + 1, pcount) : 0u;
  }
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < lcount; k += 256) queue[gbase + k] = lq[k];
  for (uint32_t k = threadIdx.x; k < pcount; k += 256) plist[pbase + k] = lq[PF_TILES * 256 - 1 - k];
}

// Second pass: the reads of match / insertion / deletion operations, one thread per listed read (every lane of a wave does the same
// kind of work); the list's length stays on the device.  A read this pass cannot finish either (adaptor geometry) joins the general
// kernel's queue: one global atomic per workgroup and trip.
__global__ __launch_bounds__(256) void k_bqsr_prologue_plain(BqCols m, BqDesc *__restrict__ desc, uint32_t *skipbits, const uint32_t *__restrict__ plist,
                                                             uint32_t *__restrict__ queue, uint32_t *queue_n, uint32_t *err, RecOut ro, const uint4 *__restrict__ plain_rec) {
  __shared__ uint32_t s_cig[256][5];  // the thread's CIGAR: build_pieces / get_read_coord walk it several times
  __shared__ uint32_t wg_n, wg_base, wr_n, wr_base;
  __shared__ PfLds L;
  const bool ref_lds = m.n_ref <= REF_LDS;
  pf_lds_fill(L, m, 256);
  __syncthreads();
  const uint64_t np = (uint64_t)queue_n[1];
  const uint64_t stride = (uint64_t)gridDim.x * 256;
  for (uint64_t t0 = (uint64_t)blockIdx.x * 256; t0 < np; t0 += stride) {  // (uniform trip count per workgroup: barriers inside)
    const uint64_t t = t0 + threadIdx.x;
    bool defer = false, to_plain = false;
    uint32_t i = 0;
    BqRec rc;
    int rcl = 0;
    if (t < np) {
      i = plist[t];
      // the read's columns as the first pass left them (pf_record<false>): one 64-byte line
      const uint4 *pr = plain_rec + 4 * (size_t)i;
      const uint4 w0 = pr[0], w1 = pr[1], w2 = pr[2], w3 = pr[3];
      const uint32_t ops[5] = {w0.x, w0.y, w0.z, w0.w, w1.x};
      PfCols cur;
      cur.has_sr = 0; cur.mq = 1;  // (the first pass made recalibrateAln's tests)
      cur.f = (uint16_t)w1.y; cur.rg = (uint16_t)(w1.y >> 16);
      cur.r = (int32_t)w1.z; cur.p = (int32_t)w1.w;
      cur.ls = w2.x & 0xFFFFu;
      cur.nrefid = (w2.x >> 19) & 1u ? -1 : 0;  // (only its sign is looked at)
      cur.c0 = (uint64_t)w2.y; cur.c1 = cur.c0 + ((w2.x >> 16) & 7u);
      cur.q0 = (uint64_t)w2.z | ((uint64_t)w2.w << 32); cur.q1 = cur.q0 + cur.ls;
      cur.qb = (uint64_t)w3.x | ((uint64_t)w3.y << 32);
      cur.pnext = (int32_t)w3.z; cur.tlen = (int32_t)w3.w;
      pf_record<true>(m, i, cur, L, ref_lds, desc, skipbits, err, ro.recs != nullptr, s_cig[threadIdx.x], defer, to_plain, rc, rcl, nullptr, ops);
    }
    // deferred reads -> the general kernel's queue, finished records (all class 2 here... or 1 if the CIGAR folded to one run) -> the other
    // region: one global atomic each per workgroup and trip
    if (threadIdx.x == 0) { wg_n = 0; wr_n = 0; }
    __syncthreads();
    uint32_t my = 0, myr = 0;
    if (defer) my = atomicAdd(&wg_n, 1u);
    if (rcl) myr = atomicAdd(&wr_n, 1u);
    __syncthreads();
    if (threadIdx.x == 0) {
      wg_base = wg_n ? atomicAdd(queue_n, wg_n) : 0u;
      wr_base = wr_n ? atomicAdd(&ro.cnt[ro.nseg * C3_CSTRIDE], wr_n) : 0u;
    }
    __syncthreads();
    if (defer) queue[wg_base + my] = i;
    if (rcl) rec_store(ro.recs, ro.other_at + wr_base + myr, rc);
  }
}

// General prologue: one thread per record of `queue` (the records k_bqsr_prologue_fast left: anything but a plain "<len>M" CIGAR
// without adaptor read-through); literal transliteration of the reference's clipping code.
__device__ inline void prologue_general(const BqCols &m, const uint64_t i, uint32_t *__restrict__ cig_scratch, BqDesc *__restrict__ desc, uint32_t *skipbits,
                                        uint32_t *err, const bool recs, BqRec &rc_out, int &rc_class) {
  int32_t rec_pos = 0;  // POS of the clipped copy (set before the final put)
  // stores the descriptor, or - recs != nullptr - the record count3.hip works from (and the descriptor only if the record cannot
  // describe the read)
  auto put = [&](const BqDesc &dd, const uint32_t *cg, int ncg) {
    if (!recs) { desc[i] = dd; return; }
    BqRec rc;
    rc.ref_lo = rc.ref_hi = rc.win = rc.ctxw = 0; rc.t0 = 0; rc.fl = rc.bpk = rc.dpk = 0;
    if (dd.fl & BQ_ELIGIBLE) {
      Pieces4 P;
      pieces4(cg, ncg, rec_pos, P);
      rc = make_rec((int)dd.a, (int)dd.len, (int)dd.left, dd.right == 0xFFFFu ? -1 : (int)dd.right, dd.cov, (dd.fl & BQ_REVERSED) != 0, (dd.fl & BQ_LAST) != 0, P,
                    P.np < 0, m.ref_seq[dd.refid], m.ref_seq_len[dd.refid], (int64_t)m.l_seq[i]);
      rc.fl |= RC_SKIPCOL;  // this kernel's reads have their known-site bits in the skip column
    }
    if (rc.fl & RC_GENERAL) desc[i] = dd;
    rc_class = rec_class(rc) ? 2 : 0;  // (this kernel's reads read the skip column)
    rec_pack_idx(rc, (uint32_t)i);
    rc_out = rc;
  };
  BqDesc d;
  d.D0 = d.D1 = d.D2 = BQ_NOREF; d.refid = 0; d.b1 = d.b2 = 0xFFFF; d.a = 0; d.len = 0; d.left = 0; d.right = 0; d.cov = 0; d.fl = 0; d.pad = 0;
  if (!recalibrate_aln(m, i)) { { put(d, nullptr, 0); return; } }
  if (m.l_seq[i] > (uint32_t)MAX_DESC_READ) { atomicOr(&err[0], 2u); { put(d, nullptr, 0); return; } }
  RAln a;
  a.pos = m.pos[i]; a.pnext = m.pnext[i]; a.tlen = m.tlen[i]; a.refid = m.refid[i]; a.next_refid = m.next_refid[i];
  a.flag = m.flag[i];
  a.cig = m.cigar + m.cigar_off[i];
  a.ncig = (int)(m.cigar_off[i + 1] - m.cigar_off[i]);
  a.off = 0; a.len = (int)m.l_seq[i];
  uint32_t *sc = cig_scratch + 2 * (m.cigar_off[i] + 4 * i);
  a.buf[0] = sc; a.buf[1] = sc + (a.ncig + 4);
  a.cur = -1;
  if (!hard_clip_adaptor(a)) { atomicOr(&err[0], 4u); { put(d, nullptr, 0); return; } }
  if (a.len == 0) { { put(d, nullptr, 0); return; } }
  hard_clip_soft_clipped(a);
  if (a.len == 0) { { put(d, nullptr, 0); return; } }

  // calculateSkipSlice, bqsr.go:389-414: bits live at (qual_off[i] + original base index)
  {
    const int ss = soft_start(a), se = soft_end(a);
    const int32_t *sv = m.sites[a.refid];
    const int64_t ns = m.n_sites[a.refid];
    // intervals.Intersect (intervals/intervals.go:166-173): sites with End >= softStart and Start <= softEnd.  The bucket index
    // replaces the two binary searches (28 dependent loads) by one look-up and a short walk.
    int64_t first = ns, last = ns;
    if (ns > 0) {
      const int64_t nbuck = ((int64_t)m.ref_len[a.refid] >> 6) + 1;
      int64_t bk = (int64_t)(ss < 0 ? 0 : ss) >> 6;
      bk = bk >= nbuck ? nbuck - 1 : bk;
      first = m.site_idx[a.refid][bk];
      while (first < ns && sv[2 * first + 1] < ss) first++;
      last = first;
      while (last < ns && sv[2 * last] <= se) last++;
    }
    const uint64_t bit0 = m.qual_off[i] + (uint64_t)a.off;
    if (recs) clear_skip_bits(skipbits, m.qual_off[i], m.l_seq[i]);  // (this kernel's reads all read the column, RC_SKIPCOL)
    for (int64_t s = first; s < last; s++) {
      bool ok;
      int fs = get_read_coord(a.cig, a.ncig, ss, sv[2 * s], false, &ok);
      if (!ok || fs < 0) fs = 0;
      int fe = get_read_coord(a.cig, a.ncig, ss, sv[2 * s + 1], false, &ok);
      if (!ok || fe > a.len - 1) fe = a.len - 1;
      set_skip_bits(skipbits, bit0, fs, fe);
    }
  }
  ReadView v{m.seq4 + m.seq_off[i], m.qual + m.qual_off[i], a.off, a.len, (bool)(a.flag & F_REVERSED), 0, -1};
  low_quality_bounds(v);
  d.refid = a.refid;
  d.a = (uint16_t)a.off; d.len = (uint16_t)a.len;
  d.left = (uint16_t)v.left; d.right = (uint16_t)(v.right < 0 ? 0xFFFF : v.right);
  d.cov = (uint8_t)m.rg_cov[m.rgid[i]];
  d.fl = BQ_ELIGIBLE | ((a.flag & F_REVERSED) ? BQ_REVERSED : 0) | ((a.flag & F_LAST) ? BQ_LAST : 0);
  rec_pos = a.pos;
  if (!build_pieces(a.cig, a.ncig, a.pos, d)) {
    d.fl |= BQ_COMPLEX;
    if (a.cur < 0) { d.D0 = (int32_t)m.cigar_off[i]; }
    else { d.D0 = (int32_t)(a.buf[a.cur] - cig_scratch); d.fl |= BQ_CIG_SCRATCH; }
    d.b1 = (uint16_t)a.ncig;
    d.D2 = a.pos - 1;
    if (a.ncig > 0xFFFF) atomicOr(&err[0], 2u);
  }
  put(d, a.cig, a.ncig);
}

// the queue's length stays on the device (no read-back between the two prologue kernels): a fixed grid strides over it
__global__ __launch_bounds__(256) void k_bqsr_prologue(BqCols m, const uint32_t *__restrict__ queue, const uint32_t *__restrict__ queue_n,
                                                       uint32_t *__restrict__ cig_scratch, BqDesc *__restrict__ desc, uint32_t *skipbits,
                                                       uint32_t *err, RecOut ro) {
  __shared__ uint32_t wr_n, wr_base;
  const uint64_t nq = (uint64_t)*queue_n;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t t0 = (uint64_t)blockIdx.x * blockDim.x; t0 < nq; t0 += stride) {  // (uniform trip count per workgroup: barriers inside)
    const uint64_t t = t0 + threadIdx.x;
    BqRec rc;
    int rcl = 0;
    if (t < nq) prologue_general(m, queue[t], cig_scratch, desc, skipbits, err, ro.recs != nullptr, rc, rcl);
    if (!ro.recs) continue;
    if (threadIdx.x == 0) wr_n = 0;
    __syncthreads();
    uint32_t myr = 0;
    if (rcl) myr = atomicAdd(&wr_n, 1u);
    __syncthreads();
    if (threadIdx.x == 0) wr_base = wr_n ? atomicAdd(&ro.cnt[ro.nseg * C3_CSTRIDE], wr_n) : 0u;
    __syncthreads();
    if (rcl) rec_store(ro.recs, ro.other_at + wr_base + myr, rc);
  }
}

// the three passes over the staged records; with ro.recs they leave 32-byte records for count3.hip, without it the descriptors of k_bqsr_count
int prologue_launch(elp_ctx *c, const PrologueBufs &b, const GatherScratch &S, const RecOut &ro) {
  const uint64_t n = c->n;
  BqCols m{n, c->refid.p, c->pos.p, c->next_refid.p, c->pnext.p, c->tlen.p, c->flag.p, c->rgid.p, c->mapq.p, c->has_sr.p, c->l_seq.p,
           c->cigar_off.p, c->seq_off.p, c->qual_off.p, c->cigar.p, c->seq4.p, c->qual.p, c->ref_len.p, c->rg_cov.p, c->n_ref,
           c->d_ref_seq.p, c->d_ref_seq_len.p, c->d_sites.p, c->d_n_sites.p, c->d_site_idx.p, c->qbounds.p};
  uint32_t *queue_n = b.block, *queue = b.block + S.queue, *plist = b.block + S.plist;
  ELP_LAUNCH(c, "bqsr_prologue_fast", k_bqsr_prologue_fast, dim3(S.pf_grid), dim3(256), 0, m, b.desc, b.skipbits, queue, queue_n, c->err_flag.p, ro, plist, b.plain_rec);
  // (sized for the worst case; workgroups beyond the list's end leave at once)
  const unsigned grid = std::min<unsigned>(blocks_for(n, 256), (unsigned)c->n_cu * 16);
  ELP_LAUNCH(c, "bqsr_prologue_plain", k_bqsr_prologue_plain, dim3(grid), dim3(256), 0, m, b.desc, b.skipbits, (const uint32_t *)plist, queue, queue_n, c->err_flag.p, ro,
             (const uint4 *)b.plain_rec);
  ELP_LAUNCH(c, "bqsr_prologue", k_bqsr_prologue, dim3(grid), dim3(256), 0, m, (const uint32_t *)queue, (const uint32_t *)queue_n, b.cs_pool, b.desc, b.skipbits,
             c->err_flag.p, ro);
  return 0;
}

}  // namespace elp
