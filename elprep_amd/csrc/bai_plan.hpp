// bai_plan.hpp — the plan of elp_index_sorted_bgzf / elp_index_merged_bgzf (bai.hip) as plain host arithmetic: the member table of the
// (untrusted) BGZF bytes a caller hands back, the virtual offset of a stream position, the size of a contig's part of the index and of
// the whole, the check that the bytes are the context's stream, and the layout of the call's scratch.  Nothing here touches the device or
// includes HIP: the header compiles with the host compiler alone (tests/bai_plan_host.cpp, tests/test_bai_plan_cpu.py, and
// tests/bai_plan_asan.cpp runs the member walk under the sanitizers).  bai.hip takes its sizes and offsets from here and computes none
// itself; the functions its kernels call are constexpr.
//
// The index is the SAM specification's section 5.2 in ONE canonical form (include/elprep_hip.h states it in full): bins ascending, the
// chunks of a bin merged where a record starts in the member the chunk ends in, the pseudo-bin last, every linear-index entry defined.
#pragma once
#include "bgzf_plan.hpp"

namespace elp {

constexpr uint32_t BAI_PSEUDO_BIN = 37450;     // the bin number above every real one: its two chunks hold the contig's extent and counts
constexpr uint32_t BAI_WINDOW_SHIFT = 14;      // linear-index windows of 16384 positions
constexpr uint64_t BAI_MAX_END = 1ull << 29;   // the largest end a bin number can express
constexpr uint64_t BAI_MAX_COFFSET = 1ull << 48;  // a virtual offset holds 48 bits of file offset

// ---- the member table: coff[m] = the first byte of member m in `bgzf`, coff[n_members] = n_bytes.  The members are the emitters'
// (bgzf_out.hip): the 18-byte header 1f 8b 08 04 | MTIME XFL OS | XLEN 6 | 'B' 'C' 2 0 | BSIZE, then CDATA, CRC-32 and ISIZE; every
// member but the last holds BGZF_PAYLOAD bytes, the last 1 .. BGZF_PAYLOAD.  An empty stream has no members.  Only these fields are read -
// the payload is never inflated -, from bytes nobody vouches for: nothing outside [bgzf, bgzf + n_bytes) is touched.
enum BaiMemberError { BAI_MEMBERS_OK = 0, BAI_TRUNCATED_MEMBER, BAI_NOT_A_MEMBER, BAI_BAD_BSIZE, BAI_SHORT_MEMBER, BAI_BAD_LAST_ISIZE };
struct BaiMembers {
  BaiMemberError error = BAI_MEMBERS_OK;
  uint64_t at = 0;       // the byte the refusal names: the member's first (TRUNCATED, NOT_A_MEMBER), its BSIZE field, its ISIZE field
  uint32_t value = 0;    // BAD_BSIZE: BSIZE + 1; SHORT_MEMBER, BAD_LAST_ISIZE: the ISIZE read
  std::vector<uint64_t> coff;  // n_members + 1
  uint64_t inflated = 0;       // the sum of the members' ISIZE
  size_t n_members() const { return coff.empty() ? 0 : coff.size() - 1; }
  // the text the index calls report (status ELP_ERR_DATA)
  std::string text(const char *who) const {
    static const char *const fmt[] = {"", "%s: truncated BGZF member at byte %llu", "%s: not a BGZF member with the BC subfield first at byte %llu",
                                      "%s: the member size at byte %llu (%u) runs past the end or is too small",
                                      "%s: the ISIZE at byte %llu is %u: every member but the last holds 65280 bytes",
                                      "%s: the last member's ISIZE at byte %llu is %u, not 1 .. 65280"};
    char buf[200];
    snprintf(buf, sizeof buf, fmt[error], who, (unsigned long long)at, value);
    return buf;
  }
};
constexpr uint32_t BAI_MEMBER_MIN = 18 + 8;  // header, CRC-32 and ISIZE around no CDATA at all
inline BaiMembers bai_members(const uint8_t *bgzf, uint64_t n_bytes) {
  BaiMembers r;
  auto fail = [&r](BaiMemberError e, uint64_t at, uint32_t value = 0) -> BaiMembers & {
    r.error = e;
    r.at = at;
    r.value = value;
    r.coff.clear();
    r.inflated = 0;
    return r;
  };
  static const uint8_t head[4] = {0x1f, 0x8b, 0x08, 0x04}, sub[6] = {0x06, 0x00, 0x42, 0x43, 0x02, 0x00};  // magic; XLEN, SI1 SI2, SLEN
  uint64_t p = 0;
  r.coff.push_back(0);
  while (p < n_bytes) {
    if (n_bytes - p < 18) return fail(BAI_TRUNCATED_MEMBER, p);
    const uint8_t *h = bgzf + p;
    if (memcmp(h, head, 4) != 0 || memcmp(h + 10, sub, 6) != 0) return fail(BAI_NOT_A_MEMBER, p);
    const uint32_t bsize = (h[16] | ((uint32_t)h[17] << 8)) + 1u;
    if (bsize < BAI_MEMBER_MIN || bsize > n_bytes - p) return fail(BAI_BAD_BSIZE, p + 16, bsize);
    uint32_t isize;
    memcpy(&isize, h + bsize - 4, 4);
    const bool last = p + bsize == n_bytes;
    if (!last && isize != BGZF_PAYLOAD) return fail(BAI_SHORT_MEMBER, p + bsize - 4, isize);
    if (last && (isize == 0 || isize > BGZF_PAYLOAD)) return fail(BAI_BAD_LAST_ISIZE, p + bsize - 4, isize);
    r.inflated += isize;
    p += bsize;
    r.coff.push_back(p);
  }
  return r;
}

// ---- a position p of the inflated stream as a virtual offset: the file offset of its member (the host writes the members at
// base_coffset, behind its header blocks) in the high 48 bits, the place inside the member's payload in the low 16.  A record that ends
// with its member ends at place 0 of the next one - at coff[n_members] for the stream's last record.
constexpr uint64_t bai_voff(uint64_t base_coffset, const uint64_t *coff, uint64_t p) {
  return ((base_coffset + coff[p / BGZF_PAYLOAD]) << 16) | (p % BGZF_PAYLOAD);
}
// the offsets fit 48 bits wherever the host puts the stream
inline bool bai_coffsets_fit(uint64_t base_coffset, uint64_t n_bytes) { return base_coffset < BAI_MAX_COFFSET && n_bytes < BAI_MAX_COFFSET - base_coffset; }
// the bytes are this context's stream: the members' ISIZE add up to the length the device's size pass found
inline bool bai_is_the_stream(const BaiMembers &m, uint64_t stream_bytes) { return m.error == BAI_MEMBERS_OK && m.inflated == stream_bytes; }

// ---- sizes.  A contig without records: n_bin = 0, n_intv = 0.  One with records: n_bin | per bin: bin, n_chunk, its chunks (beg, end) |
// the pseudo-bin with its two chunks | n_intv | the windows' offsets.
constexpr uint64_t BAI_PSEUDO_BYTES = 8 + 2 * 16;
constexpr uint64_t bai_contig_bytes(uint64_t n_records, uint64_t n_bins, uint64_t n_chunks, uint64_t n_intv) {
  return n_records ? 4 + 8 * n_bins + 16 * n_chunks + BAI_PSEUDO_BYTES + 4 + 8 * n_intv : 8;
}
// where the parts of a contig with records stand, from the contig's first byte
constexpr uint64_t bai_bin_at(uint64_t bins_before, uint64_t chunks_before) { return 4 + 8 * bins_before + 16 * chunks_before; }
constexpr uint64_t bai_chunk_at(uint64_t bins_before_and_own, uint64_t chunks_before) { return 4 + 8 * bins_before_and_own + 16 * chunks_before; }
constexpr uint64_t bai_intv_at(uint64_t n_bins, uint64_t n_chunks) { return 4 + 8 * n_bins + 16 * n_chunks + BAI_PSEUDO_BYTES; }
// the whole: "BAI\1", n_ref | the contigs | n_no_coor
constexpr uint64_t BAI_HEAD_BYTES = 8, BAI_TAIL_BYTES = 8;
constexpr uint64_t bai_total_bytes(uint64_t contig_bytes) { return BAI_HEAD_BYTES + contig_bytes + BAI_TAIL_BYTES; }
// the closed form of the same, from the index's totals (n_used: contigs with records)
constexpr uint64_t bai_size(uint64_t n_ref, uint64_t n_used, uint64_t n_bins, uint64_t n_chunks, uint64_t n_intv) {
  return BAI_HEAD_BYTES + 8 * (n_ref - n_used) + n_used * (8 + BAI_PSEUDO_BYTES) + 8 * n_bins + 16 * n_chunks + 8 * n_intv + BAI_TAIL_BYTES;
}

// ---- the scratch of one call, for n_out output records, n_ref contigs and n_members members.  Who owns a slot of elp_ctx::scratch:
//   slot 4  sizes | offs | err          the size passes, as emit_stream runs them (EmitScratch4), one pass at a time
//   slot 6  src | is_spread | before    the merged form: emit_merged's list (emit.hip), read by every size pass and by k_bai_records
//   slot 5  the merged form: merge_spread_slots' keys and slots, dead once the list is made; the sorted form of a keep permutation: the
//           keys of the order check
//   slot 0  the per-record block (BaiScratch0), from the first size pass to the last kernel
//   slot 1  the radix sort's second key and value buffers
//   slot 2  the result words, the member table, the per-contig block and the scans' partial sums (BaiScratch2)
//   slot 3  the index, as it goes to the caller
// All in units of 8 bytes from the slot's start, so that every 64-bit array is aligned.
struct BaiScratch0 {
  size_t start, key, gmax;                                               // arrays of n + 1 64-bit words
  size_t size, val, head_bin, head_chunk, bins, chunks, unm, unms, bin_chunk0;  // arrays of n + 1 32-bit words, 8 spare words behind each
  size_t words64;
  // start: S of record k as a stream position (entry n: the stream's length) | key: refid << 16 | bin | gmax: refid << 15 | last
  // window, then its running maximum | size: the record's bytes | val: k | head_bin, head_chunk: 1 = the first of its bin / its chunk in
  // the sorted list | bins, chunks: their exclusive sums (entry n: the totals) | unm: FLAG & 4 in output order, unms: its exclusive
  // sums | bin_chunk0: per bin, the chunks in front of its first
  explicit BaiScratch0(uint64_t n) {
    const size_t n1 = (size_t)n + 1, half = (n1 + 1) / 2 + 4;
    start = 0;
    key = start + n1;
    gmax = key + n1;
    size = gmax + n1;
    val = size + half;
    head_bin = val + half;
    head_chunk = head_bin + half;
    bins = head_chunk + half;
    chunks = bins + half;
    unm = chunks + half;
    unms = unm + half;
    bin_chunk0 = unms + half;
    words64 = bin_chunk0 + half;
  }
};
struct BaiScratch1 {
  size_t key, val, words64;
  explicit BaiScratch1(uint64_t n) : key(0), val((size_t)n + 1), words64((size_t)n + 1 + ((size_t)n + 2) / 2 + 4) {}
};
struct BaiRes {  // the words the kernels report in, read back as they stand here
  uint64_t contig_bytes;   // k_bai_contig_offsets: the contigs' parts together
  uint32_t n_placed;       // k_bai_records: output records with refid >= 0 (they stand in front of the others)
  uint32_t err;            // k_bai_records: BAI_ERR_* bits
  uint64_t unused[2];
};
static_assert(sizeof(BaiRes) == 32, "BaiRes is four 64-bit words");
constexpr uint32_t BAI_ERR_END = 1u, BAI_ERR_REFID = 2u, BAI_ERR_ORDER = 4u;  // an end beyond 2^29; a refid outside the dictionary; refids that descend
constexpr uint32_t BAI_SCAN_TILE = 2048;  // elements per workgroup of bai.hip's 64-bit scans (256 threads, 8 each)
struct BaiScratch2 {
  size_t res, coff, first, end, bytes, offset, partials, words64;  // 64-bit words from the slot's start
  // res: BaiRes | coff: the member table (n_members + 1) | first, end: per contig its records [first, end) among the output, 32 bits |
  // bytes: per contig bai_contig_bytes | offset: their exclusive sums | partials: one sum per tile of the longer of the two scans (the
  // running maximum over the records, the sum over the contigs)
  BaiScratch2(uint64_t n_ref, uint64_t n_members, uint64_t n_out) {
    const size_t half = ((size_t)n_ref + 1) / 2 + 4;
    res = 0;
    coff = res + sizeof(BaiRes) / 8;
    first = coff + (size_t)n_members + 1;
    end = first + half;
    bytes = end + half;
    offset = bytes + (size_t)n_ref + 1;
    partials = offset + (size_t)n_ref + 1;
    words64 = partials + (size_t)(std::max(n_ref, n_out) / BAI_SCAN_TILE) + 2;
  }
};

}  // namespace elp
