// bgzf_plan.hpp — elp_stage_bgzf's plan as plain host arithmetic: the member headers of the (untrusted) file parsed into a block list,
// the cuts of that list into inflate pieces and scan pieces, the halving of a piece whose token scratch does not fit, the schedule of the
// host-to-device chunks, the layout of the two scratch slots and the words the kernels report in.  Nothing here touches the device or
// includes HIP: the header compiles with the host compiler alone (tests/bgzf_plan_host.cpp, tests/test_bgzf_plan_cpu.py, and
// tests/bgzf_parse_asan.cpp runs the parser under the sanitizers).  bgzf.hip, bgzf_inflate.hip and bgzf_records.hip take their sizes and
// offsets from here and compute none themselves.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace elp {

// ---- types and sizes the plan shares with the kernels (each is described beside its kernel)
struct BgzfBlk { uint64_t in_off; uint32_t in_len, out_len; uint64_t out_off; uint32_t crc; uint32_t pad; };  // CDATA in the piece; ISIZE; place in c->raw
static_assert(sizeof(BgzfBlk) == 32, "BgzfBlk is four 64-bit words");
constexpr uint32_t BGZF_PAYLOAD = 65280, BGZF_OVERHEAD = 31;  // bgzf_out.hip: a member's payload at most, the bytes around a stored one
// n_bytes of a stream as BGZF members of stored blocks: the bytes, and BGZF_OVERHEAD around every BGZF_PAYLOAD of them or part of it.
// The room bgzf_frame and bgzf_deflate (bgzf_out.hip) write into; a compressed member is never larger than its stored form.
inline uint64_t bgzf_framed_size(uint64_t n_bytes) { return n_bytes + (uint64_t)BGZF_OVERHEAD * ((n_bytes + BGZF_PAYLOAD - 1) / BGZF_PAYLOAD); }
constexpr uint32_t BGZF_SLOT = 65344;   // bgzf_out.hip: bytes between two slots (>= PAYLOAD + OVERHEAD, a multiple of 64)
constexpr uint32_t TOK_STRIDE = 21888;   // bgzf_inflate.hip: tokens per block: >= 65536 / 3 + 1, a multiple of 64
constexpr int RES_THREADS = 1024;        // bgzf_inflate.hip: k_bgzf_resolve's workgroup
constexpr uint32_t REC_BAD_CAP = 1024;   // bgzf_records.hip: rejected guesses that are listed (more: the repair goes through all blocks)

// ---- the member headers (utils/bgzf/bgzf-files.go:95-123): a few fields per 64 KB, read on the host from bytes nobody vouches for.
// Members with ISIZE 0 (the end-of-file block among them) are skipped, not listed; BC may stand behind other subfields; an end-of-file
// block is not required (it is the host's to insist on: a caller may hand over a file in several calls).
enum BgzfParseError { BGZF_PARSE_OK = 0, BGZF_TRUNCATED_HEADER, BGZF_NOT_BGZF, BGZF_TRUNCATED_EXTRA, BGZF_NO_BC, BGZF_BAD_SIZE, BGZF_ISIZE_TOO_BIG };
struct BgzfParse {
  BgzfParseError error = BGZF_PARSE_OK;
  uint64_t at = 0;       // the failing member's first byte
  uint32_t claimed = 0;  // BGZF_ISIZE_TOO_BIG: the ISIZE it claims
  std::vector<BgzfBlk> blocks;  // in_off: CDATA's place in the file; out_off: the block's place in the inflated stream
  uint64_t inflated = 0;
  // the text elp_stage_bgzf reports (status ELP_ERR_DATA)
  std::string text() const {
    static const char *const fmt[] = {"", "elp_stage_bgzf: truncated block header at byte %llu", "elp_stage_bgzf: not a BGZF block at byte %llu",
                                      "elp_stage_bgzf: truncated extra field at byte %llu", "missing BC extra subfield in BGZF header (block at byte %llu)",
                                      "elp_stage_bgzf: bad block size at byte %llu", "elp_stage_bgzf: block at byte %llu claims %u inflated bytes"};
    char buf[160];
    snprintf(buf, sizeof buf, fmt[error], (unsigned long long)at, claimed);
    return buf;
  }
};
inline BgzfParse bgzf_parse(const uint8_t *bgzf, uint64_t n_bytes) {
  BgzfParse r;
  auto fail = [&r](BgzfParseError e, uint64_t at, uint32_t claimed = 0) -> BgzfParse & {
    r.error = e;
    r.at = at;
    r.claimed = claimed;
    return r;
  };
  uint64_t p = 0;
  while (p < n_bytes) {
    if (p + 18 > n_bytes) return fail(BGZF_TRUNCATED_HEADER, p);
    const uint8_t *h = bgzf + p;
    if (h[0] != 0x1f || h[1] != 0x8b || h[2] != 8 || !(h[3] & 4)) return fail(BGZF_NOT_BGZF, p);
    const uint32_t xlen = h[10] | ((uint32_t)h[11] << 8);
    if (p + 12 + xlen > n_bytes) return fail(BGZF_TRUNCATED_EXTRA, p);
    uint32_t bsize = 0;
    for (uint32_t i = 0; i + 4 <= xlen;) {
      const uint32_t slen = h[12 + i + 2] | ((uint32_t)h[12 + i + 3] << 8);
      if (h[12 + i] == 66 && h[12 + i + 1] == 67 && slen == 2 && i + 6 <= xlen) { bsize = (h[12 + i + 4] | ((uint32_t)h[12 + i + 5] << 8)) + 1u; break; }
      i += 4 + slen;
    }
    if (!bsize) return fail(BGZF_NO_BC, p);
    if (bsize < 12 + xlen + 8 || p + bsize > n_bytes) return fail(BGZF_BAD_SIZE, p);
    uint32_t crc, isize;
    memcpy(&crc, bgzf + p + bsize - 8, 4);
    memcpy(&isize, bgzf + p + bsize - 4, 4);
    if (isize > 65536) return fail(BGZF_ISIZE_TOO_BIG, p, isize);
    if (isize) r.blocks.push_back(BgzfBlk{p + 12 + xlen, bsize - 12 - xlen - 8, isize, r.inflated, crc, 0});
    r.inflated += isize;
    p += bsize;
  }
  return r;
}

// ---- pieces.  Two sizes.  INFLATE pieces (<= 2 GiB inflated: ~33 k blocks) - the decoder wants every block of the file in flight at
// once (a wave per block, 24 of them per CU: 6.1 k blocks fill the chip once; round 6: 192 MiB pieces left it half empty and cost 1.7x)
// and pays 171 KB of token scratch per block for it.  Inside one, SCAN pieces (<= 1 GiB: u32 scans and bounded scratch in
// stage_bam_columns; round 6: 192 MiB pieces cost 7 x 2 host waits and launches of 3 k threads) find the records and stage the columns.
// Both are cut by one rule: from block `from`, blocks are taken up to `limit` while their inflated bytes stay within max_bytes; the
// first block is always taken.  Returns one past the last block taken.
inline size_t bgzf_cut(const BgzfBlk *blk, size_t from, size_t limit, uint64_t max_bytes) {
  size_t to = from;
  for (uint64_t out_bytes = 0; to < limit && (to == from || out_bytes + blk[to].out_len <= max_bytes); to++) out_bytes += blk[to].out_len;
  return to;
}

// the decoder's token scratch is 171 KB per block in flight: where the device's free memory does not hold it for the whole piece the
// launch takes half the blocks, and half of that ... (a part of 2 GiB wants 5.7 GB).  fits(nt) asks for the scratch of nt blocks;
// fail_above > 0 (the tuning key "bgzf_tok_fail_above": tests, this path without a full device) answers for it, without asking, that
// more than fail_above blocks do not fit.  nt = 0: one block does not fit either - `pretended` tells whether only the key said so.
struct BgzfTokFit { size_t nt; bool pretended; };
template <class Fits>
inline BgzfTokFit bgzf_tok_fit(size_t nt, int fail_above, Fits &&fits) {
  for (;; nt /= 2) {
    const bool pretend = fail_above > 0 && nt > (size_t)fail_above;
    if (!pretend && fits(nt)) return BgzfTokFit{nt, false};
    if (nt <= 1) return BgzfTokFit{0, pretend};
  }
}

// ---- the chunks of an inflate piece of `na` blocks.  The compressed bytes cross PCIe in chunks of blocks on the copy stream, each
// chunk's decoder launch waits for its own chunk only: the decoder works on chunk k while chunk k + 1 arrives.  A chunk = the blocks that
// fill the chip once (24 waves per CU) unless "bgzf_copy_chunk" says otherwise; the first one is 1 / "bgzf_first_chunk_div" of that (the
// decoder starts early; a divisor below 1 counts as 1).  The chunks' launches alternate between the context's stream and a lane of its own (the sort lane:
// idle while records are staged): a launch behind another on ONE stream starts when the last wave of the one in front has finished - a
// block takes 4.5 ms, the chip drains for half of that per launch -; on two streams the next chunk's waves take the slots as they come
// free.  The lane is taken only where there is more than one full chunk, and by the odd turns.
struct BgzfChunks {
  struct Turn { uint32_t q0, q1; bool side; };  // blocks [q0, q1) of the piece; side: launched on the lane
  uint32_t chunk, first;
  bool lane;  // the piece needs the side lane
  std::vector<Turn> turns;
  BgzfChunks(uint32_t na, int copy_chunk, int first_chunk_div, int n_cu)
      : chunk(copy_chunk > 0 ? (uint32_t)copy_chunk : std::max(1024u, (uint32_t)n_cu * 24u)),
        first(std::max(1u, chunk / (uint32_t)std::max(1, first_chunk_div))), lane(na > chunk) {
    uint32_t turn = 0;
    for (uint32_t q0 = 0, q1 = 0; q0 < na; q0 = q1, turn++) {
      q1 = std::min(na, q0 + (turn == 0 ? first : chunk));
      turns.push_back(Turn{q0, q1, lane && (turn & 1u)});
    }
  }
};

// the inflated length most blocks of a piece have (Boyer-Moore majority vote; any value is correct - k_bgzf_resolve takes its CRC
// powers for that length from a table -, the common one is fast)
inline uint32_t bgzf_common_len(const BgzfBlk *blk, size_t n) {
  uint32_t n_common = blk[0].out_len, votes = 0;
  for (size_t k = 0; k < n; k++) {
    if (votes == 0) { n_common = blk[k].out_len; votes = 1; }
    else if (blk[k].out_len == n_common) votes++;
    else votes--;
  }
  return n_common;
}

// ---- the words the kernels report in, at the head of slot 6's `res`; the host reads them back as they stand here
struct BgzfRes {
  uint32_t err;      // (unused: no kernel of the scan writes it)
  uint32_t bad;      // k_rec_check: guesses it rejected
  uint32_t max_rec;  // k_rec_fill: the longest record of the scan piece, block_size field included
  uint32_t unused[5];
  uint32_t inflate;  // k_bgzf_tokens, k_bgzf_resolve: INFLATE_* bits.  A word of its own: the scan pieces clear theirs, this one lives as long as the inflate piece
  uint32_t unused2;
  static constexpr size_t CLEAR_PIECE = 64, CLEAR_SCAN = 16;  // bytes zeroed when an inflate piece / a scan piece begins
};
constexpr uint32_t INFLATE_BAD_DATA = 1u, INFLATE_BAD_CRC = 2u;  // a block does not inflate (k_bgzf_tokens); a block's CRC-32 differs (k_bgzf_resolve)
static_assert(offsetof(BgzfRes, bad) == 4 && offsetof(BgzfRes, max_rec) == 8 && offsetof(BgzfRes, inflate) == 32 && sizeof(BgzfRes) == 40, "the result words' places");

// ---- the scratch blocks of an inflate piece of `na` blocks.  Who owns a slot of elp_ctx::scratch:
//   slot 5  the piece's compressed bytes            from the chunks' copies to the last k_bgzf_tokens
//   slot 6  blk | entry | exit | res | cnt | base | bad_list      the inflate piece: blk from its upload on, res.inflate from the decoder
//           to the first scan piece's read-back; the others belong to the scan pieces, each to its blocks' elements [b0 - a0, b1 - a0)
//   slot 7  tokens | ntok | pow_common               k_crc_pow_common / k_bgzf_tokens to k_bgzf_resolve
// Slot 6 in 64-bit words: the block table, 4 na words, at 0 | entry, na | exit, na | res, 8 words | and as 32-bit words behind res:
// cnt, na + 8 | base, na + 8 | bad_list, REC_BAD_CAP.  The request leaves 16 words behind bad_list.  (entry stands at byte 32 na, the
// 32-bit part at byte 48 na + 64: 8-byte aligned for every na.)
struct BgzfScratch6 {
  size_t entry, exit, res;      // 64-bit words from the slot's start
  size_t cnt, base, bad_list;   // 32-bit words from the slot's start
  size_t words64;               // the request
  explicit BgzfScratch6(uint32_t na)
      : entry((size_t)na * 4), exit(entry + na), res(exit + na), cnt(2 * (res + 8)), base(cnt + na + 8), bad_list(base + na + 8),
        words64((size_t)na * 6 + 8 + (size_t)(na + 8) + 16 + REC_BAD_CAP / 2) {}
};
// Slot 7 in tokens (8 bytes each): every block's TOK_STRIDE tokens | and as 32-bit words behind them: ntok, na rounded up to even |
// pow_common, RES_THREADS.  The request leaves 8 elements behind pow_common.
struct BgzfScratch7 {
  size_t ntok;        // tokens (8-byte elements) from the slot's start
  size_t pow_common;  // 32-bit words behind ntok
  size_t elems;       // the request, in tokens
  explicit BgzfScratch7(size_t na) : ntok(na * TOK_STRIDE), pow_common((na + 1) & ~(size_t)1), elems(na * TOK_STRIDE + (na + 2) / 2 + RES_THREADS / 2 + 8) {}
};

}  // namespace elp
