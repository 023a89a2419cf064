// bgzf.hpp — what the stages of elp_stage_bgzf (bgzf.hip) share: an inflate piece as it stands on the device and the two phase
// functions, bgzf_inflate_piece (bgzf_inflate.hip) and bgzf_scan_piece (bgzf_records.hip).  Sizes and offsets: bgzf_plan.hpp.
#pragma once
#include "common.hpp"
#include "bgzf_plan.hpp"

namespace elp {

// events between the context's stream and its copy stream, destroyed when the call returns (also on an error path)
struct CopyEvents {
  std::vector<hipEvent_t> ev;
  ~CopyEvents() { for (auto e : ev) (void)hipEventDestroy(e); }
  int next(elp_ctx *c, hipEvent_t *out) {
    hipEvent_t e;
    ELP_HIP(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    ev.push_back(e);
    *out = e;
    return 0;
  }
  // `to` waits for everything queued on `from` so far
  int fence(elp_ctx *c, hipStream_t from, hipStream_t to) {
    hipEvent_t e;
    ELP_TRY(next(c, &e));
    ELP_HIP(c, hipEventRecord(e, from));
    ELP_HIP(c, hipStreamWaitEvent(to, e, 0));
    return 0;
  }
  int arrived(elp_ctx *c, hipStream_t copy, hipStream_t st) { return fence(c, copy, st); }
};

// an inflate piece: `na` blocks whose inflated bytes are queued into c->raw, and their tables in scratch slot 6 (BgzfScratch6).  The scan
// pieces inside it work on the elements [rel, rel + nb) of every table.
struct BgzfPiece {
  uint32_t na = 0;
  std::vector<BgzfBlk> tb;  // the block table as the device holds it: in_off from the piece's first compressed byte, out_off in c->raw
  const BgzfBlk *blk = nullptr;
  uint64_t *entry = nullptr, *exit = nullptr;
  BgzfRes *res = nullptr;
  uint32_t *cnt = nullptr, *base = nullptr, *bad_list = nullptr;
  bool inflate_checked = true;  // res->inflate was read back and found clear (the first scan piece's read-back does it)
};
int bgzf_inflate_piece(elp_ctx *c, const uint8_t *bgzf, const BgzfBlk *blocks, size_t n, uint64_t raw0, CopyEvents &copied, BgzfPiece *piece);

// what a scan piece found: the complete records that start in it, c->raw_off[c->n ..] filled with their starts
struct BgzfScan {
  uint32_t n_rec;
  uint64_t rec_end;  // one past the last complete record: the next piece's first record
  uint32_t max_rec;  // the longest record, block_size field included
};
int bgzf_scan_piece(elp_ctx *c, BgzfPiece &piece, size_t rel, uint32_t nb, uint64_t begin, BgzfScan *out);

}  // namespace elp
