"""SAM text in beside BAM in on the same N reads of the c3 read set, in one run on one box: elp_stage_sam of the text elp_emit_sorted_sam
wrote and elp_stage_bam of the same records, both from page-locked memory; the whole calls (best of 3, each ending in a sync) and the
kernels by stage through profile() (HIP events, one profiled call behind an untimed first one); at the end the text is staged once more
and emitted again, which must give the same bytes (the text is cut into pieces of 256 MiB: their borders).  usage: sam_in_speed.py [reads]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from elprep_amd.engine import Engine  # noqa: E402
from tools import synth  # noqa: E402

reads = int(sys.argv[1]) if len(sys.argv) > 1 else 16_000_000
cfg = synth.config("c3")
h = cfg.header()
b = synth.generate(cfg, 0, reads // 2)
raw, off = synth.bam_records(b, h.rg_ids)

e = Engine(h, 0)
e.set_read_group_ids(h.rg_ids)
e.set_reference_names()
e.stage_bam(raw, rec_off=off)
e.order_keep(fetch=False)
text = e.emit_sorted_sam(e.pinned_zeros(int(1.8 * raw.size) + (1 << 20), np.uint8))
pinned_raw = e.pinned_zeros(raw.size, np.uint8)
pinned_raw[:] = raw
e.reset()
print(f"{b.n} reads: {text.size} bytes of SAM text, {raw.size} bytes of BAM records, input order, both in page-locked memory")


def measure(stage, n_bytes):
    stage()                                                # untimed: buffers grow, the name table is made
    e.sync()
    e.reset()
    calls = []
    for _ in range(3):
        t0 = time.perf_counter()
        stage()
        e.sync()
        calls.append(time.perf_counter() - t0)
        assert e.n == b.n
        e.reset()
    e.profile_enable(True)
    e.profile_reset()
    stage()
    e.sync()
    p = e.profile()
    e.profile_enable(False)
    e.reset()
    total = sum(ms for _, ms in p.values())
    t = min(calls) * 1e3
    print(f"  whole call {t:.1f} ms: {b.n / t / 1e3:.1f} Mreads/s, {n_bytes / t / 1e6:.1f} GB/s of input; kernels {total:.1f} ms: {b.n / total / 1e3:.1f} Mreads/s")
    for name, (launches, ms) in sorted(p.items(), key=lambda kv: -kv[1][1]):
        print(f"    {name:24s} {launches:5d} launches {ms:9.3f} ms  {100 * ms / total:5.1f} %")
    return t, total


print("elp_stage_sam")
ts, ks = measure(lambda: e.stage_sam(text), text.size)
print("elp_stage_bam (record offsets given)")
tb, kb = measure(lambda: e.stage_bam(pinned_raw, rec_off=off), raw.size)
print(f"sam / bam: bytes {text.size / raw.size:.2f}, whole call {ts / tb:.2f}, kernels {ks / kb:.2f}")
# the pieces' borders (the text is cut every 256 MiB): what was staged from the text goes out as the same text
e.stage_sam(text)
e.order_keep(fetch=False)
again = e.emit_sorted_sam()
print("staged from text and emitted again: %s" % ("the same bytes" if np.array_equal(again, text) else "DIFFERENT BYTES"))
e.close()
