"""SAM text out beside BAM out on the same N reads of the c3 read set, in one run on one box: the emitters' kernels alone through profile()
(HIP events, best of 5) and the whole calls (best of 5, each ending in a sync), bytes written and rates.  usage: sam_out_speed.py [reads]"""
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
e.mark_duplicates(True, fetch=False)
e.sort_coordinate(fetch=False)
print(f"{b.n} reads, {raw.size} bytes of staged records, coordinate order")


def measure(emit, sizes_name, emit_name, out):
    emit(out)
    calls, ks = [], []
    for _ in range(5):
        t0 = time.perf_counter()
        r = emit(out)
        e.sync()
        calls.append(time.perf_counter() - t0)
    for _ in range(5):
        e.profile_enable(True)
        e.profile_reset()
        emit(out)
        e.sync()
        p = e.profile()
        e.profile_enable(False)
        ks.append((p[sizes_name][1], p[emit_name][1], p[sizes_name][0]))
    return r.size, min(calls) * 1e3, min(k[0] for k in ks), min(k[1] for k in ks), ks[0][2]


res = {}
for fmt, emit, names, room in (("bam", e.emit_sorted_bam, ("emit_bam_sizes", "emit_bam"), int(raw.size * 1.02) + (1 << 20)),
                               ("sam", e.emit_sorted_sam, ("emit_sam_sizes", "emit_sam"), int(1.8 * raw.size) + (1 << 20))):
    out = np.empty(room, np.uint8)
    n_bytes, t_call, t_sizes, t_emit, passes = measure(emit, *names, out)
    res[fmt] = (n_bytes, t_sizes, t_emit)
    k = t_sizes + t_emit
    print(f"emit_sorted_{fmt}: {n_bytes} bytes in {passes} passes; kernels {names[0]} {t_sizes:.3f} ms + {names[1]} {t_emit:.3f} ms = {k:.3f} ms: "
          f"{b.n / k / 1e3:.0f} Mreads/s, {n_bytes / k / 1e6:.0f} GB/s written; whole call with the copy to the host {t_call:.1f} ms")
    del out
(bb, bs, be), (sb, ss, se) = res["bam"], res["sam"]
print(f"sam / bam: bytes {sb / bb:.2f}, size kernel {ss / bs:.2f}, emit kernel {se / be:.2f}, both kernels {(ss + se) / (bs + be):.2f}")
e.close()
