"""elp_index_sorted_bgzf next to the elp_emit_sorted_bgzf call it follows, on N reads of the c3 set: wall time and per-kernel times of both,
the index's size and its chunk count.  usage: bai_speed.py [reads] [check]
(check: the index against tests/bairef.py's, which walks every record in Python - for a few hundred thousand reads)"""
import ctypes as C
import os
import struct
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from elprep_amd.engine import Engine, _vp  # noqa: E402
from tools import synth  # noqa: E402

reads = int(sys.argv[1]) if len(sys.argv) > 1 else 16_000_000
cfg = synth.config("c3")
h = cfg.header()
b = synth.generate(cfg, 0, reads // 2)
raw, rec_off = synth.bam_records(b, h.rg_ids)
e = Engine(h, 0)
e.set_read_group_ids(h.rg_ids)
e.stage_bam(raw, rec_off=rec_off)
e.mark_duplicates(True, fetch=False)
e.sort_coordinate(fetch=False)


def timed(call, repeats=3):
    """-> (best wall time, the profile of the best run, the result)"""
    best = None
    for _ in range(repeats):
        e.sync()
        e.profile_enable(True)
        e.profile_reset()
        t0 = time.perf_counter()
        out = call()
        t = time.perf_counter() - t0
        prof = e.profile()
        e.profile_enable(False)
        if best is None or t < best[0]:
            best = (t, prof, out)
    return best


def kernels(prof, top=12):
    rows = sorted(((k, v) for k, v in prof.items() if v[0]), key=lambda kv: -kv[1][1])[:top]
    return "  " + "\n  ".join(f"{k:24s} {int(v[0]):4d} launches {v[1]:9.3f} ms" for k, v in rows) + f"\n  all kernels {sum(v[1] for v in prof.values()):.3f} ms"


e.emit_sorted_bgzf()  # (allocations)
t_emit, p_emit, bz = timed(e.emit_sorted_bgzf)
bai = e.index_sorted_bgzf(bz, 4096)  # (allocations, and the size: the timed call below is ONE call into a buffer of that size)


def index_once():
    n = C.c_uint64()
    e._check(e.L.elp_index_sorted_bgzf(e.h, _vp(bz), bz.size, 4096, _vp(bai), bai.size, C.byref(n)))
    return bai[:int(n.value)]


t_idx, p_idx, bai = timed(index_once)
print(f"{b.n} reads (c3), {len(raw)} bytes of records, {e.n_sorted} output records")
print(f"emit_sorted_bgzf {t_emit * 1e3:.1f} ms = {b.n / t_emit / 1e6:.1f} Mreads/s, {bz.size} bytes in {-(-len(raw) // 65280)} members")
print(kernels(p_emit))
print(f"index_sorted_bgzf {t_idx * 1e3:.1f} ms = {b.n / t_idx / 1e6:.1f} Mreads/s, {t_idx / t_emit * 100:.1f} % of the emit call")
print(kernels(p_idx, 24))
size_pass = p_emit.get("emit_bam_sizes", (0, 0.0))[1]
print(f"per record: the index call's kernels {sum(v[1] for v in p_idx.values()) * 1e6 / max(e.n_sorted, 1):.2f} ns, the emit call's size pass "
      f"{size_pass * 1e6 / max(e.n_sorted, 1):.2f} ns")

# the index's shape
buf = bai.tobytes()
n_ref, at, n_bins, n_chunks, n_intv_all = struct.unpack_from("<i", buf, 4)[0], 8, 0, 0, 0
for _ in range(n_ref):
    n_bin, at = struct.unpack_from("<i", buf, at)[0], at + 4
    for _ in range(n_bin):
        number, n_chunk = struct.unpack_from("<Ii", buf, at)
        at += 8 + 16 * n_chunk
        if number != 37450:
            n_bins, n_chunks = n_bins + 1, n_chunks + n_chunk
    n_intv = struct.unpack_from("<i", buf, at)[0]
    at += 4 + 8 * n_intv
    n_intv_all += n_intv
print(f"index: {len(buf)} bytes, {n_ref} contigs, {n_bins} bins, {n_chunks} chunks, {n_intv_all} windows, n_no_coor {struct.unpack_from('<Q', buf, at)[0]}")
if len(sys.argv) > 2 and sys.argv[2] == "check":
    from tests import bairef
    print("check against tests/bairef.py:", "identical" if bairef.build(bz.tobytes(), 4096, h.n_ref) == buf else "DIFFERENT")
e.close()
