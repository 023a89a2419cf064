"""elp_emit_split_bam / _bgzf / _sam on N reads of the c3 read set (bench.py's) in 17 contig groups: kernel time from profile() (HIP events)
- the list build (split_list_*, radix_*) apart from the formats' kernels - and wall time per call, next to elp_order_keep +
elp_emit_sorted_bam / _sam on the same records in the same run.  usage: split_out_speed.py [reads]   (default 16 M)
The records are staged from BAM bytes (the oracle's encoder); one untimed call of each form, then three timed ones (best and median) into
one page-locked buffer, no size query inside the timed calls.  The expectation the rows are read against: the split emitters write
(n + n_spread) / n times the keep emitter's bytes, so their emit kernels should cost about that ratio of its time, plus the list build.
With ELP_HIP_SO naming another build of the library (the parent commit's, which has no split emitters) only the keep emitters' rows are
printed: two such runs and one of this build on one box are the A/B of the emitters every context runs."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import oracle as orc  # noqa: E402
from elprep_amd import _lib, sfm  # noqa: E402
from elprep_amd.engine import Engine  # noqa: E402
from tools import synth  # noqa: E402

TIMED = 3
N_GROUPS = 17
LIST_KERNELS = ("split_list", "radix_")


def _timed(e, call):
    """-> (per timed call: {kernel: ms}), wall ms of every timed call, bytes written; one untimed call first"""
    call()
    e.sync()
    ps, ws, nbytes = [], [], 0
    for _ in range(TIMED):
        e.profile_enable(True)
        e.profile_reset()
        t0 = time.perf_counter()
        nbytes = call()
        e.sync()
        ws.append((time.perf_counter() - t0) * 1e3)
        ps.append({name: ms for name, (_, ms) in e.profile().items()})
        e.profile_enable(False)
    return ps, ws, nbytes


def _row(label, ps, ws, nbytes):
    is_list = lambda name: name.startswith(LIST_KERNELS)
    lists = [sum(ms for k, ms in p.items() if is_list(k)) for p in ps]
    emits = [sum(ms for k, ms in p.items() if not is_list(k)) for p in ps]
    best = ps[int(np.argmin(emits))]
    kernels = ", ".join("%s %.3f" % (k, ms) for k, ms in sorted(best.items()) if ms > 0)
    print("%-34s %8.1f MB   emit kernels best %.3f ms  median %.3f ms;  list build best %.3f ms;  wall best %.1f ms   [%s]"
          % (label, nbytes / 1e6, min(emits), float(np.median(emits)), min(lists), min(ws), kernels), flush=True)


def main():
    reads = int(sys.argv[1]) if len(sys.argv) > 1 else 16_000_000
    cfg = synth.config("c3")
    h = cfg.header()
    b = synth.generate(cfg, 0, reads // 2)
    n = b.n
    gof = (1 + np.arange(h.n_ref, dtype=np.int64) * N_GROUPS // h.n_ref).astype(np.int32)
    assert int(gof.max()) == N_GROUPS
    g, sp = sfm.split_records(b, gof)
    have_split = hasattr(_lib.hip(), "elp_emit_split_bam")
    print("library %s: %d reads, %d of them spread; (n + n_spread) / n = %.4f" % (os.path.relpath(_lib.HIP_SO, ROOT), n, int(sp.sum()), (n + int(sp.sum())) / n), flush=True)
    e = Engine(h, 0)
    e.set_read_group_ids(h.rg_ids)
    piece = 2_000_000
    for lo in range(0, n, piece):                     # (the encoder's output of a piece at a time: the host holds one piece of BAM bytes)
        e.stage_bam(orc.bam_encode(b, h.rg_ids, order=np.arange(lo, min(lo + piece, n), dtype=np.uint32)))
    e.set_reference_names()
    e.sync()
    nb = C.c_uint64()
    # one buffer for every call: the SAM form of the split files is the largest output
    sizes = []
    e.order_keep(fetch=False)
    for fn in (e.L.elp_emit_sorted_bam, e.L.elp_emit_sorted_sam):
        e._check(fn(e.h, C.c_void_p(0), 0, C.byref(nb)))
        sizes.append(int(nb.value))
    off = np.zeros(N_GROUPS + 3, np.uint64)
    if have_split:
        e._check(e.L.elp_emit_split_sam(e.h, C.c_void_p(gof.ctypes.data), N_GROUPS, 0, C.c_void_p(0), 0, C.c_void_p(off.ctypes.data), C.byref(nb)))
        sizes.append(int(nb.value))
        e._check(e.L.elp_emit_split_bgzf(e.h, C.c_void_p(gof.ctypes.data), N_GROUPS, 0, C.c_void_p(0), 0, C.c_void_p(off.ctypes.data), C.byref(nb)))
        sizes.append(int(nb.value))
    out = e.pinned_zeros((max(sizes) + 64,), np.uint8)
    po = C.c_void_p(out.ctypes.data)

    def keep(fn):
        def call():
            e.order_keep(fetch=False)
            e._check(fn(e.h, po, out.size, C.byref(nb)))
            return int(nb.value)
        return call

    def split(fn):
        def call():
            e._check(fn(e.h, C.c_void_p(gof.ctypes.data), N_GROUPS, 0, po, out.size, C.c_void_p(off.ctypes.data), C.byref(nb)))
            return int(nb.value)
        return call

    _row("order_keep + emit_sorted_bam", *_timed(e, keep(e.L.elp_emit_sorted_bam)))
    _row("order_keep + emit_sorted_sam", *_timed(e, keep(e.L.elp_emit_sorted_sam)))
    if have_split:
        _row("emit_split_bam, 17 groups", *_timed(e, split(e.L.elp_emit_split_bam)))
        _row("emit_split_sam, 17 groups", *_timed(e, split(e.L.elp_emit_split_sam)))
        _row("emit_split_bgzf, 17 groups", *_timed(e, split(e.L.elp_emit_split_bgzf)))
    e.pinned_release(out)
    e.close()


if __name__ == "__main__":
    main()
