"""elp_order_keep on N reads of the c3 read set (bench.py's): kernel time from profile() (HIP events) and wall time per call, for
by_split = 0 and for by_split = 1 with the records in 1, 17 and 300 split files, next to elp_sort_coordinate on the same records in the
same run - the only call there was in front of an emit.  usage: keep_order_speed.py [reads]   (default 16 M)
One untimed call of each form, then three timed ones (best and median); every permutation timed is checked against numpy's.  3 % of the
records are sr-tagged copies, so that the partition has two classes.  "6 B/record" = the state byte twice + the permutation once, what
the two-pass partition of by_split = 0 moves; the other rows are shown against the same figure."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from elprep_amd import sfm  # noqa: E402
from elprep_amd.engine import Engine  # noqa: E402
from tools import synth  # noqa: E402

TIMED = 3


def _timed(e, call):
    """-> (kernel ms of every timed call, wall ms of every timed call); one untimed call first"""
    call()
    e.sync()
    ks, ws = [], []
    for _ in range(TIMED):
        e.profile_enable(True)
        e.profile_reset()
        t0 = time.perf_counter()
        call()
        e.sync()
        ws.append((time.perf_counter() - t0) * 1e3)
        p = e.profile()
        e.profile_enable(False)
        ks.append(sum(ms for _, ms in p.values()))
    return ks, ws, p


def _row(label, n, ks, ws, p):
    k = min(ks)
    kernels = ", ".join("%s %.3f" % (name, ms) for name, (_, ms) in sorted(p.items()) if ms > 0)
    print("%-28s kernels best %.3f ms  median %.3f ms;  6 B/record = %.1f MB in that time = %.3f TB/s;  wall best %.3f ms   [%s]"
          % (label, k, float(np.median(ks)), 6 * n / 1e6, 6 * n / (k * 1e-3) / 1e12, min(ws), kernels), flush=True)


def main():
    reads = int(sys.argv[1]) if len(sys.argv) > 1 else 16_000_000
    cfg = synth.config("c3")
    h = cfg.header()
    b = synth.generate(cfg, 0, reads // 2)
    n = b.n
    sr = np.arange(n) % 33 == 7
    print("%d reads, %d of them sr-tagged copies" % (n, int(sr.sum())), flush=True)
    e = Engine(h, 0)
    for k in (None, 1, 17, 300):
        split = np.zeros(n, np.uint16) if k is None else (np.arange(n, dtype=np.int64) * k // n).astype(np.uint16)[::-1].copy()  # (files staged last id first)
        bb = sfm.with_sr(b, sr, split)
        e.reset()
        e.stage(bb)
        e.sync()
        by = k is not None
        ks, ws, p = _timed(e, lambda: e.order_keep(by, fetch=False))
        key = (bb.has_sr != 0).astype(np.int64) * 65536 + (split if by else 0)
        assert np.array_equal(e.permutation(), np.argsort(key, kind="stable").astype(np.uint32)), "wrong permutation"
        _row("order_keep(0)" if not by else "order_keep(1), %d split%s" % (k, "" if k == 1 else "s"), n, ks, ws, p)
    # the coordinate sort of the same records (keys made by mark duplicates, outside the timed calls)
    e.mark_duplicates(True, fetch=False)
    e.sync()
    ks, ws, p = _timed(e, lambda: e.sort_coordinate(fetch=False))
    _row("sort_coordinate", n, ks, ws, p)
    e.close()


if __name__ == "__main__":
    main()
