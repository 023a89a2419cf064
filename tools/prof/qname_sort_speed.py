"""Speed of elp_sort_queryname on the bench workload's read set (synth.config("c3"), 50.2 M reads by default): usage qname_sort_speed.py [reads] (reads / 2 pairs: 50 M -> the 50.2 M records of bench.py)

Stages the reads once, runs the queryname sort once to warm up, then times 5 calls (each ending in e.sync()) and the coordinate sort on
the same context for comparison; then the same on a copy whose records are shuffled (every generated chunk in a random order, the chunks
in a random order: mates are no longer neighbours).  Every permutation timed is checked: a permutation of the records, adjacent names in
order, equal names in staging order."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from elprep_amd.engine import Engine  # noqa: E402
from tools import synth  # noqa: E402

CHUNK = 2_000_000  # pairs per generated batch


def _name_rows(b, width):
    """fixed-width rows: the record state (0 output, 1 not), then the zero-padded QNAME"""
    rows = np.zeros((b.n, width + 1), np.uint8)
    rows[:, 0] = b.has_sr != 0
    ln = np.diff(b.qname_off).astype(np.int64)
    assert b.n == 0 or ln.max() <= width, "name longer than the check's rows"
    starts = b.qname_off[:-1].astype(np.int64)
    for j in range(width):
        has = ln > j
        rows[has, j + 1] = b.qname[starts[has] + j]
    return rows


def _check(perm, rows):
    n = rows.shape[0]
    assert perm.shape == (n,) and np.array_equal(np.bincount(perm, minlength=n), np.ones(n, np.int64)), "not a permutation"
    for lo in range(0, n - 1, 1 << 20):
        hi = min(lo + (1 << 20), n - 1)
        ia, ib = perm[lo:hi], perm[lo + 1:hi + 1]
        a, b = rows[ia], rows[ib]
        diff = a != b
        anyd = diff.any(1)
        first = diff.argmax(1)
        r = np.arange(hi - lo)
        ok = np.where(anyd, a[r, first] < b[r, first], ia < ib)
        assert ok.all(), ("out of order at", lo + int(np.argmin(ok)))


def _run(label, batches, width):
    h = synth.config("c3").header()
    e = Engine(h)
    rows = []
    for b in batches:
        e.stage(b)
        rows.append(_name_rows(b, width))
    rows = np.concatenate(rows)
    n = e.n
    e.snapshot()
    e.sort_queryname(fetch=False)
    e.sync()
    ts = []
    for _ in range(5):
        t0 = time.perf_counter()
        e.sort_queryname(fetch=False)
        e.sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    _check(e.permutation(), rows)
    e.mark_duplicates(True, fetch=False)  # (adapt happens here, outside the timed coordinate sorts)
    e.sync()
    e.sort_coordinate(fetch=False)
    e.sync()
    tc = []
    for _ in range(5):
        t0 = time.perf_counter()
        e.sort_coordinate(fetch=False)
        e.sync()
        tc.append((time.perf_counter() - t0) * 1e3)
    e.close()
    best, med = min(ts), float(np.median(ts))
    print("%-9s %d reads  sort_queryname best %.3f ms  median %.3f ms  %.0f Mreads/s   (sort_coordinate best %.3f ms  median %.3f ms)"
          % (label, n, best, med, n / best / 1e3, min(tc), float(np.median(tc))), flush=True)


def main():
    reads = int(sys.argv[1]) if len(sys.argv) > 1 else 50_000_000
    cfg = synth.config("c3")
    pairs = reads // 2
    jobs = [(lo, min(lo + CHUNK, pairs)) for lo in range(0, pairs, CHUNK)]
    width = 64  # (the synthetic names are ~30 bytes: _name_rows checks)
    _run("as staged", (synth.generate(cfg, lo, hi) for lo, hi in jobs), width)
    rng = np.random.default_rng(1)
    order = rng.permutation(len(jobs))

    def shuffled():
        for k in order:
            b = synth.generate(cfg, *jobs[k])
            yield b.take(rng.permutation(b.n))
    _run("shuffled", shuffled(), width)


if __name__ == "__main__":
    main()
