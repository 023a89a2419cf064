"""A/B of the duplication-metrics pass across builds of libelprep_hip.so: usage metrics_ab.py <reads> <runs> <lib.so>...
One process per library and run, the libraries alternating.  Every process prints, for <reads> reads of the bench workload, the `mx_*`
launches of one elp_dup_metrics_hist call (Engine.profile(): names and counts), their summed event time, and the wall time of one call
(best of five, each ending in a sync); the first process of a library also prints the launches of the five read sets of
tests/test_gpu_metrics_phases.py and whether counters and histograms equal the oracle's."""
import json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if os.environ.get("ELP_AB_LIB"):
    sys.path.insert(0, ROOT)
    from elprep_amd import _lib
    _lib.HIP_SO = os.environ["ELP_AB_LIB"]
    import numpy as np
    from elprep_amd.engine import Engine
    from tools import synth
    tag = os.environ["ELP_AB_TAG"]

    def profiled(e, hist_len):
        e.profile_enable(True); e.profile_reset()
        out = e.dup_metrics(100, hist_len=hist_len); e.sync()
        prof = {k: v for k, v in e.profile().items() if v[0] and "mx_" in k}
        e.profile_enable(False)
        return out, prof

    if os.environ.get("ELP_AB_CASES"):
        import oracle as orc
        from elprep_amd import sfm
        from tests import optical_names as on, test_gpu_metrics_phases as ph
        h = on.header(2)
        e = Engine(h)
        for name, make, _, _ in ph.CASES:
            b = on.batch(*make()) if make else sfm.empty_batch()
            _, octr, ohist = orc.dup_metrics(b, h, None, ph.DIST, hist_len=8)
            e.reset()
            if b.n:
                e.stage(b)
            e.mark_duplicates(True)
            (ctr, hist), prof = profiled(e, 8)
            ok = bool(np.array_equal(ctr, octr) and np.array_equal(hist, ohist))
            print("%s | %s | oracle_equal=%s | %s" % (tag, name, ok, json.dumps({k: v[0] for k, v in sorted(prof.items())})), flush=True)
        e.close()
    reads = int(sys.argv[1])
    cfg = synth.config("c3"); h = cfg.header()
    e = Engine(h)
    for lo in range(0, reads // 2, 2_000_000):
        e.stage(synth.generate(cfg, lo, min(lo + 2_000_000, reads // 2)))
    e.mark_duplicates(True, fetch=False); e.sync()
    e.dup_metrics(100, hist_len=8); e.sync()  # (scratch, side lane)
    (ctr, hist), prof = profiled(e, 8)
    best = 1e9
    for it in range(5):
        t0 = time.perf_counter(); e.dup_metrics(100, hist_len=8); e.sync(); best = min(best, (time.perf_counter() - t0) * 1e3)
    print("%s | %d reads | %s" % (tag, reads, json.dumps({k: v[0] for k, v in sorted(prof.items())})), flush=True)
    print("%s | %d reads | mx_ launches %d, summed %.3f ms | one call %.3f ms | counters %d histograms %d" % (
        tag, reads, sum(v[0] for v in prof.values()), sum(v[1] for v in prof.values()), best, int(ctr.sum()), int(hist.sum())), flush=True)
    e.close()
else:
    reads, runs, libs = sys.argv[1], int(sys.argv[2]), sys.argv[3:]
    for r in range(runs):
        for lib in libs:
            env = dict(os.environ, ELP_AB_LIB=os.path.abspath(lib), ELP_AB_TAG=os.path.basename(lib))
            if r == 0:
                env["ELP_AB_CASES"] = "1"
            if subprocess.call([sys.executable, os.path.abspath(__file__), reads], env=env, timeout=600) != 0:
                sys.exit(1)  # (nothing more on a device that a run left in doubt)
