"""The optional-field options on N reads, best of 5, every call ending in a sync.  usage: tag_filter_speed.py [reads]
With ELP_HIP_SO naming a build without the new entry points only the unfiltered emitters are timed (the A/B against that build)."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from elprep_amd.batch import Header  # noqa: E402
from elprep_amd.engine import Engine  # noqa: E402
from tools import synth  # noqa: E402

reads = int(sys.argv[1]) if len(sys.argv) > 1 else 4_000_000
cfg = synth.config("c3")
h = cfg.header()
b = synth.generate(cfg, 0, reads // 2)
raw0, off0 = synth.bam_records(b, h.rg_ids)
SUFFIX = np.frombuffer(b"X0C\x01X1C\x00XMC\x00XOC\x00XGC\x00", np.uint8)  # every record exact by the strict filter


def with_suffix(raw, off):
    """every record with SUFFIX behind its fields and block_size raised, in chunks of 64 K records"""
    n, k = off.size - 1, SUFFIX.size
    new_off = off + np.arange(n + 1, dtype=np.uint64) * k
    out = np.empty(int(new_off[-1]), np.uint8)
    for a in range(0, n, 65536):
        z = min(a + 65536, n)
        lens = (off[a + 1:z + 1] - off[a:z]).astype(np.int64)
        src = raw[int(off[a]):int(off[z])]
        ids = np.repeat(np.arange(z - a, dtype=np.int64), lens)
        base = int(new_off[a])
        out[base + np.arange(src.size, dtype=np.int64) + k * ids] = src
        ends = (new_off[a + 1:z + 1]).astype(np.int64) - k
        out[ends[:, None] + np.arange(k)] = SUFFIX
        bs = (lens - 4 + k).astype(np.uint32)
        at = new_off[a:z].astype(np.int64)
        for byte in range(4):
            out[at + byte] = (bs >> (8 * byte)) & 255
    return out, new_off


raw, off = with_suffix(raw0, off0)
from elprep_amd import _lib  # noqa: E402
old_build = bool(os.environ.get("ELP_HIP_SO")) and not hasattr(_lib.hip(), "elp_set_tag_filter")


def best(fn, reps=5):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        e.sync()
        ts.append(time.perf_counter() - t0)
    return min(ts) * 1e3, r


e = Engine(h, 0)
e.set_read_group_ids(h.rg_ids)


def stage():
    e.reset()
    e.set_read_group_ids(h.rg_ids)
    e.stage_bam(raw, rec_off=off)


stage()
t_stage, _ = best(stage)
print(f"{b.n} reads, {raw.size} bytes of records ({os.environ.get('ELP_HIP_SO') or 'this build'})")
print(f"stage_bam, RG looked up: {t_stage:.1f} ms")
e.mark_duplicates(True, fetch=False)
e.sort_coordinate(fetch=False)
out = np.empty(int(raw.size * 1.02) + (1 << 20), np.uint8)
e.emit_sorted_bam(out)
t, r = best(lambda: e.emit_sorted_bam(out))
print(f"emit_sorted_bam  no filter: {t:.1f} ms, {r.size} bytes")


def kernels(label):
    """the emitter's two kernels alone (HIP events): the call's time is mostly the copy of the records to the host"""
    ks = []
    for _ in range(5):
        e.profile_enable(True)
        e.profile_reset()
        e.emit_sorted_bam(out)
        e.sync()
        p = e.profile()
        e.profile_enable(False)
        ks.append((p["emit_bam_sizes"][1], p["emit_bam"][1]))
    print(f"  kernels {label}: emit_bam_sizes {min(k[0] for k in ks):.3f} ms, emit_bam {min(k[1] for k in ks):.3f} ms")


kernels("no filter")
e.emit_sorted_bgzf()
t, r = best(e.emit_sorted_bgzf)
print(f"emit_sorted_bgzf no filter: {t:.1f} ms, {r.size} bytes")
if not old_build:
    e.set_tag_filter(keep="none")
    t, r = best(lambda: e.emit_sorted_bam(out))
    print(f"emit_sorted_bam  keep none: {t:.1f} ms, {r.size} bytes")
    kernels("keep none")
    t, r = best(e.emit_sorted_bgzf)
    print(f"emit_sorted_bgzf keep none: {t:.1f} ms, {r.size} bytes")
    e.set_tag_filter()
    # the predicates: a pass over the staged records' bytes against a pass over the CIGAR column (nothing is rejected: repeatable)
    def fresh(fn):  # the filter alone, each time on freshly staged records (a filter skips what an earlier one rejected)
        ts = []
        for _ in range(5):
            stage()
            e.sync()
            t0 = time.perf_counter()
            r = fn()
            e.sync()
            ts.append(time.perf_counter() - t0)
        return min(ts) * 1e3, r

    t_s, n_s = fresh(e.filter_exact_strict)
    t_f, n_f = fresh(lambda: e.filter_records(remove_non_exact=True))
    print(f"filter_exact_strict: {t_s:.2f} ms ({n_s} rejected) = {b.n / t_s / 1e3:.0f} Mreads/s, {raw.size / t_s / 1e6:.0f} GB/s of staged records")
    print(f"filter_records remove_non_exact: {t_f:.2f} ms ({n_f} rejected); ratio strict / non-exact = {t_s / t_f:.1f}")
    e.close()
    # replace-read-group: staging without the id comparison
    h1 = Header.from_read_groups(h.ref_names, h.ref_len, [{"ID": "new", "LB": "lib1", "PU": "FC1.1"}])
    e = Engine(h1, 0)

    def stage_replace():
        e.reset()
        e.set_replace_read_group("new")
        e.stage_bam(raw, rec_off=off)

    stage_replace()
    t, _ = best(stage_replace)
    print(f"stage_bam, replace-read-group: {t:.1f} ms (RG looked up: {t_stage:.1f} ms)")
e.close()
