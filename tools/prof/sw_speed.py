"""elp_sw_align at the realignment site's shape (filters/realign.go:310): N problems, 64 haplotypes of 300..600 bases as the reference
pool, 150-base alternates cut from them - 40 % exact copies (the shortcut's share), 35 % with 1-3 substitutions, 25 % with one indel of
1-8 bases (and 0-2 substitutions) -, parameters 10, -15, -30, -5, softclip.  Prints problems/s and cell updates/s of the whole call
(median and spread of the timed runs, after a warm-up) and of the kernels alone (elp_profile_*, runs of their own), the share of problems
the shortcut took, the backtrack bytes written, the same for three scratch budgets (alternating), and next to it tests/swref_c.c on 16
threads over the same problems - the only thing measured on the CPU.  Every device result is compared with that baseline's.
usage: sw_speed.py [problems] [timed runs]"""
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from elprep_amd.engine import Engine, _vp  # noqa: E402
from tests import sw_cases, swref  # noqa: E402
from tools import synth  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 200_000
runs = int(sys.argv[2]) if len(sys.argv) > 2 else 7
rng = np.random.default_rng(2026)
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
haps = [rng.choice(ACGT, int(rng.integers(300, 601))) for _ in range(64)]
ref_of = rng.integers(0, 64, n).astype(np.uint32)
kind = rng.random(n)
alts = np.empty((n, 150), dtype=np.uint8)
for k in range(n):
    hap = haps[ref_of[k]]
    at = int(rng.integers(0, hap.size - 160))
    s = hap[at:at + 160].copy()
    if kind[k] >= 0.40:
        indel = kind[k] >= 0.75
        for _ in range(int(rng.integers(0, 3)) if indel else int(rng.integers(1, 4))):
            p = int(rng.integers(0, 150))
            s[p] = ACGT[(int(np.searchsorted(ACGT, s[p])) + 1 + int(rng.integers(0, 3))) % 4]  # (another base)
        if indel:
            p, g = int(rng.integers(10, 140)), int(rng.integers(1, 9))
            s = np.concatenate([s[:p], s[p + g:], rng.choice(ACGT, g)]) if rng.random() < 0.5 else np.concatenate([s[:p], rng.choice(ACGT, g), s[p:]])
    alts[k] = s[:150]
a = np.concatenate(haps)
a_off = np.concatenate([[0], np.cumsum([h.size for h in haps])]).astype(np.uint64)
b = alts.reshape(-1)
b_off = (np.arange(n + 1, dtype=np.uint64) * 150)
alt_of = np.arange(n, dtype=np.uint32)
m_of = (a_off[1:] - a_off[:-1])[ref_of].astype(np.int64)
params, strategy = swref.P1, swref.SOFTCLIP
case = sw_cases.Case("realign", [h.tobytes() for h in haps], [alts[k].tobytes() for k in range(n)], ref_of, alt_of, params, strategy)

# the baseline, and the expected values
sw_cases.expected(sw_cases.Case("warm", case.refs[:1], case.alts[:1], [0], [0], params, strategy))
t_cpu = []
for _ in range(2):
    t0 = time.perf_counter()
    want = sw_cases.expected(case, threads=16)
    t_cpu.append(time.perf_counter() - t0)
hit = np.array([swref.last_index(case.refs[ref_of[k]], case.alts[k]) >= 0 for k in range(0, n, max(n // 2000, 1))])  # (a sample, in Python)

h = synth.config("tiny").header()
e = Engine(h, 0)
cap = int((m_of + 150 + 2).sum())
cig, coff, off, need = np.zeros(cap, np.uint32), np.zeros(n + 1, np.uint64), np.zeros(n, np.int32), C.c_uint64()


def call():
    e._check(e.L.elp_sw_align(e.h, 64, _vp(a), _vp(a_off), n, _vp(b), _vp(b_off), n, _vp(ref_of), _vp(alt_of), *params, strategy, _vp(cig), cap, _vp(coff), _vp(off),
                              C.byref(need)))


def wall(k):
    ts = []
    for _ in range(k):
        e.sync()
        t0 = time.perf_counter()
        call()
        ts.append(time.perf_counter() - t0)
    return ts


def show(label, ts, cells):
    med = statistics.median(ts)
    print(f"{label}: median {med * 1e3:.2f} ms (min {min(ts) * 1e3:.2f}, max {max(ts) * 1e3:.2f}, {len(ts)} runs) = {n / med / 1e6:.2f} M problems/s, "
          f"{cells / med / 1e9:.1f} G cell updates/s")


call()  # warm-up: allocations, code objects
same = np.array_equal(coff, want[0]) and np.array_equal(cig[:int(need.value)], want[1]) and np.array_equal(off, want[2])
e.profile_enable(True)
e.profile_reset()
call()
prof = e.profile()
e.profile_enable(False)
n_dp_launch = prof.get("sw_dp", (0, 0.0))[0]
# what ran through the DP: the problems whose CIGAR is not one M of 150 at an offset the shortcut would give are a subset; count exactly
# from the expected values - a hit is "150M" AND the alternate stands there
is_hit = np.zeros(n, dtype=bool)
one_m = (want[0][1:] - want[0][:-1] == 1) & (want[1][want[0][:-1].astype(np.int64)] == ((150 << 4) | 0))
for k in np.flatnonzero(one_m):
    o = int(want[2][k])
    is_hit[k] = o >= 0 and o + 150 <= m_of[k] and bytes(haps[ref_of[k]][o:o + 150]) == case.alts[k]
n_dp = int((~is_hit).sum())
cells_dp = int((m_of[~is_hit] * 150).sum())
cells_all = int((m_of * 150).sum())
lanes = (150 + 3) // 4
bt_bytes = int(((m_of[~is_hit] + lanes - 1) * lanes * 4 * 2).sum())  # sw_core.hpp: sw_bt_cells of one partial tile, int16

print(f"{n} problems, 64 haplotypes of 300..600 bases, 150-base alternates: 40 % exact copies, 35 % 1-3 substitutions, 25 % one indel of 1-8 (+ 0-2 substitutions)")
print(f"results equal to swref_c's: {same}; operations {int(need.value)}; shortcut hits {int(is_hit.sum())} = {is_hit.mean() * 100:.1f} % "
      f"(sampled in Python: {hit.mean() * 100:.1f} %); through the DP {n_dp} problems, {cells_dp / 1e9:.2f} G cells; backtrack written {bt_bytes / 1e9:.2f} GB "
      f"in {n_dp_launch} chunks (default budget)")
show("whole call, default budget (all cells of the DP problems)", wall(runs), cells_dp)
kern = sum(v[1] for v in prof.values()) / 1e3
print(f"kernels alone (one profiled run): {kern * 1e3:.2f} ms = {n / kern / 1e6:.2f} M problems/s, {cells_dp / kern / 1e9:.1f} G cell updates/s; "
      f"sw_dp {prof.get('sw_dp', (0, 0))[1]:.2f} ms = {cells_dp / max(prof.get('sw_dp', (0, 1e-9))[1], 1e-9) / 1e6:.1f} G cell updates/s, "
      f"{bt_bytes / max(prof.get('sw_dp', (0, 1e-9))[1], 1e-9) / 1e9:.2f} TB/s of backtrack stores")
for k, v in sorted(prof.items(), key=lambda kv: -kv[1][1]):
    if v[0]:
        print(f"  {k:16s} {int(v[0]):4d} launches {v[1]:9.3f} ms")
# scratch budgets, alternating
budgets = (256 << 20, 1 << 30, 4 << 30)
ts = {bud: [] for bud in budgets}
for _ in range(max(runs // 2, 2)):
    for bud in budgets:
        e.set_tuning("sw_scratch_bytes", bud)
        ts[bud] += wall(1)
e.set_tuning("sw_scratch_bytes", 0)
for bud in budgets:
    show(f"whole call, sw_scratch_bytes = {bud >> 20} MiB", ts[bud], cells_dp)
cpu = min(t_cpu)
print(f"swref_c on 16 threads: {cpu * 1e3:.0f} ms (best of {len(t_cpu)}) = {n / cpu / 1e6:.3f} M problems/s, {cells_dp / cpu / 1e9:.2f} G cell updates/s "
      f"(it allocates and fills two int32 matrices per problem, as the reference does)")
print(f"all cells, shortcut problems included: {cells_all / 1e9:.2f} G")
e.close()
