"""CPU tests of the BQSR gather's launch plan (elprep_amd/csrc/bqsr_plan.hpp, built by the host compiler through tests/plan_host.cpp): which
count kernel takes a read set, in which form and in how many passes, and the layout of the gather's scratch block.  A wrong plan is silent
on the device - the tables stay bit-exact, the step merely takes another kernel or more passes - so the expected plans below are worked out
by hand in the docstrings, not computed from the code.

The numbers every case uses.  LDS of a CU: 160 KiB = 163840 bytes.  Static LDS of the kernels (the constants beside their __shared__
declarations; FlatLds<256> is 1040 bytes, FlatLds<512> 2064):
  k_bqsr_count3            1024 + 1024 + 96 + 256 + (2 * 256 + 8) * 4                                           =  4480
  k_bqsr_count, 512 thr.   1040 + 256 * (32 + 4) + 1024 + 96 + 64 + 8 + 64 * 4 + 256 * 16 + 256 * 12            = 18872
  k_bqsr_count, 1024 thr.  2064 + 512 * (32 + 4) + 1024 + 96 + 64 + 8 + 64 * 4 + 256 * 16 + 512 * 12            = 32184
One-length kernel at 150 bases: ncw = (34 * 150 >> 4) + 2 = 320 cycle words; a row has rsw = (16 << rlog) + 16 + 320 rounded up to 32 words:
864 (rlog 5), 608 (4), 480 (3), 416 (2), 384 (1).  n_cov * (nq + 3) rows fit if (rows * rsw + 64) * 4 + 4480 <= 163840: rows * rsw <= 39776.
General kernel at 150 bases: a row has rs = 32 + 318 + 2 = 352 words (1408 bytes), with observation-only cycle cells (MG) 32 + 159 + 2 = 193,
even: 192 words (768 bytes).  512 threads: budget 163840 / w - 18872 - 256 = 35485 (w = 3) or 62792 (w = 2) bytes for n_cov * (slots + 3)
rows.  1024 threads: (163840 - 32184 - 256) = 131400 bytes: 93 rows of 1408 bytes, 171 rows of 768."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tests", "libplan_host.so")

LDS_CU = 160 * 1024
L3, L512, L1024 = 4480, 18872, 32184
LMAXS = (1, 16, 17, 100, 150, 151, 250, 1022, 1023)
GENERAL = ("fits", "wg_per_cu", "big", "mg", "rs", "ncp", "qcap", "passes", "dyn")


@pytest.fixture(scope="module")
def lib():
    src = os.path.join(ROOT, "tests", "plan_host.cpp")
    hdr = os.path.join(ROOT, "elprep_amd", "csrc", "bqsr_plan.hpp")
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", SO, src])
    return C.CDLL(SO)


def _lds():
    return (C.c_uint64 * 3)(L3, L512, L1024)


def _mode(L, n_cov, nq, lmax=150, max_cycle=500, uniform_len=None, count_kernel=0, count3_rlog=-1):
    return L.plan_c3_mode(n_cov, nq, lmax, max_cycle, lmax if uniform_len is None else uniform_len, count_kernel, count3_rlog, _lds())


def _count3(L, n_cov, nq, lmax=150, force_rlog=-1):
    out = (C.c_uint64 * 3)()
    rc = L.plan_count3(n_cov, nq, lmax, C.c_uint64(L3), force_rlog, out)
    return None if rc else dict(rsw=out[0], rlog=out[1], dyn=out[2])


def _general(L, n_cov, nq, lmax=150):
    out = (C.c_int64 * 9)()
    L.plan_general(n_cov, nq, lmax, _lds(), out)
    return dict(zip(GENERAL, out))


# ---- the one-length kernel's mode

def test_mode_1_one_read_group(lib):
    """1 read group, 6 qualities, 150 bases: 1 * (6 + 3) = 9 rows; rlog 5: 9 * 864 = 7776 <= 39776 fits.  Everything fits with replication 32
    -> mode 1; dyn = (7776 + 64) * 4 = 31360."""
    assert _mode(lib, 1, 6) == 1
    assert _count3(lib, 1, 6) == dict(rsw=864, rlog=5, dyn=31360)


def test_mode_1_four_read_groups(lib):
    """4 read groups, 6 qualities: 36 rows; 36 * 864 = 31104 <= 39776: rlog 5 -> mode 1; dyn = (31104 + 64) * 4 = 124672."""
    assert _mode(lib, 4, 6) == 1
    assert _count3(lib, 4, 6) == dict(rsw=864, rlog=5, dyn=124672)


def test_mode_2_replication_below_8(lib):
    """4 read groups, 20 qualities: 92 rows; 92 * 864 = 79488, 92 * 608 = 55936, 92 * 480 = 44160 do not fit, 92 * 416 = 38272 does: rlog 2,
    replication 4 < 8.  One covariate's 23 rows: 23 * 864 = 19872 fits -> mode 2, its table at rlog 5 with dyn = (19872 + 64) * 4 = 79744.
    "count_kernel" = 2 (never split) keeps the one table: mode 1."""
    assert _count3(lib, 4, 20) == dict(rsw=416, rlog=2, dyn=(38272 + 64) * 4)
    assert _mode(lib, 4, 20) == 2
    assert _count3(lib, 1, 20) == dict(rsw=864, rlog=5, dyn=79744)
    assert _mode(lib, 4, 20, count_kernel=2) == 1


def test_mode_2_one_table_does_not_fit(lib):
    """16 read groups, 6 qualities: 144 rows; even at rlog 1 144 * 384 = 55296 > 39776: no table of all covariates.  One covariate's 9 rows
    fit -> mode 2.  "count_kernel" = 2 (never split) leaves only the general kernel: mode 0."""
    assert _count3(lib, 16, 6) is None
    assert _mode(lib, 16, 6) == 2
    assert _mode(lib, 16, 6, count_kernel=2) == 0


def test_mode_0(lib):
    """the general kernel takes the count when a read can exceed --max-cycle (150 > 100), when a read has more than 1022 bases (1023, under
    --max-cycle 2000), when the lengths are ragged (uniform_len 0), and when "count_kernel" = 1 says so; the same read set otherwise: mode 1"""
    assert _mode(lib, 1, 6, lmax=150, max_cycle=150) == 1
    assert _mode(lib, 1, 6, lmax=150, max_cycle=100) == 0
    assert _mode(lib, 1, 6, lmax=1022, max_cycle=2000) == 1
    assert _mode(lib, 1, 6, lmax=1023, max_cycle=2000) == 0
    assert _mode(lib, 1, 6, uniform_len=0) == 0
    assert _mode(lib, 1, 6, count_kernel=1) == 0


def test_count_kernel_2_and_3(lib):
    """"count_kernel" = 3 (always split): 4 read groups, 6 qualities would be mode 1 (see above) and become mode 2; with ONE read group there is
    nothing to split: mode 1.  "count_kernel" = 2: see the two mode-2 cases."""
    assert _mode(lib, 4, 6, count_kernel=3) == 2
    assert _mode(lib, 1, 6, count_kernel=3) == 1
    assert _mode(lib, 4, 6, count_kernel=2) == 1


def test_count3_rlog_forced(lib):
    """"count3_rlog" = 3: 1 read group, 6 qualities: rsw = 480, dyn = (9 * 480 + 64) * 4 = 17536, mode 1.  "count3_rlog" = 1 with 4 read groups:
    36 * 384 = 13824 fits at replication 2 < 8, one covariate's table fits too (at the forced rlog) -> mode 2."""
    assert _count3(lib, 1, 6, force_rlog=3) == dict(rsw=480, rlog=3, dyn=17536)
    assert _mode(lib, 1, 6, count3_rlog=3) == 1
    assert _count3(lib, 4, 6, force_rlog=1) == dict(rsw=384, rlog=1, dyn=(13824 + 64) * 4)
    assert _mode(lib, 4, 6, count3_rlog=1) == 2


# ---- the general kernel's plan

def test_general_three_workgroups_per_cu(lib):
    """1 read group, 6 qualities: w = 3: 35485 / 1408 = 25 rows, minus 3 extra rows = 22 slots >= 6 -> three workgroups of 512 threads, one pass;
    dyn = (1 * 9 * 352 + 64) * 4 = 12928."""
    assert _general(lib, 1, 6) == dict(fits=1, wg_per_cu=3, big=0, mg=0, rs=352, ncp=1, qcap=22, passes=1, dyn=12928)


def test_general_two_workgroups_per_cu(lib):
    """1 read group, 30 qualities: w = 3 holds 22 slots < 30; w = 2: 62792 / 1408 = 44 rows - 3 = 41 >= 30 -> two workgroups; dyn = (33 * 352 + 64) * 4
    = 46720.  4 read groups, 6 qualities: w = 3: 35485 / 5632 = 6 - 3 = 3 < 6; w = 2: 62792 / 5632 = 11 - 3 = 8 >= 6 -> two; dyn = (4 * 9 * 352 + 64) * 4."""
    assert _general(lib, 1, 30) == dict(fits=1, wg_per_cu=2, big=0, mg=0, rs=352, ncp=1, qcap=41, passes=1, dyn=46720)
    assert _general(lib, 4, 6) == dict(fits=1, wg_per_cu=2, big=0, mg=0, rs=352, ncp=4, qcap=8, passes=1, dyn=50944)


def test_general_1024_threads(lib):
    """4 read groups, 12 qualities: two workgroups hold 8 slots < 12 -> one workgroup of 1024 threads: 93 rows / 4 covariates = 23 - 3 = 20 >= 12:
    one pass of all covariates and qualities, no MG; dyn = (4 * 15 * 352 + 64) * 4 = 84736."""
    assert _general(lib, 4, 12) == dict(fits=1, wg_per_cu=1, big=1, mg=0, rs=352, ncp=4, qcap=12, passes=1, dyn=84736)


def test_general_mg_saves_a_pass(lib):
    """4 read groups, 30 qualities, 1024 threads.  Plain rows: all 4 covariates hold 93 / 4 - 3 = 20 slots: 2 passes; 2 covariates hold
    93 / 2 - 3 = 43 -> 30 slots: 2 * 1 = 2 passes: no better.  MG rows (768 bytes): 171 / 4 - 3 = 39 >= 30: ONE pass -> MG;
    dyn = (4 * 33 * 192 + 64) * 4 = 101632."""
    assert _general(lib, 4, 30) == dict(fits=1, wg_per_cu=1, big=1, mg=1, rs=192, ncp=4, qcap=30, passes=1, dyn=101632)


def test_general_two_passes(lib):
    """4 read groups, 40 qualities.  Plain rows: 4 covariates x 20 slots: 2 passes (the first plan found with the fewest).  MG: 171 / 4 - 3 = 39 < 40:
    2 passes as well - not fewer, so the plain cells stay; a full pass takes (4 * 23 * 352 + 64) * 4 = 129792 bytes."""
    assert _general(lib, 4, 40) == dict(fits=1, wg_per_cu=1, big=1, mg=0, rs=352, ncp=4, qcap=20, passes=2, dyn=129792)


def test_general_covariate_subsets_64_read_groups(lib):
    """64 read groups, 6 qualities.  Plain rows, k covariates per pass hold min(6, 93 / k - 3) slots: k = 10 -> 6 slots, ceil(64 / 10) = 7 passes
    (k = 9, 8: 8 passes; k = 15: 3 slots, 5 * 2 = 10; ...): 7 at best.  MG rows: 6 slots need 171 / k >= 9, k <= 19: k = 19 -> ceil(64 / 19) = 4
    passes (k = 22 .. 34 with fewer slots: 6) -> MG, 19 covariates a pass; a full pass takes (19 * 9 * 192 + 64) * 4 = 131584 bytes
    (+ 32184 static = 163768 <= 163840)."""
    assert _general(lib, 64, 6) == dict(fits=1, wg_per_cu=1, big=1, mg=1, rs=192, ncp=19, qcap=6, passes=4, dyn=131584)


def test_general_refuses_rows_that_do_not_fit(lib):
    """8000-base reads: a row has 32 + (34 * 8000 >> 4 = 17000) + 2 = 17034 words, with MG 32 + 8500 + 2 = 8534 words = 34136 bytes:
    131400 / 34136 = 3 rows < the four one covariate needs with one quality slot -> refused.  7000-base reads: MG rows of 32 + 7437 + 2 = 7471
    -> 7470 words = 29880 bytes: 4 rows = one slot (plain rows: 14908 words, 2 rows: nothing) -> MG, one quality a pass."""
    assert _general(lib, 1, 2, lmax=8000)["fits"] == 0
    assert _general(lib, 1, 2, lmax=7000) == dict(fits=1, wg_per_cu=1, big=1, mg=1, rs=7470, ncp=1, qcap=1, passes=2, dyn=(4 * 7470 + 64) * 4)


# ---- invariants over every plan

def _sweep(L):
    out = np.zeros((255, 88, len(LMAXS), 12), dtype=np.int64)
    L.plan_sweep((C.c_int * len(LMAXS))(*LMAXS), len(LMAXS), _lds(), out.ctypes.data_as(C.POINTER(C.c_int64)))
    return out


@pytest.fixture(scope="module")
def sweep(lib):
    return _sweep(lib)


def test_every_accepted_plan_fits_the_cu(sweep):
    """dynamic + static LDS of every workgroup a CU holds at once is at most 160 KiB: the general kernel's wg_per_cu workgroups of a full pass,
    the one-length kernel's one"""
    p = dict(zip(GENERAL, np.moveaxis(sweep[..., :9], -1, 0)))
    ok = p["fits"] == 1
    assert ok[:, :, :7].all()  # (rows of up to 250 bases always fit)
    static = np.where(p["big"] == 1, L1024, L512)
    assert ((p["wg_per_cu"] * (p["dyn"] + static))[ok] <= LDS_CU).all()
    assert ((p["big"] == 1) == (p["wg_per_cu"] == 1))[ok].all() and (p["mg"] <= p["big"]).all()
    mode, dyn3 = sweep[..., 9], sweep[..., 11]
    assert ((dyn3 + L3)[mode != 0] <= LDS_CU).all() and (dyn3[mode != 0] > 0).all()
    assert (mode[:, :, LMAXS.index(1023)] == 0).all() and (mode[:, :, LMAXS.index(1022)] != 0).any()


def test_passes_cover_every_covariate_and_quality(sweep):
    """the pass loop steps ncp covariates and qcap quality slots at a time: passes = ceil(n_cov / ncp) * ceil(nq / qcap) with both steps >= 1;
    without the 1024-thread form there is one pass of everything"""
    p = dict(zip(GENERAL, np.moveaxis(sweep[..., :9], -1, 0)))
    ok = p["fits"] == 1
    n_cov = np.arange(1, 256)[:, None, None] + 0 * p["ncp"]
    nq = np.arange(1, 89)[None, :, None] + 0 * p["ncp"]
    assert (p["ncp"][ok] >= 1).all() and (p["qcap"][ok] >= 1).all() and (p["ncp"] <= n_cov)[ok].all()
    passes = -(-n_cov // np.maximum(p["ncp"], 1)) * -(-nq // np.maximum(p["qcap"], 1))
    assert (passes == p["passes"])[ok].all()
    assert (p["passes"] * p["ncp"] * p["qcap"] >= n_cov * nq)[ok].all()
    small = ok & (p["big"] == 0)
    assert (p["passes"][small] == 1).all() and (p["qcap"] >= nq)[small].all() and (p["ncp"] == n_cov)[small].all()


def test_plan_is_a_function_of_its_arguments(lib, sweep):
    """the same arguments give the same plan whatever was planned in between (no state in the header)"""
    assert _general(lib, 64, 6)["passes"] == 4 and _mode(lib, 16, 6) == 2
    assert np.array_equal(_sweep(lib), sweep)


# ---- the scratch block

@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1 << 20])
def test_gather_scratch_layout(lib, n):
    """the block of scratch slot 5: counts in words 0 and 1, the general prologue's queue from word 4, the plain pass's list from word n + 20,
    the record counters 64-word aligned behind 2 n + 48 words, then the other region's sort words, the segments' sizes and first slots -
    disjoint, in this order, inside the size the block is allocated with; and the record area in slot 4"""
    out = (C.c_uint64 * 13)()
    lib.plan_scratch(C.c_uint64(n), out)
    queue, plist, rec_cnt, cw, seg_cap, seg_base, words, pf_grid, cap_s1, other1, slots1, other2, slots2 = list(out)
    maxseg, cstride, maxcov = 256, 64, 256
    assert words == 2 * n + 128 + (maxseg + 1) * cstride + 4 * maxcov + 2 * maxseg + 32
    assert (queue, plist) == (4, n + 20)
    assert rec_cnt == (2 * n + 48 + 63) // 64 * 64 and rec_cnt % 64 == 0
    assert cw == rec_cnt + (maxseg + 1) * cstride and seg_cap == cw + 3 * maxcov + 1 and seg_base == seg_cap + maxseg
    # each region's end is at or in front of the next one's start; the last ends inside the block
    assert 2 <= queue and queue + n <= plist and plist + n <= rec_cnt and seg_base + maxseg + 1 <= words
    # the first pass: workgroups of 16 * 256 records, four waves each; a wave appends at most 16 * 64 class-1 records to segment wave % 64
    assert pf_grid == (n + 4095) // 4096 and cap_s1 == (pf_grid * 4 + 63) // 64 * 1024
    assert cap_s1 * 64 >= n  # the 64 segments hold every record, however the waves fall
    assert (other1, slots1) == (64 * cap_s1, 64 * cap_s1 + n + 64)
    assert (other2, slots2) == (n, 3 * n + 64)  # covariate split: exact segments | the other region | the other region sorted

