"""CPU tests of ApplyBQSR's plan (elprep_amd/csrc/apply_plan.hpp, built by the host compiler through tests/apply_plan_host.cpp): which kernel
takes a read set and with which row dictionary, what follows an overflow, the general kernel's LDS form, the layouts of the dictionary's
block and of the one-length kernel's scratch slot, and when a dictionary built ahead serves a plan.  A wrong plan is silent on the device -
the bytes stay the oracle's, the call merely takes another kernel or rebuilds a dictionary - so the expected values below are worked out by
hand in the docstrings, not computed from the code.

The numbers every case uses.  LDS of a CU: 160 KiB = 163840 bytes.  Static LDS of the kernels (the constants beside their __shared__
declarations; FlatLds<512> is 2064 bytes):
  k_bqsr_apply_flat          APPLY_LDS        = 2064 + 512 * 12 + 512   = 8720
  k_bqsr_apply3              APPLY3_LDS       = 256 + 256               =  512
  its covariate split adds   APPLY3_LDS_SPLIT = 1024 + 1028 + 16 + 236  = 2304
150-base reads: w = 2 * 150 + 1 = 301 cycles.  The one-length kernel's launch takes level 1 = n_cov * (6 + n_qi + 1) * w bytes rounded up
to 16, + 256 level-2 rows of 20 bytes + 16 = level 1 + 5136; it fits if level 1 <= 163840 - 512 - 5136 = 158192.  The general kernel's
level 1 has n1 = n_cov * (n_qi + 1) * w entries of 1 (mode 1) or 2 (mode 2) bytes, rounded up to 16, its level 2 (n_dict + 1) rows of 32
(mode 1) or 17 (mode 2) bytes, + 16; both with 8720 static must be <= 163840."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tests", "libapply_plan_host.so")
HDRS = [os.path.join(ROOT, "elprep_amd", "csrc", h) for h in ("apply_plan.hpp", "bqsr_plan.hpp")]

LDS_CU = 160 * 1024
LF, LA3, LA3S = 8720, 512, 2304
LUT_T2_CAP = 3855
LMAXS = (1, 16, 17, 100, 150, 151, 250, 1022, 1023)  # (those of test_bqsr_plan_cpu.py)
PLAN = ("chk", "want3", "qlo", "n_qi", "lmax", "n_rows", "n1", "a3", "dyn3", "flat_lds_lut")
FLAT = ("mode", "dyn", "per_cu", "grid")
DICT = ("n_slots", "n_rows", "n1", "counter", "slots", "slot_id", "row_slot", "t1", "t2", "t2_bytes", "words")
A3L = ("group", "rpi", "per_cu", "grid", "recs", "dump", "ridx", "cw", "blk", "size8")


@pytest.fixture(scope="module")
def lib():
    src = os.path.join(ROOT, "tests", "apply_plan_host.cpp")
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(p) for p in [src] + HDRS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", SO, src])
    L = C.CDLL(SO)
    L.ap_flat.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p]
    L.ap_apply3_launch.argtypes = [C.c_uint64, C.c_uint32, C.c_int, C.c_uint64, C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_void_p]
    L.ap_serves.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    return L


def _shape(n=1_000_000, n_cov=4, length=150, uniform_len=None, max_cycle=500, qlo=10, qhi=41, apply_kernel=0, apply_wgs=0, n_cu=256):
    """4 read groups, 150-base reads, sampled qualities 10 .. 41, --max-cycle 500, 256 CUs unless said otherwise"""
    return (C.c_int64 * 13)(n, n_cov, length, length if uniform_len is None else uniform_len, max_cycle, qlo, qhi, apply_kernel, apply_wgs, n_cu, LF, LA3, LA3S)


def _plan(L, **kw):
    out = (C.c_int64 * 10)()
    L.ap_plan(_shape(**kw), out)
    return dict(zip(PLAN, out))


def _overflow(L, a3, **kw):
    out = (C.c_int64 * 1)()
    return L.ap_overflow(_shape(**kw), a3, out), out[0]


def _flat(L, n_dict, nsteps=10000, **kw):
    out = (C.c_int64 * 4)()
    L.ap_flat(_shape(**kw), n_dict, nsteps, out)
    return dict(zip(FLAT, out))


def _a3l(L, n, length, n_cu=256, dyn=18080, split=0, apply_wgs=0):
    out = (C.c_int64 * 10)()
    L.ap_apply3_launch(n, length, n_cu, dyn, split, apply_wgs, LA3, LA3S, out)
    return dict(zip(A3L, out))


# ---- the first form

def test_apply3_bytes(lib):
    """4 read groups, qualities 6 .. 45 (40 resident), 150 bases: level 1 = 4 * (6 + 40 + 1) * 301 = 56588 bytes -> 56592, + 256 rows of 20 bytes
    + 16 = 61728; fits (+ 512 static).  16 read groups: 226352 bytes of level 1 alone do not."""
    out = (C.c_uint64 * 1)()
    assert lib.plan_apply3(4, 40, 150, C.c_uint64(LA3), out) == 0 and out[0] == 61728
    assert lib.plan_apply3(16, 40, 150, C.c_uint64(LA3), out) == 1


def test_one_table(lib):
    """4 read groups, qualities up to 41: the one-length kernel is resident from quality 6 whatever the smallest sampled one (10) was: n_qi = 36.
    Level 1 = 4 * 43 * 301 = 51772 -> 51776 <= 158192: form 1 with dyn = 51776 + 5136 = 56912.  The dictionary covers n_rows = 4 * 36 * 301 =
    43344 rows, the general kernel's level 1 would have n1 = 4 * 37 * 301 = 44548 entries (+ 8720 fits: it could hold a LUT in LDS too)."""
    assert _plan(lib) == dict(chk=0, want3=1, qlo=6, n_qi=36, lmax=150, n_rows=43344, n1=44548, a3=1, dyn3=56912, flat_lds_lut=1)


def test_covariate_split(lib):
    """16 read groups, same shape: 16 * 43 * 301 = 207088 > 158192, one covariate's 12943 -> 12944 fits: form 2, dyn = 12944 + 5136 = 18080
    (n1 = 16 * 37 * 301 = 178192 entries: no LDS LUT for the general kernel).  "apply_kernel" = 3 forces form 2 on the 4-group case;
    "apply_kernel" = 1 gives 0 - and the resident range is the hint's then: qlo = 10, n_qi = 32, n1 = 4 * 33 * 301 = 39732."""
    assert _plan(lib, n_cov=16) == dict(chk=0, want3=1, qlo=6, n_qi=36, lmax=150, n_rows=173376, n1=178192, a3=2, dyn3=18080, flat_lds_lut=0)
    p = _plan(lib, apply_kernel=3)
    assert (p["a3"], p["dyn3"], p["want3"]) == (2, 18080, 1)
    assert _plan(lib, apply_kernel=1) == dict(chk=0, want3=0, qlo=10, n_qi=32, lmax=150, n_rows=4 * 32 * 301, n1=39732, a3=0, dyn3=0, flat_lds_lut=1)


def test_overflow_steps(lib):
    """more distinct rows than one-byte ids hold: 1 -> 2 (one covariate's tables fit: dyn 18080) -> 0; with one read group there is nothing to
    split: 1 -> 0"""
    assert _overflow(lib, 1) == (2, 18080)
    assert _overflow(lib, 2)[0] == 0
    assert _overflow(lib, 1, n_cov=1)[0] == 0


def test_ragged_reads_rule_the_one_length_kernel_out(lib):
    """uniform_len = 0: no one length; the general kernel with the hint's range"""
    p = _plan(lib, uniform_len=0)
    assert (p["want3"], p["a3"], p["qlo"], p["n_qi"], p["flat_lds_lut"]) == (0, 0, 10, 32, 1)


def test_reads_shorter_than_one_block_rule_it_out(lib):
    """the one-length kernel works in whole 16-byte blocks: 15 bases against 16 (level 1 = 4 * 43 * 33 = 5676 -> 5680, dyn = 10816)"""
    p = _plan(lib, length=15)
    assert (p["want3"], p["a3"], p["lmax"]) == (0, 0, 15)
    p = _plan(lib, length=16)
    assert (p["want3"], p["a3"], p["dyn3"], p["lmax"]) == (1, 1, 10816, 16)


def test_a_read_that_can_exceed_max_cycle_rules_it_out(lib):
    """max_l_seq = max_cycle + 1: the kernel has to check every cycle (chk) - no one-length kernel, no LDS LUT; max_l_seq = max_cycle: both"""
    p = _plan(lib, max_cycle=149)
    assert (p["chk"], p["want3"], p["a3"], p["flat_lds_lut"]) == (1, 0, 0, 0)
    p = _plan(lib, max_cycle=150)
    assert (p["chk"], p["want3"], p["a3"], p["flat_lds_lut"]) == (0, 1, 1, 1)


def test_no_quality_hint_rules_it_out(lib):
    """qhi = -1 (no quality >= 6 sampled; qlo = 0): nothing is resident: n_qi = 0, no rows, n1 = 4 * 1 * 301 = 1204, dense LUT"""
    assert _plan(lib, qlo=0, qhi=-1) == dict(chk=0, want3=0, qlo=0, n_qi=0, lmax=150, n_rows=0, n1=1204, a3=0, dyn3=0, flat_lds_lut=0)


def test_row_cap(lib):
    """no dictionary over 2^22 rows or more.  2^22 - 1 = 4194303 = 89 * 69 * 683: 89 read groups, qualities 6 .. 74, 341-base reads - under the
    cap; all covariates' level 1 (89 * 76 * 683) does not fit, one covariate's 76 * 683 = 51908 -> 51920 does: form 2, dyn = 57056.  2^22
    itself has no odd factor 2 lmax + 1 > 1: the next shape up is one more quality, 89 * 70 * 683 = 4255090 rows - form 0, though one
    covariate's 77 * 683 = 52591 bytes would fit."""
    p = _plan(lib, n_cov=89, length=341, qhi=74)
    assert (p["n_rows"], p["a3"], p["dyn3"]) == ((1 << 22) - 1, 2, 57056)
    p = _plan(lib, n_cov=89, length=341, qhi=75)
    assert (p["n_rows"], p["a3"], p["want3"]) == (4255090, 0, 1)
    out = (C.c_uint64 * 1)()
    assert lib.plan_apply3(1, 70, 341, C.c_uint64(LA3), out) == 0


# ---- the general kernel's form

def test_flat_forms_by_distinct_rows(lib):
    """"apply_kernel" = 1, 4 read groups, qualities 10 .. 41: n1 = 39732, 10000 steps, 256 CUs.
    255 rows: 256 one-byte ids: mode 1, 39744 + 256 * 32 + 16 = 47952 bytes; (47952 + 8720 = 56672) goes twice into 163840: grid 512.
    256 rows: mode 2, 2 * 39732 = 79464 -> 79472, + 257 * 17 = 4369, + 16 = 83857; 92577 goes once: grid 256.
    3854 rows: 79472 + 3855 * 17 = 65535, + 16 = 145023 (+ 8720 = 153743 fits).  3855 rows: offsets no longer fit 16 bits: the dense LUT,
    8 workgroups per CU: grid 2048; and 300 steps only: grid 300."""
    kw = dict(apply_kernel=1)
    assert _flat(lib, 255, **kw) == dict(mode=1, dyn=47952, per_cu=2, grid=512)
    assert _flat(lib, 256, **kw) == dict(mode=2, dyn=83857, per_cu=1, grid=256)
    assert _flat(lib, LUT_T2_CAP - 1, **kw) == dict(mode=2, dyn=145023, per_cu=1, grid=256)
    assert _flat(lib, LUT_T2_CAP, **kw) == dict(mode=0, dyn=0, per_cu=8, grid=2048)
    assert _flat(lib, LUT_T2_CAP, nsteps=300, **kw) == dict(mode=0, dyn=0, per_cu=8, grid=300)
    assert _flat(lib, 0xFFFFFFFF, **kw) == dict(mode=0, dyn=0, per_cu=8, grid=2048)  # (no dictionary)
    assert _flat(lib, 255, qlo=0, qhi=-1) == dict(mode=0, dyn=0, per_cu=8, grid=2048)  # (the plan has no LDS LUT)


def test_flat_level_1_fits_but_not_with_level_2(lib):
    """250-base reads (w = 501), qualities 6 .. 78: n1 = 4 * 74 * 501 = 148296; + 8720 = 157016 <= 163840, the plan builds a dictionary.  With
    255 rows: 148304 + 8192 + 16 = 156512, + 8720 = 165232 > 163840: the dense form"""
    kw = dict(apply_kernel=1, length=250, qlo=6, qhi=78)
    p = _plan(lib, **kw)
    assert (p["n1"], p["flat_lds_lut"]) == (148296, 1)
    assert _flat(lib, 255, **kw)["mode"] == 0


def test_flat_workgroups_per_cu(lib):
    """min(3, 163840 / (dyn + 8720)).  Three while dyn <= 45893: qualities 6 .. 38, n1 = 4 * 34 * 301 = 40936 -> 40944; 153 rows: 40944 + 154 * 32
    + 16 = 45888 (54608 * 3 = 163824): 3; 154 rows: 45920 (54640 * 3 = 163920): 2.  Two while dyn <= 73200: qualities 6 .. 58, n1 = 4 * 54 * 301
    = 65016 -> 65024; 254 rows: 65024 + 255 * 32 + 16 = 73200 (81920 * 2 = 163840 exactly): 2; 255 rows: 73232: 1."""
    kw = dict(apply_kernel=1, qlo=6, qhi=38)
    assert _flat(lib, 153, **kw) == dict(mode=1, dyn=45888, per_cu=3, grid=768)
    assert _flat(lib, 154, **kw) == dict(mode=1, dyn=45920, per_cu=2, grid=512)
    kw = dict(apply_kernel=1, qlo=6, qhi=58)
    assert _flat(lib, 254, **kw) == dict(mode=1, dyn=73200, per_cu=2, grid=512)
    assert _flat(lib, 255, **kw) == dict(mode=1, dyn=73232, per_cu=1, grid=256)


# ---- the one-length kernel's launch

def test_apply3_lane_groups(lib):
    """150 and 151 bases: bpr = 10 blocks per read, the last one moved back; slot s ends in lane 10 s + 9, which is odd: never lane 0 of a wave:
    group 512, rpi = 51.  33 bases: bpr = 3, slot 42 ends in lane 3 * 42 + 2 = 128 = lane 0 of wave 2, its other blocks in wave 1: whole reads
    per wave: group 64, rpi = 21 * 8 = 168.  A multiple of 16 has no block moved back: group 512 whatever bpr (48 bases: 170 reads a trip,
    32: 256, 160: 51)."""
    assert [(_a3l(lib, 10**6, n)["group"], _a3l(lib, 10**6, n)["rpi"]) for n in (150, 151)] == [(512, 51), (512, 51)]
    assert (_a3l(lib, 10**6, 33)["group"], _a3l(lib, 10**6, 33)["rpi"]) == (64, 168)
    assert [(_a3l(lib, 10**6, n)["group"], _a3l(lib, 10**6, n)["rpi"]) for n in (48, 32, 160)] == [(512, 170), (512, 256), (512, 51)]


def test_apply3_workgroups_per_cu_and_grid(lib):
    """dyn 18080: 163840 / (18080 + 512) = 8.8 -> 3 workgroups per CU, with the split 163840 / 20896 = 7.8 -> 3; "apply_wgs" 1 .. 3 caps it, 0 and 4
    do not.  dyn 56912 (the one table): 163840 / 57424 = 2.85 -> 2, which "apply_wgs" = 3 does not raise.  10^6 reads in trips of 51: 19608 trips,
    grid = 256 * per_cu; 1000 reads: 20 trips."""
    assert [_a3l(lib, 10**6, 150, apply_wgs=k)["per_cu"] for k in (0, 1, 2, 3, 4)] == [3, 1, 2, 3, 3]
    assert [_a3l(lib, 10**6, 150, apply_wgs=k)["grid"] for k in (0, 1, 2, 3, 4)] == [768, 256, 512, 768, 768]
    assert _a3l(lib, 10**6, 150, split=1)["per_cu"] == 3
    assert [_a3l(lib, 10**6, 150, dyn=56912, apply_wgs=k)["per_cu"] for k in (0, 1, 3)] == [2, 1, 2]
    assert _a3l(lib, 1000, 150)["grid"] == 20


def test_apply3_slot_5(lib):
    """4 CUs, 3 workgroups each; 1001 reads of 150 bases: 20 trips -> grid 12.  Records (1001 + 5) & ~1 = 1006 8-byte units, the dump 12 * 512
    lanes * 16 bytes = 12288 units: dump at byte 8048, staging indices at 8048 + 98304 = 106352, cw behind 1002 indices: 110360, the
    workgroups' counts behind 3 * 256 + 8 words: 113464.  Size: 1006 + 12288 + 8 = 13302 units without the split, + 501 + 520 + 131072 =
    145395 with it.  1000 reads: 1004 units of records: 8032, 106336, + 1000 indices: 110336, 113440; 13300 and + 500 + 520 + 131072 = 145392."""
    for split, size8 in ((0, 13302), (1, 145395)):
        assert _a3l(lib, 1001, 150, n_cu=4, split=split) == dict(group=512, rpi=51, per_cu=3, grid=12, recs=0, dump=8048, ridx=106352, cw=110360, blk=113464, size8=size8)
    for split, size8 in ((0, 13300), (1, 145392)):
        assert _a3l(lib, 1000, 150, n_cu=4, split=split) == dict(group=512, rpi=51, per_cu=3, grid=12, recs=0, dump=8032, ridx=106336, cw=110336, blk=113440, size8=size8)
    # the split's regions end inside the slot: indices, cw's 769 words, 1024 x 256 counts
    for n, size8 in ((1001, 145395), (1000, 145392)):
        p = _a3l(lib, n, 150, n_cu=4, split=1)
        assert p["ridx"] + 4 * n <= p["cw"] and p["cw"] + 4 * 769 <= p["blk"] and p["blk"] + 4 * 1024 * 256 <= 8 * size8


# ---- the dictionary built ahead

def test_built_ahead_serves_the_plan_that_built_it(lib):
    """the dictionary the upload builds for a shape serves the apply call's plan of the same shape - not if the LUT came with the call, not
    if one of form / qlo / n_qi / lmax / max_cycle / n_cov differs (the one-table case: 1, 6, 36, 150, 500, 4), not if nothing was built"""
    assert lib.ap_serves(None, _shape(), _shape(), 0) == 1
    assert lib.ap_serves(None, _shape(), _shape(), 1) == 0
    base = (1, 6, 36, 150, 500, 4)
    assert lib.ap_serves((C.c_int64 * 6)(*base), None, _shape(), 0) == 1
    for k, other in enumerate((2, 7, 35, 151, 501, 5)):
        b = list(base)
        b[k] = other
        assert lib.ap_serves((C.c_int64 * 6)(*b), None, _shape(), 0) == 0, k
    assert lib.ap_serves((C.c_int64 * 6)(0, 6, 36, 150, 500, 4), None, _shape(), 0) == 0
    # the same through the shapes: another form ("apply_kernel" = 3), another largest quality, read length, --max-cycle, number of read groups
    for kw in (dict(apply_kernel=3), dict(qhi=42), dict(length=151), dict(max_cycle=501), dict(n_cov=5)):
        assert lib.ap_serves(None, _shape(), _shape(**kw), 0) == 0, kw
        assert lib.ap_serves(None, _shape(**kw), _shape(**kw), 0) == 1, kw
    # no one-length form, nothing built: ragged reads
    assert lib.ap_serves(None, _shape(uniform_len=0), _shape(uniform_len=0), 0) == 0


# ---- invariants over every plan

@pytest.fixture(scope="module")
def sweep(lib):
    out = np.zeros((255, 88, len(LMAXS), 18), dtype=np.int64)
    lib.ap_sweep((C.c_int * len(LMAXS))(*LMAXS), len(LMAXS), (C.c_int64 * 3)(LF, LA3, LA3S), out.ctypes.data_as(C.POINTER(C.c_int64)))
    return out


def test_every_chosen_form_fits_the_cu(sweep):
    """dyn + static <= 160 KiB wherever the one-length kernel takes a form (with APPLY3_LDS, the static LDS its condition counts) and wherever
    the general kernel takes an LDS form (255 and LUT_T2_CAP - 1 distinct rows).  Form 2's launch has the split's 2304 bytes on top, which
    the condition does not count: they fit too for every read length up to 250 (one covariate's level 1 is at most 95 * 501 = 47595
    bytes there); at 1022 bases and more some shapes (77 * 2045 = 157465) pass the condition and not the launch."""
    a3, dyn3 = sweep[..., 0], sweep[..., 1]
    assert ((dyn3 + LA3)[a3 != 0] <= LDS_CU).all() and (dyn3[a3 != 0] > 0).all()
    assert (a3[:, :, LMAXS.index(1)] == 0).all() and (a3[:, :, LMAXS.index(16)] != 0).all()  # (whole 16-byte blocks)
    assert ((dyn3 + LA3 + LA3S)[..., :LMAXS.index(250) + 1][a3[..., :LMAXS.index(250) + 1] == 2] <= LDS_CU).all()
    for mode, dyn in ((sweep[..., 3], sweep[..., 4]), (sweep[..., 5], sweep[..., 6])):
        assert ((dyn + LF)[mode != 0] <= LDS_CU).all() and (dyn[mode != 0] > 0).all()
        assert (mode[sweep[..., 2] == 0] == 0).all()
    assert (sweep[..., 3] <= 1).all() and (sweep[..., 5] != 1).all() and (sweep[..., 3] == 1).any() and (sweep[..., 5] == 2).any()


def test_dictionary_block_layout(sweep):
    """counter | slots | slot_id | row_slot | t1 | t2 in this order, disjoint, ending inside `words`; `words` is the size the block always had:
    256 counters + 2 n_slots (a power of two >= 1024 and >= 2 n_rows) + n_rows + n1 + a quarter of the level-2 bytes (3856 rows of one
    dictionary or 256 per covariate, 17 bytes each) + 80"""
    d = dict(zip(DICT, np.moveaxis(sweep[..., 7:], -1, 0)))
    n_cov = np.arange(1, 256)[:, None, None] + 0 * d["words"]
    n_qi = np.arange(1, 89)[None, :, None] + 0 * d["words"]
    w = 2 * np.asarray(LMAXS)[None, None, :] + 1
    n_rows, n1 = n_cov * n_qi * w, n_cov * (n_qi + 1) * w
    n_slots = np.maximum(1024, 2 ** np.ceil(np.log2(2 * n_rows)).astype(np.int64))
    assert (n_slots >= 2 * n_rows).all() and ((n_slots == 1024) | (n_slots < 4 * n_rows)).all()
    t2_bytes = np.maximum(3856 * 17, n_cov * 256 * 17)
    assert (d["n_rows"] == n_rows).all() and (d["n1"] == n1).all() and (d["n_slots"] == n_slots).all() and (d["t2_bytes"] == t2_bytes).all()
    assert (d["words"] == 256 + 2 * n_slots + n_rows + n1 + t2_bytes // 4 + 64 + 16).all()
    assert (d["counter"] == 0).all() and (d["counter"] + 256 <= d["slots"]).all()
    assert (d["slots"] + n_slots <= d["slot_id"]).all() and (d["slot_id"] + n_slots <= d["row_slot"]).all()
    assert (d["row_slot"] + n_rows <= d["t1"]).all() and (2 * d["t1"] + n1 <= 2 * d["t2"]).all()
    assert (4 * d["t2"] + t2_bytes <= 4 * d["words"]).all()


def test_plan_alone_under_the_sanitizers(tmp_path):
    """tests/apply_plan_asan.cpp: every byte of every region of the dictionary's block and of scratch slot 5 written through the layouts'
    offsets, in heap blocks of exactly the layouts' sizes.  The sanitizers' runtimes are linked into the program where the compiler has them
    as archives, so that nothing has to stand in front of them in the list of libraries."""
    src = os.path.join(ROOT, "tests", "apply_plan_asan.cpp")
    exe = str(tmp_path / "apply_plan_asan")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src]
    if subprocess.call(cmd + ["-static-libasan", "-static-libubsan"], stderr=subprocess.DEVNULL) != 0:
        subprocess.check_call(cmd)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "apply_plan_asan: ok" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stdout, r.stderr[-2000:])
