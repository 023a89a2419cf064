"""CPU tests of the Smith-Waterman kernels' algorithm (elprep_amd/csrc/sw_core.hpp) as tests/sw_host.cpp walks it - tiles, strips, the
value handed to the right neighbour one step later, the tile edge, the backtrack's layout, the end search as a reduction, the traceback's
64-cell fetch, the clean-up in one pass - against tests/swref_c.c on the case lists the GPU tests use (tests/sw_cases.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import sw_cases, swref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tests", "libsw_host.so")
HDRS = [os.path.join(ROOT, "elprep_amd", "csrc", h) for h in ("sw_core.hpp", "sw_plan.hpp")]


@pytest.fixture(scope="module")
def lib():
    src = os.path.join(ROOT, "tests", "sw_host.cpp")
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(p) for p in [src] + HDRS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", SO, src])
    L = C.CDLL(SO)
    L.swh_batch.argtypes = [C.c_void_p] * 4 + [C.c_uint64] * 2 + [C.c_void_p] * 2 + [C.c_int32] * 4 + [C.c_int] + [C.c_void_p] * 4
    L.swh_run.argtypes = [C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32] + [C.c_int32] * 4 + [C.c_int, C.c_void_p, C.c_void_p]
    L.swh_layout_ok.argtypes = [C.c_uint32, C.c_uint32]
    return L


def _same(got, want, case):
    for g, w, what in zip(got, want, ("cigar_off", "cigar", "offset")):
        if not np.array_equal(g, w):
            k = int(np.flatnonzero(np.asarray(g[:min(len(g), len(w))]) != np.asarray(w[:min(len(g), len(w))]))[0]) if len(g) and len(w) else 0
            raise AssertionError("%s: %s differs first at %d" % (case.name, what, k))


def test_the_walk_equals_the_restatement_on_the_shared_cases(lib):
    n = 0
    for case in sw_cases.core_cases():
        _same(sw_cases.run_batch(lib.swh_batch, case), sw_cases.expected(case), case)
        n += len(case.ref_of)
    assert n > 20000


def test_hand_cases_through_the_walk(lib):
    """the table of tests/test_swref_cpu.py once more: 3D inside 8M .. 9M, the clip on both sides and its leadingIndel form"""
    def run(ref, alt, params, strategy):
        out, off = (C.c_uint32 * (len(ref) + len(alt) + 2))(), C.c_int32()
        n = lib.swh_run(ref, len(ref), alt, len(alt), *params, strategy, out, C.byref(off))
        assert n >= 0
        return swref.cigar_string(swref.decode(out[:n])), off.value
    assert run(b"ACGTACGT", b"ACGT", swref.P1, swref.SOFTCLIP) == ("4M", 4)
    assert run(b"AAAACCCCGGGG", b"TTTTCCCCGGGG", swref.P1, swref.SOFTCLIP) == ("4I8M", 4)
    assert run(b"ACGTACGTTTGACCAGTACA", b"ACGTACGTACCAGTACA", swref.P2, swref.LEADING_INDEL) == ("8M3D9M", 0)
    assert run(b"ACG", b"TACGT", swref.P1, swref.SOFTCLIP) == ("1S3M1S", 0)
    assert run(b"ACG", b"TACGT", swref.P1, swref.LEADING_INDEL) == ("1I3M1I", 0)


def test_long_gaps_and_the_clamp(lib):
    """a deletion of 300 is one backtrack value of 300 (beyond a byte); leadingIndel with gap_extend = -60000 on 300 x 300: the first row
    reaches -110 - 299 * 60000 = -17940110 unclamped ... and on 2000 x 2000 passes -100000000 while every interior cell stays at or
    above it (the GPU test runs that size; here 1700 x 1700 already passes the cutoff: -110 - 1699 * 60000 = -101940110)"""
    rng = np.random.default_rng(9)
    ref = sw_cases.rand_seq(rng, 1700)
    alt = bytearray(ref)
    for at in rng.integers(0, 1700, 40):
        alt[int(at)] = ord("A")
    case = sw_cases._pairs("clamp", [(ref, bytes(alt)), (ref[:300], bytes(alt[:300]))], (25, -50, -110, -60000), swref.LEADING_INDEL)
    _same(sw_cases.run_batch(lib.swh_batch, case), sw_cases.expected(case), case)


def test_every_cell_has_a_place_of_its_own(lib):
    """sw_bt_index is the strips' store address, one to one onto the planned cells: one lane, a full strip, a partial last strip, a full
    tile, one column into the second tile, three tiles"""
    for m in (1, 2, 5, 64, 130):
        for n in (1, 3, 4, 5, 255, 256, 257, 300, 513):
            assert lib.swh_layout_ok(m, n) == 1, (m, n)
