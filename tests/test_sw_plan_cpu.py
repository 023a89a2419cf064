"""CPU tests of the Smith-Waterman calls' plan (elprep_amd/csrc/sw_plan.hpp and the layout arithmetic of sw_core.hpp, built by the host
compiler through tests/sw_plan_host.cpp): the limits and refusals, a problem's share of the chunk scratch, the chunk cuts, the slots'
layouts - expected values worked out by hand in the docstrings -, the plan on its own under the sanitizers (tests/sw_plan_asan.cpp), and
the two entry points' presence."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from elprep_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tests", "libsw_plan_host.so")
HDRS = [os.path.join(ROOT, "elprep_amd", "csrc", h) for h in ("sw_plan.hpp", "sw_core.hpp")]
NEW = ("elp_sw_align", "elp_sw_align_reads")
OK, ARG, UNSUPPORTED = 0, 1, 2


@pytest.fixture(scope="module")
def lib():
    src = os.path.join(ROOT, "tests", "sw_plan_host.cpp")
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(p) for p in [src] + HDRS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", SO, src])
    L = C.CDLL(SO)
    for name, n_args in (("sp_tiles", 1), ("sp_tile_lanes", 2), ("sp_bt_cells", 2)):
        getattr(L, name).restype = C.c_uint64
        getattr(L, name).argtypes = [C.c_uint32] * n_args
    L.sp_chunks.restype = C.c_uint64
    L.sp_chunks.argtypes = [C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    L.sp_check_params.argtypes = [C.c_int32] * 4 + [C.c_int, C.c_char_p, C.c_uint64]
    L.sp_check_batch.argtypes = [C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64] + [C.c_void_p] * 5 + [C.c_char_p, C.c_uint64]
    L.sp_need.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p]
    L.sp_per_problem.argtypes = [C.c_uint64, C.c_uint64, C.c_void_p]
    L.sp_inputs.argtypes = [C.c_uint64] * 3 + [C.c_void_p]
    return L


# ---- the entry points
def test_the_two_entry_points_are_exported_and_listed():
    L = _lib.hip()
    for name in NEW:
        assert hasattr(L, name), name
        assert name in _lib.HIP_SYMBOLS, name


def test_the_entry_points_reject_null_contexts_without_a_gpu():
    L = _lib.hip()
    null, n = C.c_void_p(0), C.c_uint64(0)
    assert L.elp_sw_align(null, 0, null, null, 0, null, null, 0, null, null, 10, -15, -30, -5, 0, null, 0, null, null, C.byref(n)) != 0
    assert L.elp_sw_align_reads(null, 0, null, null, 0, null, null, 10, -15, -30, -5, 0, null, 0, null, null, C.byref(n)) != 0


def test_constants(lib):
    """sequences of at most 4095 bytes, parameters within +-65535, four columns per lane and so tiles of 256, a gibibyte of chunk
    scratch by default, descriptors of 4 + 4 + 3 * 8 = 32 bytes.  The arithmetic the limits rest on: MinInt32 / 2 - 4095 * 65535 =
    -1073741824 - 268365825 = -1342107649 > -2147483648, and 8190 * 65535 = 536731650 < 2^30"""
    out = (C.c_uint64 * 6)()
    lib.sp_consts(out)
    assert tuple(out) == (4095, 65535, 4, 256, 1 << 30, 32)
    assert -(1 << 30) - 4095 * 65535 == -1342107649 > -(1 << 31) and 8190 * 65535 == 536731650 < (1 << 30)


# ---- limits and refusals
def test_parameters(lib):
    """+-65535 pass, +-65536 are UNSUPPORTED in each of the four places; strategies 0..3 pass, -1 and 4 are ARG (before the parameters
    are looked at)"""
    text = C.create_string_buffer(200)
    assert lib.sp_check_params(65535, -65535, -65535, 65535, 3, text, 200) == OK
    for at in range(4):
        for bad in (65536, -65536):
            p = [10, -15, -30, -5]
            p[at] = bad
            assert lib.sp_check_params(*p, 0, text, 200) == UNSUPPORTED and b"65535" in text.value
    for s in range(4):
        assert lib.sp_check_params(10, -15, -30, -5, s, text, 200) == OK
    assert lib.sp_check_params(10, -15, -30, -5, 4, text, 200) == ARG and lib.sp_check_params(65536, 0, 0, 0, -1, text, 200) == ARG


def _batch(lib, a_lens, b_lens, ref_of, alt_of, a_off=None, b_off=None):
    a_off = np.asarray(a_off if a_off is not None else np.concatenate([[0], np.cumsum(a_lens)]), dtype=np.uint64)
    b_off = np.asarray(b_off if b_off is not None else np.concatenate([[0], np.cumsum(b_lens)]), dtype=np.uint64)
    ref_of, alt_of = np.asarray(ref_of, dtype=np.uint32), np.asarray(alt_of, dtype=np.uint32)
    n = ref_of.size
    lr, la, bound, text = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32), C.c_uint64(), C.create_string_buffer(200)
    rc = lib.sp_check_batch(a_off.size - 1, a_off.ctypes.data, b_off.size - 1, b_off.ctypes.data, n, ref_of.ctypes.data, alt_of.ctypes.data, lr.ctypes.data, la.ctypes.data,
                            C.byref(bound), text, 200)
    return rc, text.value.decode(), bound.value, lr[:n].tolist(), la[:n].tolist()


def test_batches(lib):
    """pools of 3 and 2 sequences, three problems: lengths gathered through the index pairs; the operation bound is the sum of len_ref +
    len_alt + 2 = (5 + 7 + 2) + (4095 + 1 + 2) + (5 + 1 + 2) = 14 + 4098 + 8 = 4120.  An UNUSED empty or oversize sequence is no refusal"""
    rc, _, bound, lr, la = _batch(lib, [5, 4095, 0], [1, 7, 4096], [0, 1, 0], [1, 0, 0])
    assert (rc, bound, lr, la) == (OK, 4120, [5, 4095, 5], [7, 1, 1])
    assert _batch(lib, [], [], [], [])[:3] == (OK, "", 0)
    rc, text, *_ = _batch(lib, [5, 0], [3], [0, 1], [0, 0])
    assert rc == ARG and "problem 1 uses an empty reference" in text
    rc, text, *_ = _batch(lib, [5], [3, 0], [0], [1])
    assert rc == ARG and "empty alternate" in text
    rc, text, *_ = _batch(lib, [4096], [3], [0], [0])
    assert rc == UNSUPPORTED and "4096" in text
    rc, text, *_ = _batch(lib, [5], [3, 4096], [0], [1])
    assert rc == UNSUPPORTED
    assert _batch(lib, [5], [3], [1], [0])[0] == ARG and _batch(lib, [5], [3], [0], [1])[0] == ARG
    assert _batch(lib, None, [3], [0], [0], a_off=[1, 5])[0] == ARG      # does not start at 0
    assert _batch(lib, None, [3], [0], [0], a_off=[0, 5, 4])[0] == ARG   # decreases


# ---- the backtrack's layout
def test_tiles_and_cells(lib):
    """tiles of 256 columns: 1 .. 256 -> 1, 257 -> 2, 513 -> 3, 4095 -> 16.  Lanes of a tile: 64, the last ceil(width / 4): n = 1, 4 -> 1;
    5 -> 2; 150 -> 38; 256 -> 64; 257 -> 64 and 1.  Cells: a tile of L lanes takes (m + L - 1) steps of L * 4 cells.
    500 x 150: 537 * 152 = 81624.  1 x 1: 1 * 4.  400 x 300: (400 + 63) * 256 = 118528 for the full tile + (400 + 10) * 11 * 4 = 18040
    for the 44 columns behind it = 136568"""
    assert [lib.sp_tiles(n) for n in (1, 256, 257, 513, 4095)] == [1, 1, 2, 3, 16]
    assert [lib.sp_tile_lanes(n, 0) for n in (1, 4, 5, 150, 256, 257)] == [1, 1, 2, 38, 64, 64]
    assert lib.sp_tile_lanes(257, 1) == 1 and lib.sp_tile_lanes(513, 2) == 1 and lib.sp_tile_lanes(300, 1) == 11
    assert lib.sp_bt_cells(500, 150) == 81624 and lib.sp_bt_cells(1, 1) == 4 and lib.sp_bt_cells(400, 300) == 136568


def _need(lib, m, n):
    out = (C.c_uint64 * 4)()
    lib.sp_need(m, n, out)
    return tuple(out)


def test_what_a_problem_needs(lib):
    """60 x 45: 12 lanes, (60 + 11) * 48 = 3408 cells; 60 + 45 + 3 operations + the count word = 109 -> 110 words; no edge: 6816 + 440 =
    7256 bytes.  400 x 300: 136568 cells, 704 words, an edge of 3 * 400 = 1200 words: 273136 + 2816 + 4800 = 280752.  1 x 1: 4 cells, 6
    words: 32 bytes.  3 x 2: 12 cells, 9 -> 10 words: 64 bytes.  3 x 257: the edge is 9 -> 10 words"""
    assert _need(lib, 60, 45) == (3408, 110, 0, 7256)
    assert _need(lib, 400, 300) == (136568, 704, 1200, 280752)
    assert _need(lib, 1, 1) == (4, 6, 0, 32)
    assert _need(lib, 3, 2) == (12, 10, 0, 64)
    assert _need(lib, 3, 257)[2] == 10 and _need(lib, 3, 256)[2] == 0


def _chunks(lib, lens, budget):
    lr, la = np.array([m for m, _ in lens], np.uint32), np.array([n for _, n in lens], np.uint32)
    cuts, prob_at, chunk_at = np.zeros((64, 5), np.uint64), np.zeros((len(lens), 3), np.uint64), np.zeros((64, 4), np.uint64)
    k = lib.sp_chunks(len(lens), lr.ctypes.data, la.ctypes.data, budget, cuts.ctypes.data, 64, prob_at.ctypes.data, chunk_at.ctypes.data)
    assert k <= 64
    return cuts[:k].tolist(), prob_at.tolist(), chunk_at[:k].tolist()


def test_chunk_cuts(lib):
    """three of 60 x 45 (7256 bytes each), one of 400 x 300 (280752), two of 60 x 45, budget 15000: two fit (14512), the third would make
    21768: cut.  The third alone; the large one does not fit behind it and is larger than the budget: a chunk of its own; the last two
    together.  Offsets restart in every chunk: the second of a pair lies 3408 cells and 110 words behind the first.  A chunk's arrays:
    backtrack at 0, raw operations behind its 2-byte cells, the edge behind the raw words"""
    small, large = (60, 45), (400, 300)
    cuts, prob_at, chunk_at = _chunks(lib, [small, small, small, large, small, small], 15000)
    assert cuts == [[0, 2, 6816, 220, 0], [2, 3, 3408, 110, 0], [3, 4, 136568, 704, 1200], [4, 6, 6816, 220, 0]]
    assert prob_at == [[0, 0, 0], [3408, 110, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0], [3408, 110, 0]]
    assert chunk_at == [[0, 13632, 14512, 14512], [0, 6816, 7256, 7256], [0, 273136, 275952, 280752], [0, 13632, 14512, 14512]]
    # everything in one chunk under the default; one problem per chunk under a budget of one byte; no problems, no chunks
    assert len(_chunks(lib, [small] * 5, 1 << 30)[0]) == 1 and len(_chunks(lib, [small] * 5, 1)[0]) == 5 and _chunks(lib, [], 1 << 30)[0] == []


def test_no_two_regions_overlap(lib):
    """for lengths around the alignments' parities (cells in fours, words in twos): the problems' regions of a chunk are disjoint, in
    order, aligned (backtrack offsets multiples of 4 cells = 8 bytes, word offsets even), and end inside the chunk's totals"""
    lens = [(m, n) for m in range(1, 10) for n in list(range(1, 10)) + [255, 256, 257, 258, 513]]
    cuts, prob_at, chunk_at = _chunks(lib, lens, 1 << 30)
    assert len(cuts) == 1
    ends = [0, 0, 0]
    for (m, n), at in zip(lens, prob_at):
        need = _need(lib, m, n)
        for i in range(3):
            assert at[i] == ends[i] and at[i] % (4 if i == 0 else 2) == 0
            ends[i] = at[i] + need[i]
    assert ends == cuts[0][2:5]
    assert chunk_at[0] == [0, 2 * ends[0], 2 * ends[0] + 4 * ends[1], 2 * ends[0] + 4 * ends[1] + 4 * ends[2]] and all(v % 8 == 0 for v in chunk_at[0])


def test_slot_layouts(lib):
    """per problem, n = 5 and 2 listed: miss 0 (20 bytes -> 24), counts at 24 (6 words -> 48), their scan at 48 (-> 72), offsets at 72 (20
    -> 96), CIGAR offsets at 96 (6 * 8 -> 144), descriptors at 144 (2 * 32): 208 bytes.  Inputs, a pool of 10 bytes, 3 sequences, 5
    problems: offsets at 16 (4 * 8 -> 48), three index arrays of 20 bytes at 48, 72, 96: 120 bytes"""
    out = (C.c_uint64 * 7)()
    lib.sp_per_problem(5, 2, out)
    assert tuple(out) == (0, 24, 48, 72, 96, 144, 208)
    out = (C.c_uint64 * 6)()
    lib.sp_inputs(10, 3, 5, out)
    assert tuple(out) == (0, 16, 48, 72, 96, 120)


def test_plan_alone_under_the_sanitizers(tmp_path):
    """tests/sw_plan_asan.cpp: the checks, the chunks and the layouts over heap buffers of exactly the planned sizes, every region written
    where the kernels write it.  The sanitizers' runtimes are linked into the program where the compiler has them as archives, so that
    nothing has to stand in front of them in the list of libraries."""
    src = os.path.join(ROOT, "tests", "sw_plan_asan.cpp")
    exe = str(tmp_path / "sw_plan_asan")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src]
    if subprocess.call(cmd + ["-static-libasan", "-static-libubsan"], stderr=subprocess.DEVNULL) != 0:
        subprocess.check_call(cmd)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "sw_plan_asan: ok" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stdout, r.stderr[-2000:])
