"""CPU tests of the duplication-metrics pass's launch plan (elprep_amd/csrc/metrics_plan.hpp, built by the host compiler through
tests/metrics_plan_host.cpp): the sizes a call's arguments fix, the layout of the scratch slots and the host arithmetic behind the
last copy.  A sub-buffer that is a few words short shows on the device only as a silent overlap, so the expected values below are
worked out by hand in the docstrings, not computed from the code.  Every case sits one below or one above a step.  The plan and the
name parser also run on their own under the sanitizers (tests/metrics_plan_asan.cpp).

The rules.  A library row per library of the header plus "Unknown Library"; 7 counters a row.  The counter block, in 64-bit cells:
7 per row | (with histograms) an origin count per row | 3 histograms of hist_len bins per row | per split a pair-read cell per row;
8 cells more are asked for.  k_dup_counters: a 32-bit LDS cell per counter and per (split, row), at most 46 000 B (over it the call is
refused); a workgroup per 1024 records, at most 2048, each taking a multiple of 1024 records.  The loser list holds n / 2 + 8 entries
and is sorted by as many bytes as n has.  k_opt_eval: 128 threads a workgroup, at most 2048; in LDS a cell per row and min(hist_len,
32) bins of 3 histograms per row, or no bins if that is over 32 768 B."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tests", "libmetrics_plan_host.so")

SIZES = ("ncell", "norg", "nhist", "npr", "origins", "hist", "pair_reads", "cells", "block", "lds_refused", "counters_lds", "counters_grid",
         "chunk", "lcap", "ndig", "lds_bins", "eval_lds", "origin_grid", "origin_lds")
LIST = ("words", "pk", "pv", "pk2", "pv2", "head", "gidx", "gstart", "grid")
SETS = ("tp", "words3", "parent", "mset", "linfo", "lcount", "setcnt", "lvals", "lvals_tmp", "lkeys", "lkeys_tmp", "zero", "zero_words",
        "members", "mread", "ginfo", "member_grid", "eval_grid", "cand_grid")


@pytest.fixture(scope="module")
def lib():
    src = os.path.join(ROOT, "tests", "metrics_plan_host.cpp")
    hdr = os.path.join(ROOT, "elprep_amd", "csrc", "metrics_plan.hpp")
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", SO, src])
    return C.CDLL(SO)


def _sizes(L, n, n_lib=1, n_split=1, hist_len=0):
    out = (C.c_uint64 * len(SIZES))()
    L.mx_sizes(C.c_uint64(n), n_lib, n_split, hist_len, out)
    return dict(zip(SIZES, out))


def _list(L, lcap, keys_in_first=True, vals_in_first=True, n_losers=1):
    out = (C.c_uint64 * len(LIST))()
    L.mx_list_scratch(C.c_uint64(lcap), int(keys_in_first), int(vals_in_first), C.c_uint32(n_losers), out)
    return dict(zip(LIST, out))


def _sets(L, total, cl=1):
    out = (C.c_uint64 * len(SETS))()
    L.mx_set_scratch(C.c_uint32(total), C.c_uint32(cl), out)
    return dict(zip(SETS, out))


def _sub(d, **want):
    return {k: d[k] for k in want} == want


# ---- MxSizes

def test_constants(lib):
    """What the kernels take from the header: sets of up to 32 members by one thread, strand lists capped at 300 000, 2048 losers in a
    workgroup's LDS and 1024 records a round, grids of at most 2048, 128 threads and 32 LDS bins in k_opt_eval, the two LDS budgets,
    words 2 (bad name) and 3 (mailbox) of the error block."""
    out = (C.c_uint64 * 11)()
    lib.mx_constants(out)
    assert list(out) == [32, 300000, 2048, 1024, 2048, 128, 32, 46000, 32768, 2, 3]


def test_sizes_of_one_record(lib):
    """n = 1, one library (two rows with "Unknown Library"), one split, no histograms: 2 x 7 = 14 counter cells, no origins, no
    histogram cells, 1 x 2 = 2 pair cells: 16 cells, every part starting where the one before ends (14, 14, 14); 16 + 8 = 24 asked
    for.  LDS: (14 + 2) x 4 = 64 B.  One workgroup of 1024 records.  n / 2 + 8 = 8 list entries, one key byte.  k_opt_eval: no bins,
    2 cells = 8 B; k_origin_count: one workgroup, 8 B."""
    assert _sizes(lib, 1) == dict(ncell=14, norg=0, nhist=0, npr=2, origins=14, hist=14, pair_reads=14, cells=16, block=24, lds_refused=0,
                                  counters_lds=64, counters_grid=1, chunk=1024, lcap=8, ndig=1, lds_bins=0, eval_lds=8, origin_grid=1,
                                  origin_lds=8)


def test_sizes_with_histograms(lib):
    """n = 1000, two libraries (3 rows), two splits, 8 bins: 21 counter cells, 3 origins, 3 x 3 x 8 = 72 histogram cells, 2 x 3 = 6
    pair cells: origins at 21, histograms at 24, pair reads at 96, 102 cells, 110 asked for.  LDS (21 + 6) x 4 = 108 B.
    1000 records: one workgroup of 1024; ceil(1000 / 256) = 4 for the origins.  500 + 8 list entries; 1000 >= 256: two key bytes.
    8 bins in LDS: 3 x (1 + 24) x 4 = 300 B."""
    assert _sizes(lib, 1000, 2, 2, 8) == dict(ncell=21, norg=3, nhist=72, npr=6, origins=21, hist=24, pair_reads=96, cells=102, block=110,
                                              lds_refused=0, counters_lds=108, counters_grid=1, chunk=1024, lcap=508, ndig=2, lds_bins=8,
                                              eval_lds=300, origin_grid=4, origin_lds=12)


def test_no_records(lib):
    """n = 0: the block is still made and read back; no workgroup of anything, and no division by the grid."""
    assert _sub(_sizes(lib, 0), cells=16, block=24, counters_grid=0, chunk=0, lcap=8, ndig=1, origin_grid=0)


def test_counters_grid_and_chunk(lib):
    """1024 records: one workgroup; 1025: two, ceil(1025 / 2) = 513 records each, rounded up to 1024.  2 097 152 = 2048 x 1024: 2048
    workgroups of 1024; one record more: the grid stays at its cap, ceil(n / 2048) = 1025 -> 2048 each.  4 194 304 = 2048 x 2048: 2048
    each; one more: 2049 -> 3072."""
    got = {n: _sizes(lib, n) for n in (1024, 1025, 2097152, 2097153, 4194304, 4194305)}
    assert [(got[n]["counters_grid"], got[n]["chunk"]) for n in sorted(got)] == [(1, 1024), (2, 1024), (2048, 1024), (2048, 2048), (2048, 2048),
                                                                                  (2048, 3072)]
    for n, s in got.items():
        assert s["counters_grid"] * s["chunk"] >= n and s["chunk"] % 1024 == 0


def test_origin_grid(lib):
    """A workgroup per 256 records, at most 2048: 2047 x 256 = 524 032 -> 2047, one more -> 2048; 524 288 = 2048 x 256 -> 2048, one
    more -> still 2048."""
    assert [_sizes(lib, n)["origin_grid"] for n in (256, 257, 524032, 524033, 524288, 524289)] == [1, 2, 2047, 2048, 2048, 2048]


def test_list_sort_digits(lib):
    """The list's keys are record indices below n: one byte up to n = 255, two from 256, three from 65 536, four from 2^24 - never more."""
    ns = (255, 256, 65535, 65536, (1 << 24) - 1, 1 << 24, (1 << 32) - 1)
    assert [_sizes(lib, n)["ndig"] for n in ns] == [1, 2, 2, 3, 3, 4, 4]


def test_list_capacity(lib):
    """n / 2 + 8, the division rounding down: 8 for 0 and 1, 9 for 2 and 3."""
    assert [_sizes(lib, n)["lcap"] for n in (0, 1, 2, 3, 1000001)] == [8, 8, 9, 9, 500008]


def test_lds_refusal(lib):
    """100 rows (99 libraries): 7 + 108 splits = 115 cells a row, 11 500 cells = 46 000 B: fits exactly.  109 splits: 11 600 cells =
    46 400 B: refused."""
    fits, over = _sizes(lib, 1000, 99, 108), _sizes(lib, 1000, 99, 109)
    assert fits["ncell"] + fits["npr"] == 11500 and _sub(fits, counters_lds=46000, lds_refused=0)
    assert over["ncell"] + over["npr"] == 11600 and _sub(over, counters_lds=46400, lds_refused=1)


def test_histogram_lds_bins(lib):
    """min(hist_len, 32) bins, one row: 2 -> 2 bins, (1 + 6) x 4 = 28 B; 31 -> 31, 94 x 4 = 376; 32 -> 32, 97 x 4 = 388; 33 -> 32.
    At 32 bins a row takes 97 words: 84 rows = 32 592 B fit, 85 rows = 32 980 B do not - no bins, a cell per row: 340 B.
    At hist_len 2 a row takes 7 words: 1170 rows = 32 760 B fit, 1171 rows = 32 788 B do not: 4684 B."""
    assert [(_sizes(lib, 10, 0, 1, h)["lds_bins"], _sizes(lib, 10, 0, 1, h)["eval_lds"]) for h in (2, 31, 32, 33)] == [(2, 28), (31, 376), (32, 388),
                                                                                                                     (32, 388)]
    assert _sub(_sizes(lib, 10, 83, 1, 32), lds_bins=32, eval_lds=32592) and _sub(_sizes(lib, 10, 84, 1, 32), lds_bins=0, eval_lds=340)
    assert _sub(_sizes(lib, 10, 1169, 1, 2), lds_bins=2, eval_lds=32760) and _sub(_sizes(lib, 10, 1170, 1, 2), lds_bins=0, eval_lds=4684)
    assert _sub(_sizes(lib, 10, 0, 1, 0), lds_bins=0, eval_lds=4)  # no histograms: no bins


# ---- MxListScratch

def test_list_scratch_of_eight(lib):
    """lcap = 8: 2 x 8 keys of two words at word 0 (the second buffer at 16), 2 x 8 values at word 32 (the second at 40), 48 + 16 = 64
    words.  Sorted into the first halves: heads at 16, group numbers 8 words on at 24, group starts at 40.  Into the second halves:
    0, 8 and 32.  Mixed: the keys' free half and the values' free half are chosen each by its own."""
    assert _list(lib, 8, True, True) == dict(words=64, pk=0, pv=32, pk2=16, pv2=40, head=16, gidx=24, gstart=40, grid=1)
    assert _sub(_list(lib, 8, False, False), head=0, gidx=8, gstart=32)
    assert _sub(_list(lib, 8, True, False), head=16, gidx=24, gstart=32)
    assert _sub(_list(lib, 8, False, True), head=0, gidx=8, gstart=40)
    assert [_list(lib, 1000, n_losers=k)["grid"] for k in (1, 256, 257)] == [1, 1, 2]


# ---- MxSetScratch

def test_set_scratch_rounding(lib):
    """tp = total rounded up to 8: 8 at 1 and 8, 16 at 9.  Slot 3: 12 tp + 16 words = 112 / 208.  At tp = 8: parent 0, mset 8, linfo 16,
    lcount 24, setcnt (64-bit) 32 .. 48, values 48 and 56, keys (64-bit) 64 and 80, end 96.  Zeroed: words 16 .. 48.  total + 4
    elements of slots 2, 4, 5."""
    assert _sets(lib, 1) == dict(tp=8, words3=112, parent=0, mset=8, linfo=16, lcount=24, setcnt=32, lvals=48, lvals_tmp=56, lkeys=64, lkeys_tmp=80,
                                 zero=16, zero_words=32, members=5, mread=5, ginfo=5, member_grid=1, eval_grid=1, cand_grid=1)
    assert _sub(_sets(lib, 8), tp=8, words3=112, members=12) and _sub(_sets(lib, 9), tp=16, words3=208, linfo=32, setcnt=64, lkeys=128, members=13)


def test_set_scratch_grids(lib):
    """A thread per member slot in workgroups of 256; k_opt_eval in workgroups of 128, at most 2048: 2047 x 128 = 262 016 -> 2047,
    262 144 -> 2048, one more -> 2048.  A thread per candidate."""
    assert [_sets(lib, t)["member_grid"] for t in (256, 257)] == [1, 2]
    assert [_sets(lib, t)["eval_grid"] for t in (128, 129, 262016, 262017, 262144, 262145)] == [1, 2, 2047, 2048, 2048, 2048]
    assert [_sets(lib, 1000, cl)["cand_grid"] for cl in (1, 256, 257)] == [1, 1, 2]


# ---- containment

STEP_NS = (2, 3, 16, 17, 255, 256, 1024, 1025, 65535, 65536, 2097152, 2097153, (1 << 24) - 1, 1 << 24)


def _inside(a, n, lo, hi):
    return lo <= a and a + n <= hi


def _disjoint(a, na, b, nb):
    return a + na <= b or b + nb <= a


@pytest.mark.parametrize("n", STEP_NS)
def test_groups_lie_in_the_free_halves(lib, n):
    """head (L words), gidx (L) and gstart (G + 1) for every pair of halves the sort can leave its result in, L = 1 and n / 2 (every
    pair a loser), G = 1 and L: inside the slot, inside the half that is free, off the halves that hold the sorted list, off each other."""
    lcap = _sizes(lib, n)["lcap"]
    for kf in (True, False):
        for vf in (True, False):
            s = _list(lib, lcap, kf, vf)
            live_k = s["pk"] if kf else s["pk2"]
            free_k = s["pk2"] if kf else s["pk"]
            live_v = s["pv"] if vf else s["pv2"]
            free_v = s["pv2"] if vf else s["pv"]
            assert {s["pk"], s["pk2"]} == {0, 2 * lcap} and {s["pv"], s["pv2"]} == {4 * lcap, 5 * lcap}
            for L in sorted({1, n // 2}):
                for G in sorted({1, L}):
                    arrays = [(s["head"], L), (s["gidx"], L), (s["gstart"], G + 1)]
                    for a, na in arrays:
                        assert _inside(a, na, 0, s["words"]), (n, kf, vf, L, G)
                        assert _disjoint(a, na, live_k, 2 * lcap) and _disjoint(a, na, live_v, lcap), (n, kf, vf, L, G)
                    assert _inside(s["head"], L, free_k, free_k + 2 * lcap) and _inside(s["gidx"], L, free_k, free_k + 2 * lcap)
                    assert _inside(s["gstart"], G + 1, free_v, free_v + lcap), (n, kf, vf, L, G)
                    assert _disjoint(s["head"], L, s["gidx"], L)


@pytest.mark.parametrize("total", [1, 2, 7, 8, 9, 15, 16, 17, 255, 256, 257, 262144, 262145, 3 * (1 << 23)])
def test_slot_three_arrays(lib, total):
    """The seven arrays one behind the other at their element widths (setcnt and the keys 64-bit), the sort's second buffers behind the
    first, everything inside the slot, 64-bit arrays on 8-byte boundaries; the zeroed range is linfo, lcount and setcnt, no more."""
    s = _sets(lib, total)
    tp = s["tp"]
    assert tp >= total and tp - total < 8 and tp % 8 == 0
    order = [("parent", tp), ("mset", tp), ("linfo", tp), ("lcount", tp), ("setcnt", 2 * tp), ("lvals", tp), ("lvals_tmp", tp), ("lkeys", 2 * tp),
             ("lkeys_tmp", 2 * tp)]
    at = 0
    for name, words in order:
        assert s[name] == at, name
        at += words
    assert at <= s["words3"]
    for name in ("setcnt", "lkeys", "lkeys_tmp"):
        assert (4 * s[name]) % 8 == 0
    assert s["zero"] == s["linfo"] and s["zero"] + s["zero_words"] == s["lvals"]
    assert s["members"] >= total and s["mread"] >= total and s["ginfo"] >= total


# ---- mx_finish

def _finish(L, n_lib, n_split, hist_len, block):
    counters = np.zeros((n_lib + 1, 7), np.int64)
    hist = np.zeros((n_lib + 1, 3, max(hist_len, 1)), np.int64)
    L.mx_finish_block(C.c_uint64(100), n_lib, n_split, hist_len, block.ctypes.data_as(C.c_void_p), counters.ctypes.data_as(C.c_void_p),
                      hist.ctypes.data_as(C.c_void_p) if hist_len else None)
    return counters, hist


def _block(L, n_lib, n_split, hist_len, ctr, pair_reads, origins=None, hist=None):
    s = _sizes(L, 100, n_lib, n_split, hist_len)
    b = np.zeros(s["cells"], np.uint64)
    b[:s["ncell"]] = np.asarray(ctr, np.uint64).reshape(-1)
    b[s["pair_reads"]:s["pair_reads"] + s["npr"]] = np.asarray(pair_reads, np.uint64).reshape(-1)
    if hist_len:
        b[s["origins"]:s["origins"] + s["norg"]] = origins
        b[s["hist"]:s["hist"] + s["nhist"]] = np.asarray(hist, np.uint64).reshape(-1)
    return b


CTR = [[100 * l + k + 1 for k in range(7)] for l in range(3)]  # row l: 100 l + 1 .. 100 l + 7; cell 1 is replaced by the pairs
PAIR_READS = [[3, 4, 1], [5, 4, 1], [0, 2, 1]]                 # [split][row]


def _want_counters():
    """Pairs: the reads of every split halved, then summed.  Row 0: 3 // 2 + 5 // 2 + 0 = 1 + 2 + 0 = 3 (not 8 // 2 = 4).  Row 1:
    2 + 2 + 1 = 5.  Row 2 ("Unknown Library"): 1 // 2 three times = 0 (not 3 // 2 = 1)."""
    want = np.array(CTR, np.int64)
    want[:, 1] = [3, 5, 0]
    return want


def test_finish_without_histograms(lib):
    """Two libraries + unknown, three splits: the counters as read back, ReadPairsExamined halved split by split."""
    counters, _ = _finish(lib, 2, 3, 0, _block(lib, 2, 3, 0, CTR, PAIR_READS))
    assert np.array_equal(counters, _want_counters())


def test_finish_with_eight_bins(lib):
    """Row 0 has 10 origins and 3 + 2 + 1 = 6 sets with duplicates (bins 2, 3 and the last of the first histogram): 4 origins stand
    alone and join bin 1 of the first histogram (0 + 4) and of the second (1 + 4 = 5); the third is untouched.  Row 1 has 4 origins,
    all 4 with duplicates: nothing is added.  Row 2 has nothing at all."""
    hist = np.zeros((3, 3, 8), np.uint64)
    hist[0, 0, [2, 3, 7]] = [3, 2, 1]
    hist[0, 1, [1, 2, 3, 7]] = [1, 2, 2, 1]
    hist[0, 2, 2] = 1
    hist[1, 0, 2] = 4
    hist[1, 1, 2] = 4
    counters, out = _finish(lib, 2, 3, 8, _block(lib, 2, 3, 8, CTR, PAIR_READS, [10, 4, 0], hist))
    assert np.array_equal(counters, _want_counters())
    want = hist.astype(np.int64)
    want[0, 0, 1] = 4
    want[0, 1, 1] = 5
    assert np.array_equal(out, want)


def test_finish_with_two_bins(lib):
    """hist_len 2: bin 1 is also the overflow bin, so it holds all 6 sets of row 0 already; the 4 lone origins are added on top: 10 in
    the first histogram, 6 + 4 = 10 in the second.  Row 1: 4 origins, 4 sets: unchanged."""
    hist = np.zeros((3, 3, 2), np.uint64)
    hist[0, :, 1] = [6, 6, 1]
    hist[1, :, 1] = [4, 4, 0]
    _, out = _finish(lib, 2, 3, 2, _block(lib, 2, 3, 2, CTR, PAIR_READS, [10, 4, 0], hist))
    want = hist.astype(np.int64)
    want[0, 0, 1] = 10
    want[0, 1, 1] = 10
    assert np.array_equal(out, want)


# ---- sanitizers

def test_plan_and_name_parser_under_the_sanitizers(tmp_path):
    """tests/metrics_plan_asan.cpp: the plan's edge cases with every block at exactly its size, and the name parser over buffers that
    end with the name.  The sanitizers' runtimes are linked into the program where the compiler has them as archives, so that nothing
    has to stand in front of them in the list of libraries."""
    src = os.path.join(ROOT, "tests", "metrics_plan_asan.cpp")
    exe = str(tmp_path / "metrics_plan_asan")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src]
    if subprocess.call(cmd + ["-static-libasan", "-static-libubsan"], stderr=subprocess.DEVNULL) != 0:
        subprocess.check_call(cmd)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "metrics_plan_asan: ok" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (
        r.returncode, r.stdout, r.stderr[-2000:])
