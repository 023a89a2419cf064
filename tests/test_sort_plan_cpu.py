"""CPU tests of the sorts' plan (elprep_amd/csrc/sort_plan.hpp, built by the host compiler through tests/sort_plan_host.cpp): the key
format, the long runs' bounds, the layout of the scratch slots on the sort's lane, the rank tables and the packing of the rounds' keys.
A width that is one bit short or a sub-buffer that is a few words short shows on the device only as a wrong order in a rare input or a
silent overlap, so the expected values below are worked out by hand in the docstrings, not computed from the code.  Every case sits one
below or one above a step.  The plan also runs on its own under the sanitizers (tests/sort_plan_asan.cpp).

The rules.  Index bits of n records: the least b >= 1 with n >> b == 0, at most 32.  The passes move words key << b | index where
key_bits >= 1, key_bits + b <= 64 and the tuning key sort_pairs is not 1.  The key: contig code (0 .. n_ref + 1) | POS | strand.
A run of more than 48 (TIE_SMALL) equal keys is long; its bounds come in two lists of bounds_cap(n) = min(n / 48 + 16, n + 2) words,
256 (TIE_HEAD) of each with the first read-back.  A rank takes the least b >= 1 bits with 2^b >= the number of values."""
import ctypes as C
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tests", "libsort_plan_host.so")

SORT = ("keys", "vals", "flags", "cap", "starts", "ends")
TIE = ("m_bytes", "rw", "use_rows", "u_pos", "u_read", "u_seg", "uv0", "uv1", "d_start", "d_first", "u_words", "words3",
       "uk0", "uk1", "words4", "d_vals", "d_lut", "words5")
QN = ("vwords", "d_over", "d_lut", "lut_words", "words3")
QN_STATE, QN_LEN = 0xFFFF, 0xFFFE


@pytest.fixture(scope="module")
def lib():
    src = os.path.join(ROOT, "tests", "sort_plan_host.cpp")
    hdr = os.path.join(ROOT, "elprep_amd", "csrc", "sort_plan.hpp")
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", SO, src])
    L = C.CDLL(SO)
    L.sp_index_bits.argtypes = L.sp_bounds_cap.argtypes = L.sp_rank_keys_apply.argtypes = [C.c_uint64]
    L.sp_bounds_cap.restype = L.sp_bounds_head.restype = C.c_uint32
    L.sp_key_width.argtypes = [C.c_uint32, C.c_int32, C.c_void_p]
    L.sp_sort_scratch.argtypes = [C.c_uint64, C.c_void_p]
    L.sp_byte_cuts.argtypes = [C.c_uint64, C.c_void_p]
    for name in ("sp_bounds_head", "sp_bounds_in_head", "sp_segbits"):
        getattr(L, name).argtypes = [C.c_uint32]
    L.sp_run_counts_ok.argtypes = [C.c_uint32] * 3
    return L


def _key_width(L, max_pos, n_ref):
    out = (C.c_int * 3)()
    L.sp_key_width(max_pos, n_ref, out)
    return tuple(out)


def _long_runs(L, starts, ends):
    s, e = (C.c_uint32 * len(starts))(*starts), (C.c_uint32 * len(ends))(*ends)
    so, fo, cnt = (C.c_uint32 * len(starts))(), (C.c_uint32 * (len(starts) + 1))(), (C.c_uint32 * 2)()
    if not L.sp_long_runs(s, len(starts), e, len(ends), so, fo, cnt):
        return None
    return list(so), list(fo), cnt[0], cnt[1]


def _struct(fn, names, *args):
    out = (C.c_uint64 * len(names))()
    fn(*args, out)
    return dict(zip(names, out))


def _set(values):
    w = [0] * 8
    for v in values:
        w[v >> 5] |= 1 << (v & 31)
    return w


def _fields(fn, sets, nfields_max, args):
    """-> pos, slot, bits, lut rows (lists of 256)"""
    sw = (C.c_uint32 * len(sets))(*sets)
    pos, slot, bits = (C.c_uint16 * nfields_max)(), (C.c_uint16 * nfields_max)(), (C.c_int * nfields_max)()
    lut, rows = (C.c_uint8 * (256 * nfields_max))(), C.c_int()
    n = fn(*args(sw), pos, slot, bits, lut, C.byref(rows))
    return list(pos[:n]), list(slot[:n]), list(bits[:n]), [list(lut[256 * r:256 * r + 256]) for r in range(rows.value)]


def _tie_fields(L, lp, sets):
    lpa = (C.c_uint16 * len(lp))(*lp)
    return _fields(L.sp_tie_fields, sets, max(1, len(lp)), lambda sw: (lpa, len(lp), sw))


def _qn_fields(L, sets, maxq, any_not_output):
    return _fields(L.sp_qn_fields, sets, maxq + 2, lambda sw: (sw, maxq, int(any_not_output)))


def _prefix(L, bits, reserved):
    out = (C.c_int * 3)()
    L.sp_pack_prefix((C.c_int * len(bits))(*bits), len(bits), reserved, out)
    return tuple(out)


def _lsd(L, bits):
    out = (C.c_int * (3 * max(1, len(bits))))()
    n = L.sp_lsd_cuts((C.c_int * len(bits))(*bits), len(bits), out)
    return [tuple(out[3 * k:3 * k + 3]) for k in range(n)]


def _shifts(L, bits, cut):
    out = (C.c_uint8 * (cut[1] - cut[0]))()
    L.sp_field_shifts((C.c_int * len(bits))(*bits), len(bits), cut[0], cut[1], cut[2], out)
    return list(out)


# ---- key format

def test_constants(lib):
    """what the kernels and the plan share: runs up to 48 records are ranked by comparison, 256 bounds come with the first read-back,
    rank keys for up to 96 live positions; the queryname key's two fields that are no byte position."""
    out = (C.c_int * 5)()
    lib.sp_constants(out)
    assert list(out) == [48, 256, 96, 0xFFFF, 0xFFFE]


def test_index_bits(lib):
    """n = 1: 1 >> 1 = 0 -> 1 bit (never 0).  2 = 0b10 and 3: 2 bits; 4: 3.  2^k - 1 has k bits, 2^k has k + 1: 65535 -> 16, 65536 -> 17,
    2^31 - 1 -> 31, 2^31 -> 32.  2^32 - 1 -> 32, and the loop stops there whatever n (2^32: 32)."""
    got = [lib.sp_index_bits(n) for n in (1, 2, 3, 4, 65535, 65536, (1 << 31) - 1, 1 << 31, (1 << 32) - 1, 1 << 32)]
    assert got == [1, 2, 2, 3, 16, 17, 31, 32, 32, 32]


def test_words_or_pairs(lib):
    """A key of 40 bits: 2^24 - 1 records have 24 index bits, 40 + 24 = 64 -> words; 2^24 records have 25: 65 -> pairs.  sort_pairs = 1
    forces pairs, 2 (or anything else) does not.  A key of no bits at all: pairs."""
    ib = [lib.sp_index_bits(n) for n in ((1 << 24) - 1, 1 << 24)]
    assert ib == [24, 25]
    assert [lib.sp_sort_words(40, b, 0) for b in ib] == [1, 0]
    assert [lib.sp_sort_words(40, 24, sp) for sp in (0, 1, 2)] == [1, 0, 1]
    assert lib.sp_sort_words(0, 24, 0) == 0 and lib.sp_sort_words(1, 24, 0) == 1


def test_key_width(lib):
    """POS: max_pos 0 and 1 -> 1 bit (never 0), 2 -> 2, 2^31 - 1 -> 31, 2^32 - 1 (POS -1 as staged) -> 32.  Contig codes 0 .. n_ref + 1,
    the width is that of n_ref + 1: n_ref 0 -> 1 -> 1 bit; 1 -> 2 -> 2 bits (codes 0, 1, 2); 2 -> 3 -> 2 bits (0 .. 3); 3 -> 4 -> 3 bits;
    65535 -> 65536 -> 17 bits.  key_bits = both + 1 for the strand."""
    assert [_key_width(lib, p, 0) for p in (0, 1, 2, (1 << 31) - 1, (1 << 32) - 1)] == [(1, 1, 3), (1, 1, 3), (2, 1, 4), (31, 1, 33), (32, 1, 34)]
    assert [_key_width(lib, 0, r) for r in (0, 1, 2, 3, 65535)] == [(1, 1, 3), (1, 2, 4), (1, 2, 4), (1, 3, 5), (1, 17, 19)]
    assert _key_width(lib, (1 << 31) - 1, 65535) == (31, 17, 49)


# ---- long runs

def test_bounds_cap_and_first_copy(lib):
    """min(n / 48 + 16, n + 2): n = 1 -> 3; 13 -> 15; 14 and 15 -> 16 (the two arms cross); 47 -> 16, 48 -> 17; 13000 -> 270 + 16 = 286.
    The first read-back brings min(256, cap) bounds of each list, and holds all of them for up to 256 runs."""
    assert [lib.sp_bounds_cap(n) for n in (1, 13, 14, 15, 47, 48, 13000)] == [3, 15, 16, 16, 16, 17, 286]
    assert [lib.sp_bounds_head(c) for c in (3, 255, 256, 257, 286)] == [3, 255, 256, 256, 256]
    assert [lib.sp_bounds_in_head(nr) for nr in (0, 1, 256, 257)] == [1, 1, 1, 0]


def test_run_counts(lib):
    """as many starts as ends, and no more than the lists hold (a count past the lists' end means bounds were dropped)"""
    assert [lib.sp_run_counts_ok(*a) for a in ((0, 0, 3), (3, 3, 3), (3, 2, 8), (2, 3, 8), (4, 4, 3))] == [1, 1, 0, 0, 0]


def test_segbits(lib):
    """run ids 1 .. nr: one run needs no id; 2 runs: ids 1, 2 = 0b10 -> 2 bits; 3 -> 2; 4 = 0b100 -> 3; 255 -> 8; 256 and 257 -> 9."""
    assert [lib.sp_segbits(nr) for nr in (0, 1, 2, 3, 4, 255, 256, 257)] == [0, 0, 2, 2, 3, 8, 9, 9]


def test_long_runs_sorted_and_numbered(lib):
    """No run: nothing, first = [0].  One run [100, 149]: 50 members.  Three runs given shuffled - starts 300, 10, 120, ends 199, 349, 59 -
    pair up as [10, 59], [120, 199], [300, 349]: 50, 80 and 50 members, first = 0, 50, 130, 180.  Adjacent runs [10, 59], [60, 100] are in
    order (50 + 41 members).  A run of one position is not refused here."""
    assert _long_runs(lib, [], []) == ([], [0], 0, 0)
    assert _long_runs(lib, [100], [149]) == ([100], [0, 50], 1, 50)
    assert _long_runs(lib, [300, 10, 120], [199, 349, 59]) == ([10, 120, 300], [0, 50, 130, 180], 3, 180)
    assert _long_runs(lib, [60, 10], [59, 100]) == ([10, 60], [0, 50, 91], 2, 91)
    assert _long_runs(lib, [7], [7]) == ([7], [0, 1], 1, 1)


def test_long_runs_at_the_first_copys_size(lib):
    """256 and 257 runs of 49 records, run r = [100 r, 100 r + 48], starts given last first and ends rotated: 256 x 49 = 12544 and
    257 x 49 = 12593 members, first[r] = 49 r."""
    for nr in (256, 257):
        starts = [100 * r for r in reversed(range(nr))]
        ends = [100 * ((r + 5) % nr) + 48 for r in range(nr)]
        s, f, got_nr, nu = _long_runs(lib, starts, ends)
        assert (got_nr, nu) == (nr, 49 * nr) and s == [100 * r for r in range(nr)] and f == [49 * r for r in range(nr + 1)]


def test_long_runs_refused(lib):
    """an end before its start; a start at the previous end, and before it; unequal counts"""
    assert _long_runs(lib, [10], [9]) is None
    assert _long_runs(lib, [10, 59], [59, 100]) is None
    assert _long_runs(lib, [10, 40], [59, 100]) is None
    assert _long_runs(lib, [10, 60], [59]) is None and _long_runs(lib, [10], [59, 100]) is None


# ---- layout

def test_sort_scratch_by_hand(lib):
    """n = 1000: three slots of 2 n + 8 = 2008 elements; cap = min(20 + 16, 1002) = 36: starts at word 4, ends at 40.  n = 1: slots of
    10, cap 3, ends at 7, the lists end at word 10 = the slot's end exactly."""
    assert _struct(lib.sp_sort_scratch, SORT, 1000) == dict(keys=2008, vals=2008, flags=2008, cap=36, starts=4, ends=40)
    assert _struct(lib.sp_sort_scratch, SORT, 1) == dict(keys=10, vals=10, flags=10, cap=3, starts=4, ends=7)


def test_bounds_lie_inside_their_slot(lib):
    """the four counters, then two lists of cap words: inside 2 n + 8 words for every n, with no room to spare up to n = 14"""
    for n in (1, 2, 13, 14, 15, 47, 48, 49, 1000, 13000, (1 << 32) - 1):
        s = _struct(lib.sp_sort_scratch, SORT, n)
        assert s["starts"] == 4 and s["starts"] + s["cap"] <= s["ends"] and s["ends"] + s["cap"] <= s["flags"], n
        assert s["keys"] >= 2 * n and s["vals"] >= 2 * n, n


def test_tie_scratch_by_hand(lib):
    """nu = 100 members of nr = 3 runs, names up to 20 bytes: strings of 35 bytes in rows of (20 + 30) & ~15 = 48.  Slot 3: five arrays of
    100 words, d_start at 500 (3 words), d_first at 503 (4 words, to 507); (500 + 6 + 64 + 3) & ~3 = 572 words, then 4800 bytes of rows:
    (4800 + 64) / 4 = 1216 -> 1788 words.  Slot 4: two halves of 100 keys, 216.  Slot 5: 96 sets of 8 words, the LUT at word 768, 96 x 64
    words of it + 64 = 6976."""
    assert _struct(lib.sp_tie_scratch, TIE, 100, 3, 20) == dict(
        m_bytes=35, rw=48, use_rows=1, u_pos=0, u_read=100, u_seg=200, uv0=300, uv1=400, d_start=500, d_first=503, u_words=572, words3=1788,
        uk0=0, uk1=100, words4=216, d_vals=0, d_lut=768, words5=6976)


def test_row_width_steps(lib):
    """rw = (maxq + 30) & ~15 against a string of maxq + 15 bytes: maxq 0 -> 15 bytes in 16; 1 -> 16 in 16; 2 -> 17 in 32; 17 -> 32 in 32;
    18 -> 33 in 48; 1000 -> 1015 in 1024."""
    got = [(t["m_bytes"], t["rw"]) for t in (_struct(lib.sp_tie_scratch, TIE, 50, 1, q) for q in (0, 1, 2, 17, 18, 1000))]
    assert got == [(15, 16), (16, 16), (17, 32), (32, 32), (33, 48), (1015, 1024)]


def test_tie_scratch_holds_its_sub_buffers(lib):
    """around the steps of the alignment (5 nu + 2 nr + 67 rounded down to four words; rows of 16 bytes): every sub-buffer of slot 3
    ends where the next begins or before, the two lists of run bounds fit before word u_words, the rows - which the kernels read eight
    bytes at a time - begin on a 16-byte boundary and end inside the slot; slot 4 holds two halves of nu keys; slot 5 holds 96 value
    sets and 96 LUT rows of 256 bytes."""
    for maxq in (0, 1, 2, 17, 18, 255, 1000):
        for nu in (49, 50, 51, 52, 97, 1000, 1001):
            for nr in (1, 2, 3, 4, 5):
                t = _struct(lib.sp_tie_scratch, TIE, nu, nr, maxq)
                where = (maxq, nu, nr)
                parts = ("u_pos", "u_read", "u_seg", "uv0", "uv1", "d_start")
                for a, b in zip(parts, parts[1:]):
                    assert t[a] + nu <= t[b], (where, a, b)
                assert t["d_start"] + nr <= t["d_first"] and t["d_first"] + nr + 1 <= t["u_words"], where
                assert t["u_words"] % 4 == 0 and t["rw"] % 16 == 0 and t["rw"] >= t["m_bytes"], where
                assert t["use_rows"] == 1 and 4 * t["u_words"] + nu * t["rw"] <= 4 * t["words3"], where
                assert t["uk0"] + nu <= t["uk1"] and t["uk1"] + nu <= t["words4"], where
                assert t["d_vals"] + 96 * 8 <= t["d_lut"] and 4 * t["d_lut"] + 96 * 256 <= 4 * t["words5"], where


def test_rows_up_to_512_mib(lib):
    """rows of 16 bytes (maxq = 1): 2^29 / 16 = 33554432 members are written out, one more are not - slot 3 then ends with the run
    bounds.  Rows of 1024 bytes (maxq = 994): 524288 and 524289 members."""
    for maxq, rw, nu in ((1, 16, 1 << 25), (994, 1024, 1 << 19)):
        at, over = _struct(lib.sp_tie_scratch, TIE, nu, 1, maxq), _struct(lib.sp_tie_scratch, TIE, nu + 1, 1, maxq)
        assert (at["rw"], at["use_rows"], over["use_rows"]) == (rw, 1, 0)
        assert at["words3"] == at["u_words"] + (nu * rw + 64) // 4 and over["words3"] == over["u_words"]


def test_queryname_scratch(lib):
    """maxq = 20: 160 words of value sets and the NUL word = 161; the overflow word at 161; the LUT at word 162, 20 x 256 bytes = 1280
    words: 1442.  No names at all: the NUL word, the overflow word, no LUT.  maxq = 1: 9, 9, 10, 64, 74.  1000: 8001 | 8001 | 8002, 64000."""
    assert _struct(lib.sp_qn_scratch, QN, 20) == dict(vwords=161, d_over=161, d_lut=162, lut_words=1280, words3=1442)
    assert _struct(lib.sp_qn_scratch, QN, 0) == dict(vwords=1, d_over=1, d_lut=2, lut_words=0, words3=2)
    assert _struct(lib.sp_qn_scratch, QN, 1) == dict(vwords=9, d_over=9, d_lut=10, lut_words=64, words3=74)
    assert _struct(lib.sp_qn_scratch, QN, 1000) == dict(vwords=8001, d_over=8001, d_lut=8002, lut_words=64000, words3=72002)


# ---- rank tables

def test_rank_widths(lib):
    """1, 2, 3, 4, 5, 128, 129, 256 values -> 1, 1, 2, 2, 3, 7, 8, 8 bits (a single value gets one bit)"""
    assert [lib.sp_rank_bits(v) for v in (1, 2, 3, 4, 5, 128, 129, 256)] == [1, 1, 2, 2, 3, 7, 8, 8]
    for count, width in ((1, 1), (2, 1), (3, 2), (4, 2), (5, 3), (128, 7), (129, 8), (256, 8)):
        values = [(255 + 101 * k) % 256 for k in range(count)]  # (101 is odd: distinct values)
        row = (C.c_uint8 * 256)()
        s = (C.c_uint32 * 8)(*_set(values))
        assert lib.sp_value_count(s) == count and lib.sp_rank_row(s, row) == count
        assert [row[v] for v in sorted(values)] == list(range(count))
        assert lib.sp_rank_bits(count) == width


def test_lut_rows_are_ranks_in_byte_order(lib):
    """'0' = 0x30, 'A' = 0x41, 'C' = 0x43 at a position: ranks 0, 1, 2; every other byte maps to 0.  A second position with 0x00 and
    0xFF: ranks 0 and 1.  Slots number the positions in order; widths 2 and 1."""
    pos, slot, bits, rows = _tie_fields(lib, [5, 9], _set([0x43, 0x30, 0x41]) + _set([0xFF, 0x00]))
    assert (pos, slot, bits) == ([5, 9], [0, 1], [2, 1])
    want = [0] * 256
    want[0x41], want[0x43] = 1, 2
    assert rows[0] == want and rows[1] == [0] * 255 + [1]


def test_live_positions(lib):
    """bits 0, 31, 32 and 40 of the bitmap with strings of 40 bytes: positions 0, 31, 32 (bit 40 lies behind the string); of 41: and 40"""
    live = (C.c_uint32 * 32)()
    live[0], live[1] = (1 << 31) | 1, (1 << 8) | 1
    out = (C.c_uint16 * 64)()
    assert list(out[:lib.sp_live_positions(live, 40, out)]) == [0, 31, 32]
    assert list(out[:lib.sp_live_positions(live, 41, out)]) == [0, 31, 32, 40]
    assert [lib.sp_rank_keys_apply(n) for n in (0, 1, 96, 97)] == [0, 1, 1, 0]


def test_queryname_fields(lib):
    """names up to 3 bytes: position 0 holds 'A' and 'B', position 1 only 'A' (one value: not live), position 2 a padding 0 and 'x'.
    No record held back, no NUL: positions 0 and 2 with slots 0 and 1, one bit each.  Records that are not output: the state in front,
    one bit.  A NUL inside a name: the length behind, 11 bits."""
    sets = _set([0x41, 0x42]) + _set([0x41]) + _set([0, 0x78])
    assert _qn_fields(lib, sets + [0], 3, False)[:3] == ([0, 2], [0, 1], [1, 1])
    assert _qn_fields(lib, sets + [0], 3, True)[:3] == ([QN_STATE, 0, 2], [0, 0, 1], [1, 1, 1])
    pos, slot, bits, rows = _qn_fields(lib, sets + [1], 3, True)
    assert (pos, slot, bits) == ([QN_STATE, 0, 2, QN_LEN], [0, 0, 1, 0], [1, 1, 1, 11])
    assert len(rows) == 2 and rows[0][0x42] == 1 and rows[1][0x78] == 1 and sum(rows[0]) == 1 and sum(rows[1]) == 1
    assert _qn_fields(lib, [0], 0, True)[:3] == ([QN_STATE], [0], [1]) and _qn_fields(lib, [0], 0, False)[:3] == ([], [], [])


# ---- packing

def test_prefix_that_fits(lib):
    """eight fields of 8 bits fill 64 exactly; a ninth of one bit does not fit; 7 x 8 + 7 = 63 leaves no room for 2 more.  70 one-bit
    fields: 64 of them.  One reserved bit: seven of the eight.  Fields 3, 5, 2 beside 59 reserved bits: 62, then 67 - the first only;
    beside 61: 64 - still the first; beside 62: none."""
    assert _prefix(lib, [8] * 8, 0) == (0, 8, 64)
    assert _prefix(lib, [8] * 8 + [1], 0) == (0, 8, 64)
    assert _prefix(lib, [8] * 7 + [7, 2], 0) == (0, 8, 63)
    assert _prefix(lib, [1] * 70, 0) == (0, 64, 64)
    assert _prefix(lib, [8] * 8, 1) == (0, 7, 56)
    assert [_prefix(lib, [3, 5, 2], r) for r in (59, 61, 62)] == [(0, 1, 3), (0, 1, 3), (0, 0, 0)]
    assert _prefix(lib, [], 0) == (0, 0, 0)


def test_key_then_compare_round(lib):
    """taken unless tie_rounds = 1.  Its second condition - the run id and the first rank fit 64 bits - is pinned as the code has it:
    56 + 8 fits, 57 + 8 does not; a run id has at most 27 bits (n / 48 + 16 < 2^27 runs), so it never fails."""
    assert [lib.sp_key_then_compare(*a) for a in ((0, 27, 8), (2, 0, 1), (1, 27, 8), (0, 56, 8), (0, 57, 8))] == [1, 1, 0, 1, 0]


def test_lsd_cuts(lib):
    """from the least significant field up.  Ten fields of 8: the last eight (64 bits), then the first two (16).  Eight of 8 and a last
    one of 1: 1 + 7 x 8 = 57 takes fields 1 .. 8 (an eighth 8 would make 65), then field 0 alone.  70 one-bit fields: 64 and 6.  None:
    no round."""
    assert _lsd(lib, [8] * 10) == [(2, 10, 64), (0, 2, 16)]
    assert _lsd(lib, [8] * 8 + [1]) == [(1, 9, 57), (0, 1, 8)]
    assert _lsd(lib, [1] * 70) == [(6, 70, 64), (0, 6, 6)]
    assert _lsd(lib, [5]) == [(0, 1, 5)] and _lsd(lib, []) == []


def test_shifts_and_digits(lib):
    """fields 3, 5, 2 in one key of 10 bits: at bits 7, 2, 0; the last two alone (7 bits): 2, 0.  Radix passes of 8 bits: 0 -> 0, 1 .. 8
    -> 1, 9 -> 2, 64 -> 8."""
    assert _shifts(lib, [3, 5, 2], (0, 3, 10)) == [7, 2, 0]
    assert _shifts(lib, [3, 5, 2], (1, 3, 7)) == [2, 0]
    assert [lib.sp_key_digits(b) for b in (0, 1, 8, 9, 63, 64)] == [0, 1, 1, 2, 8, 8]


def test_byte_rounds(lib):
    """97 positions, eight per round from the last: [89, 97), [81, 89), ... [1, 9), then [0, 1): 13 rounds, 64 bits each but the last (8).
    8 positions: one round; none: none."""
    out = (C.c_int * (3 * 16))()
    n = lib.sp_byte_cuts(97, out)
    cuts = [tuple(out[3 * k:3 * k + 3]) for k in range(n)]
    assert cuts == [(97 - 8 * k - 8, 97 - 8 * k, 64) for k in range(12)] + [(0, 1, 8)]
    assert lib.sp_byte_cuts(8, out) == 1 and tuple(out[:3]) == (0, 8, 64) and lib.sp_byte_cuts(0, out) == 0


# ---- the plan's keys order strings as the strings themselves

def test_keys_order_like_the_strings(lib):
    """300 random cases: strings of random bytes from a random alphabet per position (some positions constant).  From the value sets the
    plan gives positions, LUT and widths.  (a) The key of the longest prefix that fits beside `reserved` bits, built here from (position,
    LUT row, shift), orders the strings exactly as their bytes at those positions do.  (b) Stable sorts over the LSD cuts, least
    significant first, leave the strings in the order of one stable sort on the whole string."""
    rng = random.Random(20240611)
    multi = 0
    for case in range(300):
        length, count = rng.randrange(1, 48), rng.randrange(2, 40)
        alphabets = [rng.sample(range(256), rng.choice((1, 1, 2, 3, 4, 5, 9, 17, 200))) for _ in range(length)]
        strings = [bytes(rng.choice(a) for a in alphabets) for _ in range(count)]
        lp = [j for j in range(length) if len({s[j] for s in strings}) > 1]
        if not lp:
            continue
        sets = sum((_set({s[j] for s in strings}) for j in lp), [])
        pos, slot, bits, rows = _tie_fields(lib, lp, sets)
        assert pos == lp and slot == list(range(len(lp)))

        def key(s, cut):
            sh = _shifts(lib, bits, cut)
            return sum(rows[slot[k]][s[pos[k]]] << sh[k - cut[0]] for k in range(cut[0], cut[1]))

        reserved = rng.choice((0, 1, 9, 27))
        cut = _prefix(lib, bits, reserved)
        assert cut[2] + reserved <= 64 and (cut[1] == len(bits) or cut[2] + reserved + bits[cut[1]] > 64 or cut[1] == 64)
        by_key = sorted(range(count), key=lambda i: key(strings[i], cut))
        by_bytes = sorted(range(count), key=lambda i: bytes(strings[i][p] for p in pos[:cut[1]]))
        assert by_key == by_bytes, case
        assert all(key(s, cut) < (1 << max(1, cut[2])) for s in strings), case
        cuts = _lsd(lib, bits)
        assert cuts[0][1] == len(bits) and cuts[-1][0] == 0 and all(a[0] == b[1] for a, b in zip(cuts, cuts[1:])), case
        multi += len(cuts) > 1
        order = list(range(count))
        for c in cuts:
            assert c[2] <= 64 and c[1] - c[0] <= 64, case
            order.sort(key=lambda i: key(strings[i], c))
        assert order == sorted(range(count), key=lambda i: strings[i]), case
    assert multi >= 30  # (cases that need more than one round are not rare here)


# ---- under the sanitizers

def test_plan_alone_under_the_sanitizers(tmp_path):
    """tests/sort_plan_asan.cpp: the edge cases above with every array at exactly its size.  The sanitizers' runtimes are linked into the
    program where the compiler has them as archives, so that nothing has to stand in front of them in the list of libraries."""
    src = os.path.join(ROOT, "tests", "sort_plan_asan.cpp")
    exe = str(tmp_path / "sort_plan_asan")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src]
    if subprocess.call(cmd + ["-static-libasan", "-static-libubsan"], stderr=subprocess.DEVNULL) != 0:
        subprocess.check_call(cmd)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "sort_plan_asan: ok" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stdout, r.stderr[-2000:])
