"""CPU tests of mark duplicates' launch plan (elprep_amd/csrc/markdup_plan.hpp, built by the host compiler through
tests/markdup_plan_host.cpp): the sizes the record count fixes, the fragment table's size, the mates' path and the layout of the scratch
blocks.  A wrong table size or a sub-buffer that is a few words short shows on the device only as a rare overflow or a silent overlap, so
the expected values below are worked out by hand in the docstrings, not computed from the code.  Every case sits one below or one above
a step.

The rules.  A table for n entries: the least power of two >= 2 n + 16, at least 1024.  The pair list's partition: the least bbits <= 24
with (n / 2 + 1) >> bbits <= 384; ndig = ceil(bbits / 8) radix passes over sbits = 8 ndig bits, nb = 2^bbits buckets.  Bloom words: 1024
doubled while < n / 16, at most 2^20.  A workgroup covers 256 records (k_md_front 312, k_frag_list 2048, k_pair_list 2048)."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tests", "libmarkdup_plan_host.so")

SIZES = ("T", "bbits", "ndig", "sbits", "nb", "bw", "tab_cap", "npmax", "nfx",
         "grid", "frag_list_blocks", "front_grid", "mate_grid", "coarse_grid", "list_grid", "bounds_grid", "frag_list_grid")
SCRATCH = ("table", "best", "winner", "fkey", "big", "flist", "words1", "bounds_words",
           "coarse", "hash32", "code", "tab_list", "hash_lo", "words6", "pv", "ftable", "fbits", "words64")
MATE = ("fixed", "fast", "listed", "nfixed", "Tm", "list_n")


@pytest.fixture(scope="module")
def lib():
    src = os.path.join(ROOT, "tests", "markdup_plan_host.cpp")
    hdr = os.path.join(ROOT, "elprep_amd", "csrc", "markdup_plan.hpp")
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", SO, src])
    L = C.CDLL(SO)
    L.md_table_size_for.restype = L.md_frag_table_size.restype = C.c_uint64
    L.md_table_size_for.argtypes = [C.c_uint64]
    L.md_frag_table_size.argtypes = [C.c_uint32, C.c_uint64]
    return L


def _sizes(L, n, n_cu=256):
    out = (C.c_uint64 * len(SIZES))()
    L.md_sizes(C.c_uint64(n), n_cu, out)
    return dict(zip(SIZES, out))


def _scratch(L, n, Tf=0):
    out = (C.c_uint64 * len(SCRATCH))()
    L.md_scratch(C.c_uint64(n), C.c_uint64(Tf), out)
    return dict(zip(SCRATCH, out))


def _mate(L, n, n_tab, mate_path, T):
    out = (C.c_uint64 * len(MATE))()
    L.md_mate_plan(C.c_uint64(n), C.c_uint32(n_tab), mate_path, C.c_uint64(T), out)
    return dict(zip(MATE, out))


def _sub(d, **want):
    return {k: d[k] for k in want} == want


# ---- MdSizes

def test_sizes_of_one_record(lib):
    """n = 1: 2 + 16 = 18 -> T = 1024.  n / 2 + 1 = 1 <= 384: bbits 0, no radix pass, one bucket.  n / 16 = 0: 1024 Bloom
    words, 64 lines of 16 words, one workgroup for them.  One workgroup of everything; k_mate_pairs' one workgroup gives the 64 lists
    (1 + 63) / 64 = 1 share of 256 records.  npmax = 3, one fixed slot ((1 + 1) / 2)."""
    assert _sizes(lib, 1) == dict(T=1024, bbits=0, ndig=0, sbits=0, nb=1, bw=1024, tab_cap=256,
                                  npmax=3, nfx=1, grid=1, frag_list_blocks=1, front_grid=1, mate_grid=1, coarse_grid=1, list_grid=1, bounds_grid=1,
                                  frag_list_grid=1)


def test_table_size_crosses_a_power_of_two(lib):
    """2 n + 16 = 1024 at n = 504 (T stays 1024), 1026 at 505 (2048); 2048 at n = 1016, 2050 at 1017 (4096).  No records: 1024."""
    assert [lib.md_table_size_for(n) for n in (0, 504, 505, 1016, 1017)] == [1024, 1024, 2048, 2048, 4096]
    assert [_sizes(lib, n)["T"] for n in (504, 505, 1016, 1017)] == [1024, 2048, 2048, 4096]


def test_pair_list_one_bucket_gives_way_to_a_radix_pass(lib):
    """n = 766: 383 + 1 = 384 <= 384 -> bbits 0; 767: 383 + 1 as well; 768: 385 > 384, 385 >> 1 = 192 -> bbits 1: one radix pass over 8 bits,
    two buckets.  2 n + 16 = 1548 / 1550 / 1552 -> T = 2048.  Workgroups: 766, 767, 768 = 3
    x 256; k_md_front 3 (2 x 312 = 624 < 766); k_pair_bounds over npmax = 768 -> 3, 769 and 770 -> 4.  Fixed slots (n + 1) / 2: 383, 384, 384."""
    one = dict(bbits=0, ndig=0, sbits=0, nb=1, T=2048, grid=3, front_grid=3, list_grid=1, frag_list_blocks=1)
    assert _sub(_sizes(lib, 766), npmax=768, bounds_grid=3, nfx=383, **one)
    assert _sub(_sizes(lib, 767), npmax=769, bounds_grid=4, nfx=384, **one)
    assert _sub(_sizes(lib, 768), npmax=770, bounds_grid=4, nfx=384, bbits=1, ndig=1, sbits=8, nb=2, T=2048, grid=3, front_grid=3)


def test_pair_list_second_radix_pass(lib):
    """n = 197117: n / 2 + 1 = 98559; >> 7 = 769 > 384, >> 8 = 384 -> bbits 8, one pass, 256 buckets.  n = 197118: 98560 >> 8 = 385
    > 384, >> 9 = 192 -> bbits 9: two passes over 16 bits, 512 buckets.
    Both: 2 n + 16 < 2^19 = 524288 = T; n / 16 = 12319 -> 16384 Bloom words, 1024 lines, 4 workgroups.  256 x 769 = 196864 < n <= 197120: 770
    workgroups, (770 + 63) / 64 = 13 of them per list: tab_cap = 13 x 256 = 3328.  2048 x 96 = 196608 < n: 97; 312 x 631 = 196872 < n: 632.
    npmax = 197119 / 197120 <= 256 x 770.  k_frag_list: at most 8 workgroups per CU: 97 on 256 CUs, 32 on 4."""
    both = dict(T=524288, bw=16384, coarse_grid=4, grid=770, mate_grid=770, tab_cap=3328, frag_list_blocks=97,
                list_grid=97, front_grid=632, bounds_grid=770, nfx=98559, frag_list_grid=97)
    assert _sub(_sizes(lib, 197117), bbits=8, ndig=1, sbits=8, nb=256, npmax=197119, **both)
    assert _sub(_sizes(lib, 197118), bbits=9, ndig=2, sbits=16, nb=512, npmax=197120, **both)
    assert _sizes(lib, 197118, n_cu=4)["frag_list_grid"] == 32


def test_bloom_words(lib):
    """n = 16399: n / 16 = 1024, 1024 < 1024 fails: 1024 words.  16400: 1025 -> 2048 words, 128 lines, still one workgroup.  The cap: n = 8388623 -> n / 16 =
    524288 = 2^19: 2^19 words; 8388624 -> 524289: 2^20; n = 2^25 (n / 16 = 2^21) stays at 2^20, 65536 lines, 256 workgroups."""
    assert _sub(_sizes(lib, 16399), bw=1024, coarse_grid=1)
    assert _sub(_sizes(lib, 16400), bw=2048, coarse_grid=1)
    assert _sizes(lib, 8388623)["bw"] == 1 << 19
    assert _sizes(lib, 8388624)["bw"] == 1 << 20
    assert _sub(_sizes(lib, 1 << 25), bw=1 << 20, coarse_grid=256)


def test_bucket_bits_stop_at_24(lib):
    """bbits 23 -> 24 where (n / 2 + 1) >> 23 first exceeds 384: n / 2 + 1 = 385 x 2^23 = 3229614080, n = 6459228158; one record less: 23.
    n = 2^34: (2^33 + 1) >> 24 = 512 > 384 would ask for more: the cap holds at 24 - three passes over 24 bits, 2^24 buckets."""
    assert _sub(_sizes(lib, 6459228157), bbits=23, ndig=3, sbits=24, nb=1 << 23)
    assert _sub(_sizes(lib, 6459228158), bbits=24, ndig=3, sbits=24, nb=1 << 24)
    assert _sub(_sizes(lib, 1 << 34), bbits=24, ndig=3, sbits=24, nb=1 << 24)


# ---- the fragments' table

def test_fragment_table(lib):
    """No true fragment: no table.  One: 4 entries' worth, 2 x 4 + 16 = 24 -> 1024 slots.  100 under a mate table of 4096: 2 x 400 + 16 =
    816 -> 1024.  600 of 1000 records (T = 2048): 4 x 600 = 2400 entries exceed T; 2 x 2400 + 16 = 4816 -> 8192 > T: the mate table's 2048
    slots bound it."""
    assert [lib.md_frag_table_size(nf, 1024) for nf in (0, 1)] == [0, 1024]
    assert lib.md_frag_table_size(100, 4096) == 1024
    assert [lib.md_frag_table_size(nf, 2048) for nf in (0, 1, 600)] == [0, 1024, 2048]


# ---- the mates' path

def test_mate_path_below_eight_records(lib):
    """n / 8 = 0 for n < 8: no n_tab is below it, so such a call is never fixed (nor fast, nor listed) - it takes the full table, T = 1024.
    n = 8, nobody on the table path: 0 < 1 -> fixed and fast; 4 fixed slots; the table for min(8, 1024) = 8 entries: 1024."""
    for n in (1, 7):
        assert _mate(lib, n, 0, 0, 1024) == dict(fixed=0, fast=0, listed=0, nfixed=0, Tm=1024, list_n=n)
    assert _mate(lib, 8, 0, 0, 1024) == dict(fixed=1, fast=1, listed=0, nfixed=4, Tm=1024, list_n=8)
    assert _mate(lib, 8, 1, 0, 1024) == dict(fixed=0, fast=0, listed=0, nfixed=0, Tm=1024, list_n=8)


def test_mate_path_and_first_table_size(lib):
    """n = 100000: T = 2^18 (200016 <= 262144), n / 8 = 12500, 50000 fixed slots.
    n_tab 0: fast; Tm for 1024 entries: 2064 -> 4096; the lists' bound min(n, 4096) = 4096.
    n_tab 1: listed; 4 + 1024 = 1028 entries: 2072 -> 4096; bound 4098.
    n_tab 12499: listed; 4 x 12499 + 1024 = 51020 entries: 102056 -> 131072; bound 2 x 12499 + 4096 = 29094.
    n_tab 12500: not below n / 8: the full table, no fixed slot.  mate_path 2 whatever n_tab: the same."""
    T = 262144
    assert _sizes(lib, 100000)["T"] == T
    assert _mate(lib, 100000, 0, 0, T) == dict(fixed=1, fast=1, listed=0, nfixed=50000, Tm=4096, list_n=4096)
    assert _mate(lib, 100000, 1, 0, T) == dict(fixed=1, fast=0, listed=1, nfixed=50000, Tm=4096, list_n=4098)
    assert _mate(lib, 100000, 12499, 0, T) == dict(fixed=1, fast=0, listed=1, nfixed=50000, Tm=131072, list_n=29094)
    assert _mate(lib, 100000, 12500, 0, T) == dict(fixed=0, fast=0, listed=0, nfixed=0, Tm=T, list_n=29096)
    assert _mate(lib, 100000, 0, 2, T) == dict(fixed=0, fast=0, listed=0, nfixed=0, Tm=T, list_n=4096)
    assert _mate(lib, 100000, 1, 2, T) == dict(fixed=0, fast=0, listed=0, nfixed=0, Tm=T, list_n=4098)


def test_first_table_never_exceeds_the_full_one(lib):
    """n = 1000 (T = 2048), n / 8 = 125, n_tab 124: min(1000, 496 + 1024) = 1000 entries: 2016 -> 2048 = T."""
    assert _mate(lib, 1000, 124, 0, 2048) == dict(fixed=1, fast=0, listed=1, nfixed=500, Tm=2048, list_n=1000)


# ---- the scratch blocks

def test_scratch_offsets_by_hand(lib):
    """n = 1000: 1024 Bloom words | coarse at 1024, 1024 / 512 = 2 words + 16 | hash32 at 1042, n words + 8 | code at 2050, 8 words +
    (1000 + 16) / 4 = 254 | tab_list at 2312, 64 lists x 256 (4 workgroups: one share) + 8 | hash_lo at 18704, 8 + n + 16 -> 19728 words.
    Slot 1: rep | flist at n + 8 = 1008, 2016 words; 501 > 384 -> two buckets: 2 x 2 + 8 = 12 words asked for later.
    Slot 7 with npmax = 1002 and a table of 2048: pk 2004 x 8 bytes | pv at word 4008 | ftable at 6012 | fbits at 8060;
    (8060 + 64 + 64) / 2 + 8 = 4102 64-bit words.
    n = 1001: hash32 at 1042, code at 2051, tab_list at 2051 + 8 + 1017 / 4 = 2313, hash_lo at 18705, 19730 words.  npmax = 1003: pv at
    4012, ftable at 6018, fbits (Tf = 1024) at 7042; (7042 + 32 + 64) / 2 + 8 = 3577."""
    s = _scratch(lib, 1000, 2048)
    assert s == dict(table=2048, best=1016, winner=1016, fkey=1008, big=2008, flist=1008, words1=2016, bounds_words=12, coarse=1024, hash32=1042,
                     code=2050, tab_list=2312, hash_lo=18704, words6=19728, pv=4008, ftable=6012, fbits=8060, words64=4102)
    assert _sub(_scratch(lib, 1001, 1024), coarse=1024, hash32=1042, code=2051, tab_list=2313, hash_lo=18705, words6=19730, flist=1009, words1=2018,
                pv=4012, ftable=6018, fbits=7042, words64=3577)


def test_scratch_blocks_hold_their_sub_buffers(lib):
    """Slots 1, 6 and 7 at odd and even n on both sides of every step above: consecutive sub-buffers do not overlap given their element
    counts and the last ends inside the block.  Offsets are 32-bit words from the slot's start; a slot itself is aligned far beyond 16
    bytes.  Alignment of what kernels load wider than a word: pk and the sort's second half of it, pk + npmax, are whole 64-bit words; pv
    stands at byte 16 npmax; the Bloom filter, read in 64-byte lines, starts its slot.  The fragment table, which k_frag_bits loads 16 bytes
    at a time, stands at word 6 npmax = 6 n + 12: on a 16-byte boundary for even n, on an 8-byte one for odd n.  That is the layout as
    it was before the plan became a header, which must not move here; the test pins it as it is, so that the change that aligns the table
    has to say so."""
    for n in (1, 2, 7, 8, 311, 312, 313, 766, 767, 768, 1000, 1001, 16399, 16400, 197117, 197118, (1 << 20) + 1, 8388623, 8388624):
        S = _sizes(lib, n)
        for nf in (0, 1, n // 200, n):
            Tf = lib.md_frag_table_size(nf, S["T"])
            L = _scratch(lib, n, Tf)
            where = (n, nf)
            # slot 6: bloom bw at 0 | coarse, a bit per 16 words | hash32 n | code n bytes | tab_list 64 x tab_cap | hash_lo n
            parts = (("coarse", S["bw"] // 512), ("hash32", n), ("code", (n + 3) // 4), ("tab_list", 64 * S["tab_cap"]), ("hash_lo", n))
            assert S["bw"] <= L["coarse"], where
            for (a, words), (b, _) in zip(parts, parts[1:] + (("words6", 0),)):
                assert L[a] + words <= L[b], (where, a, b)
            # slot 1: rep n at 0 | flist n; later the buckets' first and last entries
            assert n <= L["flist"] and L["flist"] + n <= L["words1"], where
            assert 2 * S["nb"] <= L["bounds_words"] <= L["words1"], where
            # slot 7: pk 2 npmax x 8 bytes | pv 2 npmax | ftable Tf | fbits Tf / 32
            assert 4 * S["npmax"] <= L["pv"] and L["pv"] + 2 * S["npmax"] <= L["ftable"], where
            assert L["ftable"] + Tf <= L["fbits"] and L["fbits"] + Tf // 32 <= 2 * L["words64"], where
            assert L["pv"] % 4 == 0 and L["ftable"] % 4 == (0 if n % 2 == 0 else 2), where
            # the slots that are one buffer
            assert L["table"] == S["T"] and L["best"] >= n and L["winner"] >= n and L["fkey"] >= n and 2 * n <= L["big"], where
