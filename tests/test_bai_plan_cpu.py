"""CPU tests of the index calls' plan (elprep_amd/csrc/bai_plan.hpp, built by the host compiler through tests/bai_plan_host.cpp): the
member walk over bytes nobody vouches for, the virtual offset of a stream position, the size of a contig's part and of the whole index,
the layout of the scratch slots - expected values worked out by hand in the docstrings -, the walk on its own under the sanitizers
(tests/bai_plan_asan.cpp), and the two entry points' presence."""
import ctypes as C
import os
import struct
import subprocess

import pytest

from elprep_amd import _lib
from tests import bairef

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tests", "libbai_plan_host.so")
HDRS = [os.path.join(ROOT, "elprep_amd", "csrc", h) for h in ("bai_plan.hpp", "bgzf_plan.hpp")]
ERRORS = ("ok", "truncated", "not_a_member", "bad_bsize", "short_member", "bad_last_isize")
NEW = ("elp_index_sorted_bgzf", "elp_index_merged_bgzf")


@pytest.fixture(scope="module")
def lib():
    src = os.path.join(ROOT, "tests", "bai_plan_host.cpp")
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(p) for p in [src] + HDRS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", SO, src])
    L = C.CDLL(SO)
    for name, n_args in (("bp_voff", 0), ("bp_contig_bytes", 4), ("bp_bin_at", 2), ("bp_chunk_at", 2), ("bp_intv_at", 2), ("bp_total_bytes", 1), ("bp_size", 5)):
        getattr(L, name).restype = C.c_uint64
        getattr(L, name).argtypes = [C.c_uint64] * n_args
    L.bp_voff.argtypes = [C.c_uint64, C.c_void_p, C.c_uint64]
    L.bp_coffsets_fit.argtypes = [C.c_uint64, C.c_uint64]
    L.bp_is_the_stream.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64]
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
    assert L.elp_index_sorted_bgzf(null, null, 0, 0, null, 0, C.byref(n)) != 0
    assert L.elp_index_merged_bgzf(null, null, null, 0, 0, null, 0, C.byref(n)) != 0


def test_constants(lib):
    """the pseudo-bin 37450; windows of 2^14; ends up to 2^29 = 536870912; file offsets below 2^48; the smallest member 18 + 8 = 26 bytes;
    scan tiles of 2048; four result words of 8 bytes"""
    out = (C.c_uint64 * 7)()
    lib.bp_consts(out)
    assert tuple(out) == (37450, 14, 536870912, 1 << 48, 26, 2048, 32)
    assert 37450 == ((1 << 18) - 1) // 7 + 1  # (8^6 - 1) / 7 = 37449 bins, numbered 0 .. 37448; the specification's pseudo-bin is 37450


# ---- the member walk
def _walk(L, data):
    out, coff, text = (C.c_uint64 * 4)(), (C.c_uint64 * 8)(), C.create_string_buffer(240)
    buf = (C.c_uint8 * max(1, len(data))).from_buffer_copy(data or b"\0")
    e = L.bp_members(buf, C.c_uint64(len(data)), out, coff, C.c_uint64(8), text, C.c_uint64(240))
    if e:
        return ERRORS[e], out[0], out[1], text.value.decode()
    return dict(coff=list(coff[:out[2] + 1]), inflated=out[3])


STREAM = bytes(range(256)) * 510 + bytes(100)  # 130560 + 100 bytes: two full members and one of 100
THREE = bairef.bgzf_write(STREAM, level=0)     # stored: a member is 18 + 5 + its payload + 8 bytes


def test_three_members():
    """level 0 writes one stored DEFLATE block of up to 65535 bytes per member - zlib splits 65280 bytes into no more -: the members are 18
    + (5 + 65280) + 8 = 65311, 65311 and 18 + 105 + 8 = 131 bytes"""
    assert len(THREE) == 2 * 65311 + 131
    assert [p for p, _ in bairef.members(THREE)[0]] == [0, 65311, 130622]


def test_walk_of_a_sound_stream(lib):
    """the table has a last entry, the stream's length; the ISIZE add up to 130660.  No bytes at all: no members, one entry, 0"""
    assert _walk(lib, THREE) == dict(coff=[0, 65311, 130622, 130753], inflated=130660)
    assert _walk(lib, b"") == dict(coff=[0], inflated=0)
    assert _walk(lib, THREE[130622:]) == dict(coff=[0, 131], inflated=100)
    assert lib.bp_is_the_stream(THREE, len(THREE), 130660) == 1 and lib.bp_is_the_stream(THREE, len(THREE), 130661) == 0
    assert lib.bp_is_the_stream(b"", 0, 0) == 1 and lib.bp_is_the_stream(b"", 0, 1) == 0


def test_walk_refusals_name_the_byte(lib):
    """Cut inside the third member's header (130622 + 17 bytes): truncated, at its first byte.  Cut behind its header: its BSIZE + 1 = 131
    runs past the end, named at the BSIZE field, byte 130638.  The second member's magic damaged: not a member, at byte 65311; its
    subfield id damaged (byte 65311 + 12): the same.  BSIZE + 1 = 25, below header + trailer.  The first member's ISIZE (its last four
    bytes, at 65307) 65279: every member but the last holds 65280.  The last member's ISIZE 0 or 65281: named at byte 130749."""
    assert _walk(lib, THREE[:130622 + 17])[:2] == ("truncated", 130622)
    assert _walk(lib, THREE[:130622 + 18])[:3] == ("bad_bsize", 130638, 131)
    assert _walk(lib, THREE[:-1])[:3] == ("bad_bsize", 130638, 131)
    bad = bytearray(THREE)
    bad[65311] ^= 1
    assert _walk(lib, bytes(bad))[:2] == ("not_a_member", 65311)
    bad = bytearray(THREE)
    bad[65311 + 12] = ord("X")
    assert _walk(lib, bytes(bad)) == ("not_a_member", 65311, 0, "elp_index_sorted_bgzf: not a BGZF member with the BC subfield first at byte 65311")
    bad = bytearray(THREE)
    bad[16:18] = struct.pack("<H", 24)
    assert _walk(lib, bytes(bad))[:3] == ("bad_bsize", 16, 25)
    bad = bytearray(THREE)
    bad[65307:65311] = struct.pack("<I", 65279)
    assert _walk(lib, bytes(bad))[:3] == ("short_member", 65307, 65279)
    for isize in (0, 65281):
        bad = bytearray(THREE)
        bad[-4:] = struct.pack("<I", isize)
        assert _walk(lib, bytes(bad))[:3] == ("bad_last_isize", 130749, isize)
    # a full last member is sound; a short member in front of another is not
    assert _walk(lib, THREE[:130622]) == dict(coff=[0, 65311, 130622], inflated=130560)
    assert _walk(lib, THREE[130622:] + THREE[:65311])[:3] == ("short_member", 127, 100)


# ---- virtual offsets
def test_virtual_offsets(lib):
    """members at 0, 500, 900 of the bytes, 1200 bytes in all, written at file offset 1000: position 0 -> 1000 << 16; 65279 -> the last
    place of member 0; 65280 -> place 0 of member 1 at 1500; 2 x 65280 + 100 -> place 100 of member 2 at 1900; 3 x 65280, the end of a
    stream whose last member is full -> place 0 at 2200, the byte behind the members"""
    coff = (C.c_uint64 * 4)(0, 500, 900, 1200)
    v = lambda p: lib.bp_voff(1000, coff, p)
    assert v(0) == 1000 << 16 and v(65279) == 1000 << 16 | 65279 and v(65280) == 1500 << 16
    assert v(2 * 65280 + 100) == 1900 << 16 | 100 and v(3 * 65280) == 2200 << 16
    assert lib.bp_voff((1 << 33) + 7, coff, 65281) == ((1 << 33) + 507) << 16 | 1
    assert lib.bp_coffsets_fit(0, 0) == 1 and lib.bp_coffsets_fit((1 << 48) - 2, 1) == 1 and lib.bp_coffsets_fit((1 << 48) - 1, 1) == 0
    assert lib.bp_coffsets_fit(1 << 48, 0) == 0 and lib.bp_coffsets_fit(0, 1 << 48) == 0 and lib.bp_coffsets_fit(0, (1 << 64) - 1) == 0


# ---- sizes
def test_sizes(lib):
    """The hand-derived file of tests/test_bairef_cpu.py: contig 0 has 7 records in 6 bins of one chunk each and 4097 windows: 4 + 6 x 8 +
    6 x 16 + 40 (the pseudo-bin) + 4 + 4097 x 8 = 32968; contig 1 is empty: 8; contig 2: 2 bins, 2 chunks, 2 windows: 4 + 16 + 32 + 40 +
    4 + 16 = 112.  The index: 8 + 33088 + 8 = 33104 - the closed form from the totals (3 contigs, 2 used, 8 bins, 8 chunks, 4099
    windows) agrees, and so does the reference's builder.  Inside a contig: the first bin at 4; with 2 bins and 3 chunks in front a bin
    at 4 + 16 + 48 = 68; the chunk behind 3 bin headers and 3 chunks at 4 + 24 + 48 = 76; n_intv behind 6 bins, 6 chunks and the
    pseudo-bin at 4 + 48 + 96 + 40 = 188."""
    assert lib.bp_contig_bytes(7, 6, 6, 4097) == 32968 and lib.bp_contig_bytes(0, 0, 0, 0) == 8 and lib.bp_contig_bytes(2, 2, 2, 2) == 112
    assert lib.bp_total_bytes(32968 + 8 + 112) == 33104 == lib.bp_size(3, 2, 8, 8, 4099)
    from tests.test_bairef_cpu import _hand_file
    assert len(bairef.build(_hand_file(), 1000, 3)) == 33104
    assert lib.bp_bin_at(0, 0) == 4 and lib.bp_bin_at(2, 3) == 68 and lib.bp_chunk_at(3, 3) == 76 and lib.bp_intv_at(6, 6) == 188
    assert lib.bp_size(70000, 0, 0, 0, 0) == 8 + 70000 * 8 + 8 and lib.bp_total_bytes(0) == 16


# ---- the scratch slots
def test_scratch_layouts(lib):
    """Slot 0, in 64-bit words, for 10 records: three arrays of 11 words at 0, 11, 22; then nine arrays of 11 32-bit words, each in (11 +
    1) / 2 + 4 = 10 words (8 spare 32-bit words): 33, 43, ... 113; the request 123.  No records: arrays of 1 and of 1 / 2 -> 1 + 4 = 5
    words.  Slot 1 for 10: keys at 0, values at 11, 11 + 6 + 4 = 21 words.  Slot 2 for 3 contigs, 2 members, 10 records: the result
    words 0 .. 3, the member table (3) at 4, first and end (4 32-bit words in 2 + 4 = 6) at 7 and 13, bytes and offset (4 each) at 19 and
    23, the partial sums at 27, 2 of them: 29.  For 70000 contigs and 5000 records: halves of 35000 + 4, 70000 / 2048 = 34 tiles + 2."""
    def lay(fn, n_out, *args):
        out = (C.c_uint64 * n_out)()
        fn(*[C.c_uint64(a) for a in args], out)
        return tuple(out)
    assert lay(lib.bp_scratch0, 13, 10) == (0, 11, 22, 33, 43, 53, 63, 73, 83, 93, 103, 113, 123)
    assert lay(lib.bp_scratch0, 13, 0) == (0, 1, 2, 3, 8, 13, 18, 23, 28, 33, 38, 43, 48)
    assert lay(lib.bp_scratch1, 3, 10) == (0, 11, 21) and lay(lib.bp_scratch1, 3, 0) == (0, 1, 6)
    assert lay(lib.bp_scratch2, 8, 3, 2, 10) == (0, 4, 7, 13, 19, 23, 27, 29)
    assert lay(lib.bp_scratch2, 8, 70000, 0, 5000) == (0, 4, 5, 35009, 70013, 140014, 210015, 210051)
    # no two arrays of slot 0 overlap for any count around the parities
    for n in (1, 2, 3, 255, 256, 4097):
        s = lay(lib.bp_scratch0, 13, n)
        assert all(s[k] + n + 1 <= s[k + 1] for k in range(3)) and all(2 * s[k] + n + 1 + 8 <= 2 * s[k + 1] for k in range(3, 12))


def test_plan_alone_under_the_sanitizers(tmp_path):
    """tests/bai_plan_asan.cpp: every truncation and every damaged header byte of a three-member stream from a heap buffer of exactly the
    stream's size.  The sanitizers' runtimes are linked into the program where the compiler has them as archives, so that nothing has to
    stand in front of them in the list of libraries."""
    src = os.path.join(ROOT, "tests", "bai_plan_asan.cpp")
    exe = str(tmp_path / "bai_plan_asan")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src]
    if subprocess.call(cmd + ["-static-libasan", "-static-libubsan"], stderr=subprocess.DEVNULL) != 0:
        subprocess.check_call(cmd)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "bai_plan_asan: ok" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stdout, r.stderr[-2000:])
