"""CPU tests of the emitters' plan (elprep_amd/csrc/emit_plan.hpp and bgzf_framed_size in bgzf_plan.hpp, built by the host compiler
through tests/emit_plan_host.cpp): the bound on an output record, the records of a device pass, what a pass frames into BGZF members
and what it carries on, the size query's term, the capacity test, the layout of the loop's scratch slot, the tag filter's table and
elp_stage_bam's cut of a run of records into pieces.  A mistake of a few bytes here is a silent overlap between scratch slots on the
device and a BGZF member of the wrong length for a caller, so the expected values below are worked out by hand in the docstrings, not
computed from the code.  The cut and the pass functions also run on their own under the sanitizers (tests/emit_plan_asan.cpp)."""
import ctypes as C
import os
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tests", "libemit_plan_host.so")
HDRS = [os.path.join(ROOT, "elprep_amd", "csrc", h) for h in ("emit_plan.hpp", "bgzf_plan.hpp")]
BAM, BGZF, SAM = 0, 1, 2
CUT_ERRORS = ("ok", "bad_offsets", "truncated", "bad_block_size")


@pytest.fixture(scope="module")
def lib():
    src = os.path.join(ROOT, "tests", "emit_plan_host.cpp")
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(p) for p in [src] + HDRS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", SO, src])
    L = C.CDLL(SO)
    for name in ("ep_rec_bound", "ep_query_bytes", "ep_framed_size"):
        getattr(L, name).restype = C.c_uint64
    L.ep_pass_records.restype = C.c_uint32
    return L


def _bound(L, fmt, max_raw_rec, max_name=0):
    return L.ep_rec_bound(fmt, C.c_uint64(max_raw_rec), C.c_uint32(max_name))


def _records(L, rec_bound, tune=0):
    return L.ep_pass_records(C.c_uint64(rec_bound), tune)


def _pass(L, fmt, held, chunk_bytes, last):
    out = (C.c_uint64 * 6)()
    L.ep_pass(fmt, C.c_uint64(held), C.c_uint64(chunk_bytes), int(last), out)
    return dict(zip(("pass_bytes", "frame_bytes", "carry_bytes", "out_bound", "slot5", "slot7"), out))


def _stream(L, fmt, chunks):
    """the passes of a real call over these chunks, as emit_stream runs them: each pass holds what the one before carried"""
    held, passes = 0, []
    for k, chunk in enumerate(chunks):
        p = _pass(L, fmt, held, chunk, k + 1 == len(chunks))
        assert p["pass_bytes"] == held + chunk and held < 65280, p  # the invariant held < BGZF_PAYLOAD
        passes.append(p)
        held = p["carry_bytes"]
    return passes


def test_constants(lib):
    """0xFC000000 = 4227858432 = 63/64 of 4 GiB; 2^21 records; members of 65280 bytes with 31 around a stored one; pieces of 256 MiB =
    268435456 bytes; 65536 bits = 2048 words; 64 bytes of padding behind slots 5 and 7"""
    out = (C.c_uint64 * 7)()
    lib.ep_consts(out)
    assert tuple(out) == (4227858432, 2097152, 65280, 31, 268435456, 2048, 64)
    assert 4227858432 == 0xFC000000 == (1 << 32) // 64 * 63


# ---- the record bound and the pass size

def test_bam_record_bound_and_pass(lib):
    """BAM and BGZF: max(max_raw_rec, 64) + 4, names do not count.  300 -> 304; 4227858432 / 304 = 13.9 million, above 2^21 = 2097152: a
    pass is 2^21 records.  4000 -> 4004; 4004 x 1055908 = 4227855632, 2800 short of 4227858432 (< 4004): 1055908 records.  10 -> the
    floor of 64 applies: 68, and 2^21 records."""
    for fmt in (BAM, BGZF):
        assert _bound(lib, fmt, 300, 77) == 304 and _records(lib, 304) == 2097152
        assert _bound(lib, fmt, 4000) == 4004 and _records(lib, 4004) == 1055908
        assert _bound(lib, fmt, 10) == 68 and _bound(lib, fmt, 64) == 68 and _bound(lib, fmt, 65) == 69 and _records(lib, 68) == 2097152
    assert 4004 * 1055908 == 4227855632 and 4227858432 - 4227855632 == 2800


def test_sam_record_bound_and_pass(lib):
    """SAM: 5 x 4000 + 2 x 5 + 64 = 20074; 20074 x 210613 = 4227845362, 13070 short of 4227858432 (< 20074): 210613 records.  No floor:
    a staged record of 10 bytes and no names gives 5 x 10 + 64 = 114."""
    assert _bound(lib, SAM, 4000, 5) == 20074 and _records(lib, 20074) == 210613
    assert 20074 * 210613 == 4227845362 and 4227858432 - 4227845362 == 13070
    assert _bound(lib, SAM, 10, 0) == 114


def test_pass_of_one_record_and_the_tuning_key(lib):
    """A bound above 0xFC000000 (one byte above; a SAM bound of 5 x 2^30 + 64): the division gives 0, a pass is 1 record.  Exactly
    0xFC000000: 1 too.  The key "emit_pass": 97 caps 2^21 and 1055908 at 97, leaves a pass of 1 at 1; 0 (and below) is off; a key above
    the pass's own size changes nothing."""
    assert _records(lib, 0xFC000001) == 1 and _records(lib, 0xFC000000) == 1 and _records(lib, 0xFC000000 // 2) == 2
    assert _bound(lib, SAM, 1 << 30, 0) == 5 * (1 << 30) + 64 and _records(lib, 5 * (1 << 30) + 64) == 1
    assert _records(lib, 304, 97) == 97 and _records(lib, 4004, 97) == 97 and _records(lib, 0xFC000001, 97) == 1
    assert _records(lib, 304, 0) == 2097152 and _records(lib, 304, -1) == 2097152 and _records(lib, 4004, 0) == 1055908
    assert _records(lib, 4004, 2000000) == 1055908 and _records(lib, 304, 1 << 30) == 2097152 and _records(lib, 304, 1) == 1


# ---- the passes

def test_bgzf_passes_keep_members_whole(lib):
    """Chunks of 100000, 50000 and 30000 bytes, the third the last.  Pass 1 holds 100000: one member of 65280 goes out (65280 + 31 =
    65311 in stored form), 34720 are carried.  Pass 2 holds 34720 + 50000 = 84720: one member again, 84720 - 65280 = 19440 carried.
    Pass 3 holds 19440 + 30000 = 49440 and is the last: all of it, 49440 + 31 = 49471.  Three members for 180000 bytes:
    2 x 65311 + 49471 = 180093 = 180000 + 3 x 31.  Slot 5 is asked for the pass + 64, slot 7 for the bound + 64."""
    p = _stream(lib, BGZF, (100000, 50000, 30000))
    assert [q["pass_bytes"] for q in p] == [100000, 84720, 49440]
    assert [q["frame_bytes"] for q in p] == [65280, 65280, 49440]
    assert [q["carry_bytes"] for q in p] == [34720, 19440, 0]
    assert [q["out_bound"] for q in p] == [65311, 65311, 49471]
    assert sum(q["out_bound"] for q in p) == 180093 == 180000 + 3 * 31 and sum(q["frame_bytes"] for q in p) == 180000
    assert [q["slot5"] for q in p] == [100064, 84784, 49504] and [q["slot7"] for q in p] == [65375, 65375, 49535]


def test_bgzf_pass_below_one_member_and_on_a_member_boundary(lib):
    """A pass that is not the last and holds less than a member (100 carried in + 1000): nothing is framed, nothing goes out (bound 0), all
    1100 bytes are carried; 65279 bytes: the same.  280 + 65000 = 65280, exactly a member: it goes out, carry 0 - last or not.  Two
    members and a byte: 130560 out (130560 + 62 = 130622), 1 carried.  A last pass that holds nothing frames nothing: bound 0."""
    assert _pass(lib, BGZF, 100, 1000, False) == dict(pass_bytes=1100, frame_bytes=0, carry_bytes=1100, out_bound=0, slot5=1164, slot7=64)
    assert _pass(lib, BGZF, 65000, 279, False)["carry_bytes"] == 65279 and _pass(lib, BGZF, 65000, 279, False)["out_bound"] == 0
    for last in (False, True):
        assert _pass(lib, BGZF, 280, 65000, last) == dict(pass_bytes=65280, frame_bytes=65280, carry_bytes=0, out_bound=65311, slot5=65344, slot7=65375)
    assert _pass(lib, BGZF, 1, 130560, False) == dict(pass_bytes=130561, frame_bytes=130560, carry_bytes=1, out_bound=130622, slot5=130625, slot7=130686)
    assert _pass(lib, BGZF, 1, 130560, True)["out_bound"] == 130561 + 3 * 31
    assert _pass(lib, BGZF, 0, 0, True) == dict(pass_bytes=0, frame_bytes=0, carry_bytes=0, out_bound=0, slot5=64, slot7=64)
    assert _pass(lib, BGZF, 100, 1000, True)["out_bound"] == 1100 + 31


def test_bam_and_sam_passes_go_out_as_they_are(lib):
    """the same chunks as BAM records or SAM lines: every pass sends its chunk, nothing is held or carried, last or not"""
    for fmt in (BAM, SAM):
        p = _stream(lib, fmt, (100000, 50000, 30000))
        assert [(q["pass_bytes"], q["frame_bytes"], q["carry_bytes"], q["out_bound"]) for q in p] == [(100000, 100000, 0, 100000), (50000, 50000, 0, 50000), (30000, 30000, 0, 30000)]
        assert _pass(lib, fmt, 0, 70000, False) == _pass(lib, fmt, 0, 70000, True)


def test_size_query_is_an_upper_bound_for_bgzf_and_exact_otherwise(lib):
    """A query frames every pass on its own: 100000 -> two members, + 62 = 100062; 50000 -> 50031; 30000 -> 30031: 180124.  The real call
    frames 180093 in stored form (above): the query is 31 bytes looser - one short member more, kept as it always was - and never below.
    BAM and SAM: the chunks' sum."""
    chunks = (100000, 50000, 30000)
    assert [lib.ep_query_bytes(BGZF, C.c_uint64(b)) for b in chunks] == [100062, 50031, 30031]
    assert sum(lib.ep_query_bytes(BGZF, C.c_uint64(b)) for b in chunks) == 180124 >= sum(q["out_bound"] for q in _stream(lib, BGZF, chunks)) == 180093
    for fmt in (BAM, SAM):
        assert sum(lib.ep_query_bytes(fmt, C.c_uint64(b)) for b in chunks) == 180000
    # whatever the chunks: passes of 1 to 3 members and their edges
    for chunks in ((65280, 65280), (65279, 1, 65280), (1, 1, 1), (65281, 65279), (130561, 5, 200000, 7)):
        assert sum(lib.ep_query_bytes(BGZF, C.c_uint64(b)) for b in chunks) >= sum(q["out_bound"] for q in _stream(lib, BGZF, chunks)) == lib.ep_framed_size(C.c_uint64(sum(chunks)))


def test_capacity(lib):
    """the third pass above needs 49471 bytes behind 2 x 65311 = 130622: a buffer of 180093 holds it, one of 180092 does not; a pass
    that sends nothing fits a full buffer"""
    assert lib.ep_fits(C.c_uint64(130622), C.c_uint64(49471), C.c_uint64(180093)) == 1
    assert lib.ep_fits(C.c_uint64(130622), C.c_uint64(49471), C.c_uint64(180092)) == 0
    assert lib.ep_fits(C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)) == 1 and lib.ep_fits(C.c_uint64(7), C.c_uint64(0), C.c_uint64(7)) == 1
    assert lib.ep_fits(C.c_uint64(0), C.c_uint64(1), C.c_uint64(0)) == 0


def test_bgzf_framed_size(lib):
    """31 bytes around every 65280 or part of it: nothing -> 0; 1 -> 32; 65280 -> 65311; 65281 -> two members, 65281 + 62 = 65343;
    2 x 65280 = 130560 -> 130622"""
    assert [lib.ep_framed_size(C.c_uint64(n)) for n in (0, 1, 65280, 65281, 130560)] == [0, 32, 65311, 65343, 130622]


# ---- slot 4

def test_slot_4_layout(lib):
    """sizes at 0, cnt + 8 words | offs, cnt + 8 | err; the request 2 (cnt + 8) + 8.  cnt 0: 8, 16, 24.  cnt 1: 9, 18, 26.  cnt 1000:
    1008, 2016, 2024."""
    def lay(cnt):
        out = (C.c_uint64 * 4)()
        lib.ep_scratch4(cnt, out)
        return tuple(out)
    assert lay(0) == (0, 8, 16, 24) and lay(1) == (0, 9, 18, 26) and lay(1000) == (0, 1008, 2016, 2024)
    assert lay(1 << 21) == (0, 2097160, 4194320, 4194328)


# ---- the tag filter's table

def _table(L, remove, keep):
    """remove / keep: None = -1, else a list of two-letter keys"""
    words = (C.c_uint32 * 2048)()
    r = L.ep_tag_table(b"".join(remove) if remove else None, -1 if remove is None else len(remove), b"".join(keep) if keep else None, -1 if keep is None else len(keep), words)
    assert r in (0, 1)
    return None if r == 0 else {32 * w + b for w in range(2048) for b in range(32) if words[w] >> b & 1}


def test_tag_table(lib):
    """The key of a field: its first byte low, its second high.  XA = 0x58, 0x41 -> 0x4158 = 16728 (word 522, bit 24); RG = 0x52, 0x47 ->
    0x4752 = 18258; NM = 0x4E, 0x4D -> 0x4D4E = 19790.  AB is 0x4241, BA 0x4142.
    Remove {XA}, no keep list: that one bit.  Keep {RG, NM} alone: every bit but those two.  (0, -1): no filter at all; (0, 0) - keep
    nothing - and (-1, -1) - remove all: every bit.
    Remove all AND keep {RG}: every bit, RG's too.  (The issue behind this test expects only RG clear.  The fold is filters2's order -
    remove, then keep of what is left - as elp_set_tag_filter always computed it: all ones, or-ed with anything, stay all ones.  Pinned
    as it is.)"""
    everything = set(range(65536))
    assert _table(lib, [b"XA"], None) == {16728} and 16728 == 522 * 32 + 24 == 0x4158
    assert _table(lib, [], [b"RG", b"NM"]) == everything - {18258, 19790}
    assert _table(lib, [], None) is None
    assert _table(lib, [], []) == everything and _table(lib, None, None) == everything
    assert _table(lib, None, [b"RG"]) == everything
    assert _table(lib, [b"AB"], None) == {0x4241} and _table(lib, [b"BA"], None) == {0x4142}
    assert _table(lib, [b"XA", b"XA", b"RG"], [b"RG", b"NM", b"XA"]) == everything - {19790}


# ---- elp_stage_bam's pieces

def _records_of(*block_sizes):
    return b"".join(struct.pack("<I", bs) + bytes(bs) for bs in block_sizes)


def _cut(L, data, rec_off=None, at_byte=0, at_rec=0, limit=1 << 28):
    """the piece that begins at at_byte = record at_rec (the walk, rec_off None, counts no records: its next_rec stays 0)"""
    out, off = (C.c_uint64 * 7)(), (C.c_uint64 * 16)()
    text = C.create_string_buffer(200)
    buf = (C.c_uint8 * max(1, len(data))).from_buffer_copy(data or b"\0")
    ro = None if rec_off is None else (C.c_uint64 * len(rec_off))(*rec_off)
    L.ep_cut(buf, C.c_uint64(len(data)), ro, C.c_uint64(0 if rec_off is None else len(rec_off) - 1), C.c_uint64(at_byte),
             C.c_uint64(0 if rec_off is None else at_rec), C.c_uint64(limit), out, off, C.c_uint64(16), text, C.c_uint64(200))
    if out[0]:
        return (CUT_ERRORS[out[0]], out[1]), text.value.decode()
    return dict(off=list(off[:out[3] + 1]), end=out[4], next_rec=out[5], max_raw_rec=out[6])


THREE = _records_of(40, 50, 36)  # records of 44, 54 and 40 bytes at 0, 44 and 98: 138 bytes
THREE_OFF = [0, 44, 98, 138]


def test_cut_three_records_in_one_piece(lib):
    """both forms: the starts 0, 44, 98 and the piece's length 138; the longest record is the second, 50 + the 4 bytes of its block_size
    field = 54.  The offsets' form does not read the bytes: with every block_size field zeroed it answers the same (the device's
    k_bam_fixed compares the two)."""
    want = dict(off=[0, 44, 98, 138], end=138, max_raw_rec=54)
    assert _cut(lib, THREE) == dict(want, next_rec=0)
    assert _cut(lib, THREE, THREE_OFF) == dict(want, next_rec=3)
    assert _cut(lib, bytes(138), THREE_OFF) == dict(want, next_rec=3)
    assert _cut(lib, _records_of(32)) == dict(off=[0, 36], end=36, next_rec=0, max_raw_rec=36)


def test_cut_by_the_piece_limit(lib):
    """A record belongs to the piece if it STARTS less than `limit` bytes behind the piece's first byte; the first record is always taken.
    Limit 44, the first record's length: the second starts at 44, not below 44 - one record per piece: [0, 44), [44, 98), [98, 138), each
    with its own longest record (44, 54, 40); limit 1 and 10 (less than any record; a record longer than the limit is tolerated): the same.
    Limit 45: the second record starts at 44 < 45 and is taken, the third (98) is not: [0, 98), then [98, 138).  (The issue behind this
    test says a limit smaller than two records gives one record per piece; by the loop as it always was that holds up to the FIRST
    record's length, since starts are compared, not ends.  Pinned as it is: a piece is at most the limit + one record - 1 byte.)
    Limit 99: all three (98 < 99).  Both forms agree."""
    for ro in (None, THREE_OFF):
        nxt = (lambda k: 0) if ro is None else (lambda k: k)
        for limit in (44, 10, 1):
            assert _cut(lib, THREE, ro, 0, 0, limit) == dict(off=[0, 44], end=44, next_rec=nxt(1), max_raw_rec=44)
            assert _cut(lib, THREE, ro, 44, 1, limit) == dict(off=[0, 54], end=98, next_rec=nxt(2), max_raw_rec=54)
            assert _cut(lib, THREE, ro, 98, 2, limit) == dict(off=[0, 40], end=138, next_rec=nxt(3), max_raw_rec=40)
        assert _cut(lib, THREE, ro, 0, 0, 45) == dict(off=[0, 44, 98], end=98, next_rec=nxt(2), max_raw_rec=54)
        assert _cut(lib, THREE, ro, 98, 2, 45) == dict(off=[0, 40], end=138, next_rec=nxt(3), max_raw_rec=40)
        assert _cut(lib, THREE, ro, 0, 0, 98)["end"] == 98 and _cut(lib, THREE, ro, 0, 0, 99)["end"] == 138
        assert _cut(lib, THREE, ro, 44, 1, 54)["end"] == 98 and _cut(lib, THREE, ro, 44, 1, 55) == dict(off=[0, 54, 94], end=138, next_rec=nxt(3), max_raw_rec=54)


def test_cut_errors_of_the_walk(lib):
    """Each with its place and elp_stage_bam's text.  A block_size of 31 in the second record: at byte 44.  The stream one byte short
    (137): the third record (block_size 36 at byte 98) reaches to 138.  Three stray bytes behind the last record (141): no room for a
    block_size field at byte 138; one to three bytes are the same, four are a block_size (0) below 32."""
    bad = bytearray(THREE)
    bad[44:48] = struct.pack("<I", 31)
    assert _cut(lib, bytes(bad)) == (("bad_block_size", 44), "elp_stage_bam: bad block_size 31 at byte 44")
    assert _cut(lib, bytes(bad), at_byte=44) == (("bad_block_size", 44), "elp_stage_bam: bad block_size 31 at byte 44")
    assert _cut(lib, bytes(bad), limit=44) == dict(off=[0, 44], end=44, next_rec=0, max_raw_rec=44)
    assert _cut(lib, THREE[:137]) == (("bad_block_size", 98), "elp_stage_bam: bad block_size 36 at byte 98")
    for stray in (1, 2, 3):
        assert _cut(lib, THREE + bytes(stray)) == (("truncated", 138), "elp_stage_bam: truncated record at byte 138")
    assert _cut(lib, THREE + bytes(4)) == (("bad_block_size", 138), "elp_stage_bam: bad block_size 0 at byte 138")
    huge = bytearray(THREE)
    huge[0:4] = struct.pack("<I", 0xFFFFFFFF)
    assert _cut(lib, bytes(huge)) == (("bad_block_size", 0), "elp_stage_bam: bad block_size 4294967295 at byte 0")


def test_cut_errors_of_the_offsets(lib):
    """An entry that leaves its record 35 bytes (79 behind 44): record 1.  36 bytes (80) are a record.  An entry past n_bytes, the last
    one (139 of 138) or one in the middle (200): the record that would end there, 2 and 1.  Entries that run backwards: the record is
    shorter than 36."""
    assert _cut(lib, THREE, [0, 44, 79, 138]) == (("bad_offsets", 1), "elp_stage_bam: bad record offsets at record 1")
    assert _cut(lib, THREE, [0, 44, 80, 138]) == dict(off=[0, 44, 80, 138], end=138, next_rec=3, max_raw_rec=58)
    assert _cut(lib, THREE, [0, 44, 98, 139]) == (("bad_offsets", 2), "elp_stage_bam: bad record offsets at record 2")
    assert _cut(lib, THREE, [0, 44, 200, 138]) == (("bad_offsets", 1), "elp_stage_bam: bad record offsets at record 1")
    assert _cut(lib, THREE, [0, 98, 44, 138]) == (("bad_offsets", 1), "elp_stage_bam: bad record offsets at record 1")
    assert _cut(lib, THREE, [0, 35, 98, 138]) == (("bad_offsets", 0), "elp_stage_bam: bad record offsets at record 0")


def test_plan_alone_under_the_sanitizers(tmp_path):
    """tests/emit_plan_asan.cpp: every truncation of a three-record stream and every damaged byte of its block_size fields from a buffer of
    exactly the stream's size, offset arrays of exactly records + 1 entries, the pass functions at their edges.  The sanitizers' runtimes
    are linked into the program where the compiler has them as archives, so that nothing has to stand in front of them in the list of
    libraries."""
    src = os.path.join(ROOT, "tests", "emit_plan_asan.cpp")
    exe = str(tmp_path / "emit_plan_asan")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src]
    if subprocess.call(cmd + ["-static-libasan", "-static-libubsan"], stderr=subprocess.DEVNULL) != 0:
        subprocess.check_call(cmd)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "emit_plan_asan: ok" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stdout, r.stderr[-2000:])
