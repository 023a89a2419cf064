"""CPU tests of elp_stage_bgzf's plan (elprep_amd/csrc/bgzf_plan.hpp, built by the host compiler through tests/bgzf_plan_host.cpp): the
parser of the member headers, the cuts into inflate and scan pieces, the halving of a piece whose token scratch does not fit, the chunk
schedule, the layout of the two scratch slots, the result words and the vote for the common block length.  A sub-buffer that is a few
words short shows on the device only as a silent overlap, so the expected values below are worked out by hand in the docstrings, not
computed from the code.  The parser also runs on its own under the sanitizers (tests/bgzf_parse_asan.cpp).

A member: 10 fixed bytes (1f 8b 08, FLG with FEXTRA = 04, ...) | XLEN (2) | the extra field, subfields of id (2), length (2), data - "BC",
2, BSIZE = the member's size - 1 | DEFLATE data | CRC-32 (4) | ISIZE (4).  With BC alone XLEN is 6: 18 bytes of header, 8 of trailer."""
import ctypes as C
import os
import struct
import subprocess
import zlib

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tests", "libbgzf_plan_host.so")
HDR = os.path.join(ROOT, "elprep_amd", "csrc", "bgzf_plan.hpp")
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
ERRORS = ("ok", "truncated_header", "not_bgzf", "truncated_extra", "no_bc", "bad_size", "isize_too_big")
SCRATCH = ("entry", "exit", "res", "cnt", "base", "bad_list", "words64", "ntok", "pow_common", "elems")
TOK_STRIDE, RES_THREADS, REC_BAD_CAP = 21888, 1024, 1024


@pytest.fixture(scope="module")
def lib():
    src = os.path.join(ROOT, "tests", "bgzf_plan_host.cpp")
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(src), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", SO, src])
    L = C.CDLL(SO)
    L.bz_cut.restype = C.c_uint64
    L.bz_common_len.restype = C.c_uint32
    return L


def _member(part: bytes, before: bytes = b"", bc: bytes = b"BC", isize=None, bsize=None, level: int = 6) -> bytes:
    """as _bgzf in tests/test_gpu_round4.py builds them; `before`: subfields in front of BC; isize / bsize: what the member claims"""
    co = zlib.compressobj(level, zlib.DEFLATED, -15)
    data = co.compress(part) + co.flush()
    xlen = len(before) + 6
    total = 12 + xlen + len(data) + 8
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff" + struct.pack("<H", xlen) + before + bc + b"\x02\x00" +
            struct.pack("<H", (total if bsize is None else bsize) - 1) + data + struct.pack("<II", zlib.crc32(part), len(part) if isize is None else isize))


def _data_len(member: bytes, xlen: int = 6) -> int:
    return len(member) - 12 - xlen - 8


def _parse(L, data: bytes):
    out = (C.c_uint64 * 5)()
    blk = (C.c_uint64 * (5 * 16))()
    text = C.create_string_buffer(200)
    buf = (C.c_uint8 * max(1, len(data))).from_buffer_copy(data or b"\0")
    L.bz_parse(buf, C.c_uint64(len(data)), out, blk, C.c_uint64(16), text, C.c_uint64(200))
    blocks = [dict(zip(("in_off", "in_len", "out_len", "out_off", "crc"), blk[5 * k:5 * k + 5])) for k in range(min(out[3], 16))]
    return dict(error=ERRORS[out[0]], at=out[1], claimed=out[2], n=out[3], inflated=out[4], blocks=blocks, text=text.value.decode())


def _fails(L, data: bytes, error: str, text: str):
    r = _parse(L, data)
    assert (r["error"], r["text"]) == (error, text), r
    return r


PARTS = (bytes(range(256)) * 4, b"elprep" * 500, b"\x07" * 300)  # 1024, 3000 and 300 bytes


# ---- the parser

def test_parse_three_members_and_the_end_of_file_block(lib):
    """Members of 1024, 3000 and 300 inflated bytes, then the 28-byte empty block.  Every member's DEFLATE data starts 18 bytes behind its
    first byte and is the member's size - 26 long; the blocks stand at 0, 1024 and 4024 of the inflated stream, 4324 bytes in all.  The
    empty block (ISIZE 0) is not listed; without it the same three blocks come out: it is not required."""
    ms = [_member(p) for p in PARTS]
    starts = (0, len(ms[0]), len(ms[0]) + len(ms[1]))
    for tail in (EOF_BLOCK, b""):
        r = _parse(lib, b"".join(ms) + tail)
        assert (r["error"], r["n"], r["inflated"], r["text"]) == ("ok", 3, 4324, ""), r
        assert r["blocks"] == [dict(in_off=starts[k] + 18, in_len=len(ms[k]) - 26, out_len=len(PARTS[k]), out_off=(0, 1024, 4024)[k], crc=zlib.crc32(PARTS[k]))
                               for k in range(3)]
    assert _parse(lib, b"") == dict(error="ok", at=0, claimed=0, n=0, inflated=0, blocks=[], text="")


def test_parse_bc_behind_another_subfield(lib):
    """A subfield "XY" of three data bytes (7 bytes) in front of BC: XLEN = 13, the DEFLATE data starts at byte 12 + 13 = 25 of the
    member and is its size - 25 - 8 long.  The second member, with BC alone, starts where the first ends."""
    m0, m1 = _member(PARTS[0], before=b"XY\x03\x00abc"), _member(PARTS[2])
    r = _parse(lib, m0 + m1 + EOF_BLOCK)
    assert r["error"] == "ok" and r["blocks"] == [dict(in_off=25, in_len=len(m0) - 33, out_len=1024, out_off=0, crc=zlib.crc32(PARTS[0])),
                                                  dict(in_off=len(m0) + 18, in_len=len(m1) - 26, out_len=300, out_off=1024, crc=zlib.crc32(PARTS[2]))]


def test_parse_skips_an_empty_member_in_the_middle(lib):
    """An ISIZE-0 member (the end-of-file block, 28 bytes) between two others is not listed; the block behind it lies 28 bytes further on
    in the file and where it would have been in the inflated stream (1024)."""
    m0, m1 = _member(PARTS[0]), _member(PARTS[1])
    r = _parse(lib, m0 + EOF_BLOCK + m1)
    assert (r["error"], r["n"], r["inflated"]) == ("ok", 2, 4024)
    assert r["blocks"][1] == dict(in_off=len(m0) + 28 + 18, in_len=len(m1) - 26, out_len=3000, out_off=1024, crc=zlib.crc32(PARTS[1]))


def test_parse_truncated_header(lib):
    """17 bytes are no header (18: 12 fixed + BC's 6), at the file's start and behind a whole member; with the 18th byte the header
    stands and it is the block's size that reaches behind the data."""
    m0 = _member(PARTS[0])
    _fails(lib, m0[:17], "truncated_header", "elp_stage_bgzf: truncated block header at byte 0")
    _fails(lib, m0[:1], "truncated_header", "elp_stage_bgzf: truncated block header at byte 0")
    r = _fails(lib, m0 + m0[:17], "truncated_header", "elp_stage_bgzf: truncated block header at byte %d" % len(m0))
    assert r["at"] == len(m0)
    _fails(lib, m0[:18], "bad_size", "elp_stage_bgzf: bad block size at byte 0")


def test_parse_not_a_bgzf_block(lib):
    """Each of the three magic bytes wrong, and FEXTRA (bit 2 of byte 3) clear: other flag bits do not matter."""
    m0 = _member(PARTS[0])
    for at, value in ((0, 0x1e), (1, 0x8a), (2, 9), (3, 0x00), (3, 0xfb)):
        bad = bytearray(m0)
        bad[at] = value
        _fails(lib, bytes(bad), "not_bgzf", "elp_stage_bgzf: not a BGZF block at byte 0")
        _fails(lib, m0 + bytes(bad), "not_bgzf", "elp_stage_bgzf: not a BGZF block at byte %d" % len(m0))
    ok = bytearray(m0)
    ok[3] = 0xff
    assert _parse(lib, bytes(ok))["error"] == "ok"


def test_parse_truncated_extra_field(lib):
    """A member of S bytes alone in the file whose XLEN says S - 12 + 1: the extra field ends one byte behind the data.  S - 12: it ends
    with the data, BC (the first subfield) is found and its size S is below 12 + XLEN + 8: a bad block size."""
    m0 = _member(PARTS[2])
    S = len(m0)
    _fails(lib, m0[:10] + struct.pack("<H", S - 11) + m0[12:], "truncated_extra", "elp_stage_bgzf: truncated extra field at byte 0")
    _fails(lib, m0 + m0[:10] + struct.pack("<H", S - 11) + m0[12:], "truncated_extra", "elp_stage_bgzf: truncated extra field at byte %d" % S)
    _fails(lib, m0[:10] + struct.pack("<H", S - 12) + m0[12:], "bad_size", "elp_stage_bgzf: bad block size at byte 0")


def test_parse_missing_bc(lib):
    """No subfield named BC; BC of another length than 2; an extra field too short for a subfield (XLEN 3)."""
    m0 = _member(PARTS[0])
    text = "missing BC extra subfield in BGZF header (block at byte %d)"
    _fails(lib, _member(PARTS[2], bc=b"BD"), "no_bc", text % 0)
    _fails(lib, m0 + _member(PARTS[2], bc=b"CB"), "no_bc", text % len(m0))
    _fails(lib, m0[:14] + b"\x03\x00" + m0[16:], "no_bc", text % 0)
    _fails(lib, m0[:10] + b"\x03\x00" + m0[12:], "no_bc", text % 0)


def test_parse_bad_block_size(lib):
    """BC alone: a member is 12 + 6 + 8 = 26 bytes at least.  One of exactly 26 (no DEFLATE data, ISIZE 0) parses and lists nothing; a
    claim of 25 is refused.  A size that reaches one byte behind the data is refused, at byte 0 and behind a member."""
    empty = _member(b"")[:18] + struct.pack("<II", 0, 0)
    ok = empty[:16] + struct.pack("<H", 25) + empty[18:]
    assert len(ok) == 26 and (_parse(lib, ok)["error"], _parse(lib, ok)["n"]) == ("ok", 0)
    _fails(lib, empty[:16] + struct.pack("<H", 24) + empty[18:], "bad_size", "elp_stage_bgzf: bad block size at byte 0")
    m0 = _member(PARTS[0])
    _fails(lib, m0[:-1], "bad_size", "elp_stage_bgzf: bad block size at byte 0")
    _fails(lib, m0 + m0[:-1], "bad_size", "elp_stage_bgzf: bad block size at byte %d" % len(m0))
    _fails(lib, _member(PARTS[0], bsize=len(m0) + 1), "bad_size", "elp_stage_bgzf: bad block size at byte 0")


def test_parse_isize_above_64k(lib):
    """ISIZE 65536 is the most a block may claim; 65537 is refused with the claim in the text."""
    m0 = _member(PARTS[0])
    r = _parse(lib, _member(PARTS[0], isize=65536))
    assert r["error"] == "ok" and r["blocks"][0]["out_len"] == 65536
    r = _fails(lib, m0 + _member(PARTS[0], isize=65537), "isize_too_big", "elp_stage_bgzf: block at byte %d claims 65537 inflated bytes" % len(m0))
    assert (r["at"], r["claimed"]) == (len(m0), 65537)


def test_parser_alone_under_the_sanitizers(tmp_path):
    """tests/bgzf_parse_asan.cpp: every truncation and every damaged header byte from a buffer of exactly the file's size.  The sanitizers'
    runtimes are linked into the program where the compiler has them as archives, so that nothing has to stand in front of them in the
    list of libraries."""
    src = os.path.join(ROOT, "tests", "bgzf_parse_asan.cpp")
    exe = str(tmp_path / "bgzf_parse_asan")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src]
    if subprocess.call(cmd + ["-static-libasan", "-static-libubsan"], stderr=subprocess.DEVNULL) != 0:
        subprocess.check_call(cmd)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "bgzf_parse_asan: ok" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stdout, r.stderr[-2000:])


# ---- the cuts

def _cut(L, lens, start, limit, max_bytes):
    return L.bz_cut((C.c_uint32 * len(lens))(*lens), C.c_uint64(len(lens)), C.c_uint64(start), C.c_uint64(limit), C.c_uint64(max_bytes))


def test_inflate_pieces(lib):
    """Five blocks of 65280 and a last one of 1000.  IPIECE 150000: 2 x 65280 = 130560 fits, 195840 does not: pieces [0, 2) [2, 4); from
    block 4: 65280 + 1000 = 66280: [4, 6).  IPIECE 130560 exactly: still two; 130559: one.  IPIECE 65279: less than a block - the first block
    is always taken: one per piece.  A cut never passes its limit."""
    lens = [65280] * 5 + [1000]
    assert [_cut(lib, lens, a, 6, 150000) for a in (0, 2, 4)] == [2, 4, 6]
    assert (_cut(lib, lens, 0, 6, 130560), _cut(lib, lens, 0, 6, 130559)) == (2, 1)
    assert [_cut(lib, lens, a, 6, 65279) for a in range(6)] == [1, 2, 3, 4, 5, 6]
    assert _cut(lib, lens, 0, 6, 1 << 40) == 6 and _cut(lib, lens, 3, 5, 1 << 40) == 5 and _cut(lib, lens, 6, 6, 150000) == 6


def test_scan_pieces_inside_an_inflate_piece(lib):
    """Inside the inflate piece [0, 2): PIECE 70000 holds one block of 65280 (130560 > 70000): [0, 1) [1, 2); 130560: both.  Inside [4, 6), the
    short last block: 66280 <= 70000: one scan piece."""
    lens = [65280] * 5 + [1000]
    assert [_cut(lib, lens, b, 2, 70000) for b in (0, 1)] == [1, 2]
    assert _cut(lib, lens, 0, 2, 130560) == 2
    assert _cut(lib, lens, 4, 6, 70000) == 6 and _cut(lib, lens, 4, 6, 66279) == 5


def _fit(L, nt, fail_above, room):
    out = (C.c_uint64 * 3)()
    L.bz_tok_fit(C.c_uint64(nt), fail_above, C.c_uint64(room), out)
    return tuple(out)  # blocks taken, pretended, times the scratch was asked for


def test_halving(lib):
    """100 blocks, "does not fit" above 37: 100 and 50 are refused unasked, 25 is asked for and fits - the next piece starts at block 25.
    Failure above 0: the key is off, 100 fit at once.  A device with room for 10: 100, 50, 25, 12 fail, 6 fit (four requests failed, the
    fifth fits); with the key at 37 the first two are not asked: three requests.  One block that still fails is the error (0 blocks), and
    it is a real one: the key cannot refuse a single block."""
    big = 1 << 40
    assert _fit(lib, 100, 37, big) == (25, 0, 1)
    assert _fit(lib, 100, 0, big) == (100, 0, 1)
    assert _fit(lib, 37, 37, big) == (37, 0, 1) and _fit(lib, 38, 37, big) == (19, 0, 1)
    assert _fit(lib, 100, 0, 10) == (6, 0, 5)
    assert _fit(lib, 100, 37, 10) == (6, 0, 3)
    assert _fit(lib, 1, 0, 0) == (0, 0, 1)
    assert _fit(lib, 3, 0, 0) == (0, 0, 2)
    assert _fit(lib, 3, 1, 0) == (0, 0, 1)


# ---- the chunks

def _chunks(L, na, copy_chunk, div, n_cu):
    out = (C.c_uint64 * (4 + 3 * 64))()
    L.bz_chunks(na, copy_chunk, div, n_cu, out, C.c_uint64(64))
    return dict(chunk=out[0], first=out[1], lane=out[2], turns=[tuple(out[4 + 3 * k:7 + 3 * k]) for k in range(out[3])])


def test_chunk_sizes(lib):
    """256 CUs: 24 x 256 = 6144 blocks fill the chip, the first chunk is a quarter: 1536.  32 CUs: 768 < 1024: 1024 and 256.  The key
    "bgzf_copy_chunk" replaces either.  Divisor 0 (and below) counts as 1: the first chunk is a whole one.  A chunk of 3 by 4 is 0: 1."""
    assert {k: _chunks(lib, 1, 0, 4, 256)[k] for k in ("chunk", "first")} == dict(chunk=6144, first=1536)
    assert {k: _chunks(lib, 1, 0, 4, 32)[k] for k in ("chunk", "first")} == dict(chunk=1024, first=256)
    assert {k: _chunks(lib, 1, 500, 4, 256)[k] for k in ("chunk", "first")} == dict(chunk=500, first=125)
    assert _chunks(lib, 1, 0, 0, 256)["first"] == 6144 and _chunks(lib, 1, 0, -3, 256)["first"] == 6144
    assert _chunks(lib, 1, 3, 4, 256)["first"] == 1


def test_chunk_turns(lib):
    """Chunks of 3, the first of 1, eight blocks: [0, 1) [1, 4) [4, 7) [7, 8); 8 > 3: the side lane, for turns 1 and 3.  Three blocks: [0, 1)
    [1, 3), not more than one chunk: no lane.  Divisor 0: [0, 3) [3, 6) [6, 8).  20000 blocks on 256 CUs: 1536, then 6144 each, the odd
    turns on the lane; 6144 blocks: 6144 > 6144 fails, no lane."""
    assert _chunks(lib, 8, 3, 4, 256) == dict(chunk=3, first=1, lane=1, turns=[(0, 1, 0), (1, 4, 1), (4, 7, 0), (7, 8, 1)])
    assert _chunks(lib, 3, 3, 4, 256) == dict(chunk=3, first=1, lane=0, turns=[(0, 1, 0), (1, 3, 0)])
    assert _chunks(lib, 8, 3, 0, 256)["turns"] == [(0, 3, 0), (3, 6, 1), (6, 8, 0)]
    assert _chunks(lib, 20000, 0, 4, 256) == dict(chunk=6144, first=1536, lane=1, turns=[(0, 1536, 0), (1536, 7680, 1), (7680, 13824, 0), (13824, 19968, 1), (19968, 20000, 0)])
    assert _chunks(lib, 6144, 0, 4, 256) == dict(chunk=6144, first=1536, lane=0, turns=[(0, 1536, 0), (1536, 6144, 0)])
    assert _chunks(lib, 1, 0, 4, 256)["turns"] == [(0, 1, 0)]


# ---- the scratch slots and the result words

def _scratch(L, na):
    out = (C.c_uint64 * len(SCRATCH))()
    L.bz_scratch(na, out)
    return dict(zip(SCRATCH, out))


def test_constants(lib):
    """what the layout below is worked out with, and the writer's sizes: 65280 + 31 <= 65344 = 1021 x 64"""
    out = (C.c_uint64 * 6)()
    lib.bz_consts(out)
    assert tuple(out) == (TOK_STRIDE, RES_THREADS, REC_BAD_CAP, 65280, 31, 65344)


def test_scratch_layout_of_five_blocks(lib):
    """Slot 6 in 64-bit words: the block table 5 x 4 = 20 words at 0 | entry at 20 | exit at 25 | res at 30, 8 words, to 38 = 32-bit word 76:
    cnt there, 5 + 8 | base at 89 | bad_list at 102, 1024 entries to 32-bit word 1126 = word 563.  The request: 30 + 8 + 13 + 16 + 512 = 579.
    Slot 7 in tokens of 8 bytes: ntok behind 5 x 21888 = 109440 of them; pow_common 6 32-bit words behind ntok (5 rounded up to even); the
    request 109440 + (5 + 2) / 2 = 3 + 512 + 8."""
    s = _scratch(lib, 5)
    assert s == dict(entry=20, exit=25, res=30, cnt=76, base=89, bad_list=102, words64=579, ntok=109440, pow_common=6, elems=109440 + 3 + 512 + 8)
    assert (s["bad_list"] + REC_BAD_CAP) // 2 == 563


def test_scratch_slots_hold_their_sub_buffers(lib):
    """Consecutive sub-buffers do not overlap given their element counts and the last ends inside the request; entry, exit and res start on
    whole 64-bit words behind a block table of whole 32-byte entries at the slot's start, and the 32-bit part starts right behind res's
    eight words.  This is the layout as it was before the plan became a header; it must not move here."""
    for na in (1, 2, 5, 36, 37, 1023, 1024, 33000):
        s = _scratch(lib, na)
        # slot 6, in bytes: blk 32 na | entry 8 na | exit 8 na | res 64 | cnt 4 na | base 4 na | bad_list 4 x 1024
        parts = ((0, 32 * na), (8 * s["entry"], 8 * na), (8 * s["exit"], 8 * na), (8 * s["res"], 64), (4 * s["cnt"], 4 * na), (4 * s["base"], 4 * na),
                 (4 * s["bad_list"], 4 * REC_BAD_CAP), (8 * s["words64"], 0))
        for (a, size), (b, _) in zip(parts, parts[1:]):
            assert a + size <= b, (na, a, size, b)
        assert all(8 * s[k] % 8 == 0 for k in ("entry", "exit", "res")) and (32 * na) % 16 == 0 and 4 * s["cnt"] == 8 * s["res"] + 64, na
        # slot 7, in bytes: tokens 8 x 21888 na | ntok 4 na | pow_common 4 x 1024
        ntok, pow_common = 8 * s["ntok"], 8 * s["ntok"] + 4 * s["pow_common"]
        assert 8 * TOK_STRIDE * na <= ntok and ntok + 4 * na <= pow_common and pow_common + 4 * RES_THREADS <= 8 * s["elems"], na
        assert pow_common % 8 == 0, na


def test_result_words(lib):
    """the 32-bit words of `res` the host reads back: bad 1, max_rec 2, the inflater's 8 (the fifth 64-bit word); ten words are read; an
    inflate piece clears all 64 bytes, a scan piece the first 16 - not the inflater's word; its bits: 1 does not inflate, 2 CRC"""
    out = (C.c_uint64 * 8)()
    lib.bz_res(out)
    assert tuple(out) == (1, 2, 8, 10, 64, 16, 1, 2)


# ---- the vote

def test_common_length_vote(lib):
    """The loop of elp_stage_bgzf as it always was: an element met with no votes left becomes the candidate with one vote, an equal one adds
    a vote, another one takes a vote away.
    [a, a, b]: a (1), a (2), b takes one (1): a.  [a, b, b]: a (1), b takes it (0), b becomes the candidate (1): b.  One element: itself.
    [a, b]: a (1), b takes it (0) and nothing follows that could become the candidate: a.  (The issue behind this test lists b for [a, b]
    "as the loop does today"; traced by hand, and run, that loop answers a.  The function is the loop unchanged - any answer is correct,
    it only chooses which length gets the table of CRC powers - and the test pins what it does.)  [a, b, c]: c becomes the candidate."""
    def vote(*lens):
        return lib.bz_common_len((C.c_uint32 * len(lens))(*lens), C.c_uint64(len(lens)))
    a, b, c = 65280, 1000, 7
    assert vote(a, a, b) == a and vote(a, b, b) == b and vote(a) == a
    assert vote(a, b) == a
    assert vote(a, b, c) == c
