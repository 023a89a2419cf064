"""CPU tests of the scalar pieces of the SAM emitters (elprep_amd/csrc/samtext.hpp, built by the host compiler through
tests/samtext_host.cpp - the device kernels run the same functions) against tests/samref.py: the decimal form of an int64 at every width
boundary, the base and CIGAR tables, the float form (known answers, every power of two with its neighbours, every denormal of one bit, 2^20
bit patterns of a fixed seed) and the text of one optional field of every type - each with the size the count-only pass gives, which
must be the number of bytes written (the emitters place every line by those sizes)."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import samref
from tests.test_samref_cpu import KAT, SPECIAL, _sample

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tests", "libsamtext_host.so")


@pytest.fixture(scope="module")
def lib():
    src = os.path.join(ROOT, "tests", "samtext_host.cpp")
    hdr = os.path.join(ROOT, "elprep_amd", "csrc", "samtext.hpp")
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", SO, src])
    L = C.CDLL(SO)
    L.samtext_i64.argtypes = [C.c_void_p, C.c_int64]
    L.samtext_i64_width.argtypes = [C.c_int64]
    L.samtext_f32.argtypes = [C.c_void_p, C.c_uint32]
    L.samtext_base.argtypes = [C.c_uint32]
    L.samtext_base.restype = C.c_uint8
    L.samtext_cigar_op.argtypes = [C.c_uint32]
    L.samtext_cigar_op.restype = C.c_uint8
    L.samtext_field.argtypes = [C.c_void_p, C.c_char_p, C.c_uint8, C.c_char_p, C.c_uint32]
    L.samtext_f32_many.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    L.samtext_f32_many.restype = C.c_uint64
    return L


def test_integers_at_every_width_boundary(lib):
    vals = {0, 1, -1, 2 ** 31 - 1, -2 ** 31, 2 ** 32 - 1, 2 ** 32, -(2 ** 32 - 1), 2 ** 63 - 1, -2 ** 63}
    for k in range(1, 11):
        vals |= {10 ** k - 1, 10 ** k, -(10 ** k - 1), -(10 ** k)}
    buf = C.create_string_buffer(b"#" * 32, 32)
    for v in sorted(vals):
        C.memset(buf, 35, 32)
        n = lib.samtext_i64(buf, v)
        assert buf.raw[:n] == b"%d" % v and buf.raw[n:n + 1] == b"#", v
        assert lib.samtext_i64_width(v) == n == lib.samtext_i64(None, v), v


def test_base_and_cigar_tables(lib):
    assert bytes(lib.samtext_base(k) for k in range(16)) == samref.BASES
    assert bytes(lib.samtext_cigar_op(k) for k in range(9)) == samref.CIGAR_OPS


def _floats(lib, bits):
    bits = np.ascontiguousarray(bits, dtype=np.uint32)
    out = np.full(16 * bits.size, 35, np.uint8)
    ln = np.zeros(bits.size, np.uint8)
    bad = lib.samtext_f32_many(bits.ctypes.data, bits.size, out.ctypes.data, ln.ctypes.data)
    assert bad == 0                                        # the count-only pass agrees, no text is longer than 15 bytes
    raw = out.tobytes()
    return [raw[16 * k:16 * k + int(ln[k])] for k in range(bits.size)]


def _check(lib, bits):
    for b, got in zip(bits, _floats(lib, bits)):
        assert got == samref.float_text(int(b)), hex(int(b))


@pytest.mark.parametrize("bits,text", KAT + SPECIAL)
def test_float_known_answers(lib, bits, text):
    assert _floats(lib, [bits]) == [text]


def test_float_powers_of_two_and_neighbours(lib):
    """at a power of two the float below is half as far as the one above: the narrow side of the interval"""
    bits = [b for ef in range(1, 255) for b in ((ef << 23) - 1, ef << 23, (ef << 23) + 1)]
    _check(lib, bits + [b | 0x80000000 for b in bits])


def test_float_denormals_of_one_bit_and_the_range_ends(lib):
    _check(lib, [1 << k for k in range(23)] + [1, 2, 3, 0x007FFFFE, 0x007FFFFF, 0x00800000, 0x00800001, 0x7F7FFFFE, 0x7F7FFFFF])


def test_float_sample_of_2_to_the_20(lib):
    bits = _sample(77, 1 << 20)
    assert bits.size > 1000000
    _check(lib, bits)


def test_field_sizes_agree_with_the_bytes_written(lib):
    f = lambda x: struct.pack("<f", x)
    fields = [(b"XA", b"A", b"q"), (b"Xc", b"c", b"\x80"), (b"XC", b"C", b"\xff"), (b"Xs", b"s", struct.pack("<h", -32768)),
              (b"XS", b"S", struct.pack("<H", 65535)), (b"Xi", b"i", struct.pack("<i", -2147483648)), (b"XI", b"I", struct.pack("<I", 4294967295)),
              (b"Xf", b"f", f(1234567.0)), (b"Xg", b"f", struct.pack("<I", 0x7FC00000)), (b"XZ", b"Z", b"a\tb c\0"), (b"Xe", b"Z", b"\0")]
    for sub, fmt, vals in ((b"c", "b", [-128, -1, 0, 9, 10, 127]), (b"C", "B", [0, 9, 10, 99, 100, 255]), (b"s", "h", [-32768, -1, 0, 32767]),
                           (b"S", "H", [0, 65535]), (b"i", "i", [-2147483648, -1, 0, 2147483647]), (b"I", "I", [0, 4294967295])):
        for count in (0, 1, len(vals)):
            fields.append((b"B" + sub, b"B", sub + struct.pack("<I%d%s" % (count, fmt), count, *vals[:count])))
    fvals = [1.0, -0.0, 0.1, 1e6, 1e-5, 3.4028235e38, float("inf"), float("-inf")]
    fields.append((b"Bf", b"B", b"f" + struct.pack("<I", len(fvals)) + b"".join(f(v) for v in fvals)))
    fields.append((b"Bn", b"B", b"f" + struct.pack("<II", 1, 0x7FC00000)))
    buf = C.create_string_buffer(b"#" * 512, 512)
    for key, ty, val in fields:
        want = samref.field_text(key, ty, val)
        C.memset(buf, 35, 512)
        n = lib.samtext_field(buf, key, ty[0], val, len(val))
        assert buf.raw[:n] == want and buf.raw[n:n + 1] == b"#", (key, ty)
        assert lib.samtext_field(None, key, ty[0], val, len(val)) == n
