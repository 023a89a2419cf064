"""CPU tests of the token parsers of SAM text in (elprep_amd/csrc/samparse.hpp, built by the host compiler through
tests/samparse_host.cpp - the kernels of samin.hip run the same functions) against tests/samin_ref.py: strconv's integers at the edges
of every width, CIGAR strings with their merges and refusals, the base table, and float32(ParseFloat(s, 32)): known answers, a million
bit patterns through samref.float_text and back, the exact decimal midpoints between neighbouring floats with the decimals next to them,
the ends of the range, every refused spelling.

As a program (`python -m tests.test_samparse_cpu write FILE` / `check FILE RESULTS`) it writes the tests' tokens for the stand-alone
build of samparse_host.cpp (-DSAMPARSE_MAIN, for a sanitizer run) and compares what that program printed."""
import ctypes as C
import os
import struct
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from tests import samin_ref, samref
from tests.test_samref_cpu import KAT, SPECIAL, _sample

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tests", "libsamparse_host.so")


def _load():
    src = os.path.join(ROOT, "tests", "samparse_host.cpp")
    hdr = os.path.join(ROOT, "elprep_amd", "csrc", "samparse.hpp")
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", SO, src])
    L = C.CDLL(SO)
    L.samparse_int.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(C.c_int64)]
    L.samparse_f32.argtypes = [C.c_char_p, C.c_uint32, C.POINTER(C.c_uint32)]
    L.samparse_cigar.argtypes = [C.c_char_p, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint32)]
    L.samparse_nibble.argtypes = [C.c_uint8]
    L.samparse_entry.argtypes = [C.c_uint8, C.c_char_p, C.c_uint32, C.POINTER(C.c_uint32)]
    L.samparse_int_store.argtypes = [C.c_int64, C.c_char_p]
    L.samparse_f32_many.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    L.samparse_f32_many.restype = None
    return L


@pytest.fixture(scope="module")
def lib():
    return _load()


def _cls(reason, lib):
    return None if reason == 0 else ("unsupported" if reason >= lib.samparse_unsupported_from() else "data")


def _want(fn, *args):
    """(value, None) or (None, class of the refusal) of the restatement"""
    try:
        return fn(*args), None
    except samin_ref.SamError as e:
        return None, e.cls


# ---- integers
WIDTHS = [(8, True), (16, True), (32, True), (64, True), (8, False), (16, False), (32, False)]


def int_tokens():
    out = []
    for bits, signed in WIDTHS:
        edges = {0, 1, 9, 10, 2 ** (bits - 1) - 1, 2 ** (bits - 1), 2 ** (bits - 1) + 1, 2 ** bits - 1, 2 ** bits, 2 ** bits + 1, 10 ** 19, 10 ** 20, 2 ** 64}
        toks = set()
        for v in edges:
            toks |= {b"%d" % v, b"+%d" % v, b"-%d" % v, b"000%d" % v, b"-000%d" % v}
        toks |= {b"", b"+", b"-", b"--1", b"+-1", b"1_0", b"0x10", b"1 ", b" 1", b"1.0", b"1e3", b"12a", b"a", b"\xb9"}
        out += [(bits, signed, t) for t in sorted(toks)]
    return out


def test_integers_at_the_edges_of_every_width(lib):
    v = C.c_int64()
    for bits, signed, tok in int_tokens():
        want, cls = _want(samin_ref.parse_int if signed else samin_ref.parse_uint, tok, bits)
        ok = lib.samparse_int(tok, len(tok), bits, int(signed), C.byref(v))
        assert (ok == 1) == (cls is None), (bits, signed, tok)
        if ok:
            assert v.value == want, (bits, signed, tok)


def test_restated_integers_by_hand():
    """the restatement itself, against strconv's documentation: signs for ParseInt only, the range of the width, digits only"""
    assert samin_ref.parse_int(b"-128", 8) == -128 and samin_ref.parse_int(b"+127", 8) == 127 and samin_ref.parse_uint(b"255", 8) == 255
    for fn, tok, bits in ((samin_ref.parse_int, b"128", 8), (samin_ref.parse_int, b"-129", 8), (samin_ref.parse_uint, b"256", 8), (samin_ref.parse_uint, b"+1", 8),
                          (samin_ref.parse_uint, b"-0", 16), (samin_ref.parse_int, b"", 32), (samin_ref.parse_int, b"1_0", 32), (samin_ref.parse_int, b"2147483648", 32)):
        with pytest.raises(samin_ref.SamError):
            fn(tok, bits)


def test_integer_store_rule_and_base_table(lib):
    t = C.create_string_buffer(1)
    for v, ty, n in ((-2 ** 31, b"i", 4), (-32769, b"i", 4), (-32768, b"s", 2), (-129, b"s", 2), (-128, b"c", 1), (-1, b"c", 1), (0, b"C", 1), (255, b"C", 1),
                     (256, b"S", 2), (65535, b"S", 2), (65536, b"I", 4), (2 ** 32 - 1, b"I", 4)):
        assert lib.samparse_int_store(v, t) == n and t.raw == ty, v
    for c in range(256):
        want = samin_ref.BASES.index(bytes([c])) if bytes([c]) in samin_ref.BASES else 15
        assert lib.samparse_nibble(c) == want, c


# ---- CIGAR
CIGARS = [b"*", b"", b"5M", b"5M5M", b"5M5M3I5M", b"1M2I3D4N5S6H7P8=9X", b"1m2i3d4n5s6h7p8x", b"0M", b"00012M", b"268435455M", b"268435456M", b"268435455M1M",
          b"134217728M134217727M", b"134217728M134217728M", b"2147483647M", b"2147483648M", b"5", b"5M5", b"M", b"5MM", b"5Q", b"5M*", b"**", b"+5M", b"-5M", b"5 M",
          b"1M" * 100, b"1M1I" * 100, b"1M1I" * 32767 + b"1M", b"1M1I" * 32768, b"1M" * 70000, b"3M" * 64 + b"2I" + b"1M" * 65, b"10M" * 21 + b"7D"]


def test_cigar_strings(lib):
    ops = np.zeros(65536, np.uint32)
    n = C.c_uint32()
    for s in CIGARS:
        want, cls = _want(samin_ref.cigar, s)
        r = lib.samparse_cigar(s, len(s), ops.ctypes.data, C.byref(n))
        assert _cls(r, lib) == cls, s[:40]
        if cls is None:
            assert [(int(w) >> 4, int(w) & 15) for w in ops[:n.value]] == want, s[:40]


def test_restated_cigar_by_hand():
    assert samin_ref.cigar(b"5M5M") == [(10, 0)] and samin_ref.cigar(b"*") == [] and samin_ref.cigar(b"5M5M3I5M") == [(10, 0), (3, 1), (5, 0)]
    assert samin_ref.cigar(b"1m2=3X") == [(1, 0), (2, 7), (3, 8)]
    for s, cls in ((b"5", "data"), (b"M", "data"), (b"5Q", "data"), (b"2147483648M", "data"), (b"268435455M1M", "unsupported"), (b"1M1I" * 32768, "unsupported")):
        with pytest.raises(samin_ref.SamError) as ei:
            samin_ref.cigar(s)
        assert ei.value.cls == cls, s[:20]


# ---- floats
def _many(lib, tokens):
    text = np.frombuffer(b"".join(tokens) + b"\0", np.uint8)
    off = np.zeros(len(tokens) + 1, np.uint32)
    np.cumsum([len(t) for t in tokens], out=off[1:])
    bits = np.zeros(len(tokens), np.uint32)
    reason = np.zeros(len(tokens), np.uint8)
    lib.samparse_f32_many(text.ctypes.data, off.ctypes.data, len(tokens), bits.ctypes.data, reason.ctypes.data)
    return bits, reason


def _canonical(bits):
    return 0x7FC00000 if (bits & 0x7FFFFFFF) > 0x7F800000 else bits


@pytest.mark.parametrize("bits,text", KAT + SPECIAL)
def test_float_known_answers(lib, bits, text):
    got, reason = _many(lib, [text])
    assert reason[0] == 0 and int(got[0]) == _canonical(bits) == samin_ref.parse_float32(text)


def test_float_a_million_bit_patterns_and_back(lib):
    want = _sample(78, 1 << 20)
    assert want.size > 1000000
    got, reason = _many(lib, [samref.float_text(int(b)) for b in want])
    assert not reason.any()
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, [hex(int(want[k])) for k in bad[:5]]


def _decimal(v):
    """the exact decimal of a Fraction whose denominator is a power of two"""
    k = v.denominator.bit_length() - 1
    assert v.denominator == 1 << k
    digits = str(v.numerator * 5 ** k).rjust(k + 1, "0")
    return (digits[:len(digits) - k] + ("." + digits[len(digits) - k:] if k else "")).encode()


def midpoint_tokens():
    """(token, bits it must give): the midpoints between neighbouring float32 values in [2^-10, 2^20], exactly and one unit of the last
    digit to either side - the midpoint goes to the even mantissa, the others to their side"""
    rng = np.random.default_rng(5)
    out = []
    for e in range(-10, 20):
        for frac in [0, 1, 2, 0x7FFFFE, 0x7FFFFF, 0x400000] + [int(x) for x in rng.integers(0, 1 << 23, 58)]:
            lo = ((e + 127) << 23) | frac
            hi = lo + 1                                     # (behind the last mantissa: the next power of two)
            mid = Fraction(2 * ((1 << 23) | frac) + 1) * (Fraction(2) ** (e - 24))
            tok = _decimal(mid)
            assert len(tok) <= 64 and b"." in tok
            up = tok[:-1] + b"%d" % (int(tok[-1:]) + 1)     # (the last digit of a midpoint is 5)
            down = tok[:-1] + b"%d" % (int(tok[-1:]) - 1)
            out += [(tok, lo if frac % 2 == 0 else hi), (up, hi), (down, lo)]
    return out


def test_float_midpoints_and_the_decimals_next_to_them(lib):
    cases = midpoint_tokens()
    got, reason = _many(lib, [t for t, _ in cases])
    assert not reason.any()
    for (tok, want), g in zip(cases, got):
        assert int(g) == want, tok
    for tok, want in cases[::37]:                           # the restatement agrees (a sample: it is slow)
        assert samin_ref.parse_float32(tok) == want, tok


MAXF = Fraction((1 << 24) - 1) * Fraction(2) ** 104
RANGE = [
    (b"3.4028235e38", 0x7F7FFFFF), (b"340282346638528859811704183484516925440", 0x7F7FFFFF),
    (b"340282356779733661637539395458142568447", 0x7F7FFFFF),          # one below the midpoint to 2^128
    (b"340282356779733661637539395458142568448", None),                # the midpoint: ties to even is 2^128
    (b"3.4028236e38", None), (b"1e39", None), (b"1e40", None), (b"1e400", None), (b"1e99999999999", None), (b"-3.4028236e38", None),
    (b"1e-45", 1), (b"1.4012984643e-45", 1), (b"7.0064923216240853546186479164495806564013097093825788587853e-46", 0),   # 2^-150 cut behind 59 digits: below it
    (b"7.0064923216240853546186479164495806564013097093825788587854e-46", 1), (b"7e-46", 0), (b"1e-46", 0), (b"1e-47", 0), (b"1e-400", 0),
    (b"-1e-400", 0x80000000), (b"1e-99999999999", 0), (b"2.2e-45", 2), (b"2.1e-45", 1),                                   # either side of 1.5 * 2^-149
    (b"1.17549435e-38", 0x00800000), (b"1.1754942e-38", 0x007FFFFF), (b"0", 0), (b"-0", 0x80000000), (b"0e999", 0), (b"0.000", 0), (b"000.5", 0x3F000000),
    (b".5", 0x3F000000), (b"5.", 0x40A00000), (b"5.e0", 0x40A00000), (b"+5", 0x40A00000), (b"5E-1", 0x3F000000), (b"5e+0", 0x40A00000),
    (b"16777217", 0x4B800000), (b"16777219", 0x4B800002), (b"16777216.000000000000000000000000000000000000000000001", 0x4B800000),
    (b"16777217.000000000000000000000000000000000000000000001", 0x4B800001), (b"1" + b"0" * 38, 0x7E967699), (b"0." + b"0" * 44 + b"14", 1),
    (b"inf", 0x7F800000), (b"+Inf", 0x7F800000), (b"-INFINITY", 0xFF800000), (b"Infinity", 0x7F800000), (b"nan", 0x7FC00000), (b"NaN", 0x7FC00000),
]
REFUSED = [(b"", "data"), (b".", "data"), (b"e5", "data"), (b"1e", "data"), (b"1e+", "data"), (b"1.2.3", "data"), (b"1..2", "data"), (b"+", "data"), (b"-", "data"),
           (b"--1", "data"), (b"1 ", "data"), (b" 1", "data"), (b"1f", "data"), (b"infin", "data"), (b"infinit", "data"), (b"infinityx", "data"), (b"in", "data"),
           (b"+nan", "data"), (b"-nan", "data"), (b"nanx", "data"), (b"1e5.0", "data"), (b"1,5", "data"), (b"0x1p-2", "unsupported"), (b"0X1P3", "unsupported"),
           (b"-0x1.8p1", "unsupported"), (b"1_000", "unsupported"), (b"1_0e1_0", "unsupported"), (b"1" * 65, "unsupported"), (b"0." + b"0" * 62 + b"1", "unsupported")]


def test_float_range_ends_and_spellings(lib):
    assert samin_ref.float32_bits(MAXF) == 0x7F7FFFFF
    for tok, want in RANGE:
        ref, cls = _want(samin_ref.parse_float32, tok)
        assert ref == want and (cls is None) == (want is not None), tok
        got, reason = _many(lib, [tok])
        assert _cls(int(reason[0]), lib) == cls, tok
        if want is not None:
            assert int(got[0]) == want, tok


def test_float_refused_spellings(lib):
    for tok, cls in REFUSED:
        _, ref_cls = _want(samin_ref.parse_float32, tok)
        _, reason = _many(lib, [tok])
        assert ref_cls == cls and _cls(int(reason[0]), lib) == cls, tok


def test_array_entries_as_the_reference_reads_them(lib):
    """parseSamNumericArray's types, with its B:s quirk: ParseUint(.., 16) cast to int16"""
    v = C.c_uint32()
    for st, tok, want in ((b"c", b"-128", 0xFFFFFF80), (b"c", b"128", None), (b"C", b"255", 255), (b"C", b"-1", None), (b"s", b"40000", 40000), (b"s", b"-1", None),
                          (b"s", b"65535", 65535), (b"s", b"65536", None), (b"S", b"65535", 65535), (b"i", b"-2147483648", 0x80000000), (b"i", b"2147483648", None),
                          (b"I", b"4294967295", 0xFFFFFFFF), (b"I", b"+1", None), (b"f", b"1.5", 0x3FC00000), (b"f", b"", None), (b"c", b"", None)):
        r = lib.samparse_entry(st[0], tok, len(tok), C.byref(v))
        assert (r == 0) == (want is not None), (st, tok)
        if want is not None:
            assert v.value == want, (st, tok)
    assert struct.unpack("<h", struct.pack("<H", 40000))[0] == -25536


# ---- the token file of the stand-alone (sanitizer) build
def _token_file():
    """[(kind, token, expected line)] - tokens without tab or newline"""
    rows = []
    for bits, signed, tok in int_tokens():
        want, cls = _want(samin_ref.parse_int if signed else samin_ref.parse_uint, tok, bits)
        rows.append(("%s%d" % ("i" if signed else "u", bits), tok, "0 %d" % want if cls is None else "1 0"))
    floats = [(t, b) for t, b in RANGE] + [(t, None) for t, _ in REFUSED] + midpoint_tokens() + [(samref.float_text(int(b)), _canonical(int(b))) for b in _sample(79, 20000)]
    for tok, want in floats:
        rows.append(("f", tok, None if want is None else "0 %08x" % want))
    for s in CIGARS:
        want, cls = _want(samin_ref.cigar, s)
        rows.append(("c", s, None if cls else " ".join(["0"] + ["%x" % ((ln << 4) | op) for ln, op in want])))
    return [r for r in rows if b"\t" not in r[1] and b"\n" not in r[1] and b"\r" not in r[1]]


if __name__ == "__main__":
    rows = _token_file()
    if sys.argv[1] == "write":
        with open(sys.argv[2], "wb") as f:
            f.write(b"".join(kind.encode() + b"\t" + tok + b"\n" for kind, tok, _ in rows))
        print("%d tokens" % len(rows))
    else:
        got = open(sys.argv[3]).read().split("\n")[:len(rows)]
        assert len(got) == len(rows)
        bad = [(k, t[:30], g, w) for (k, t, w), g in zip(rows, got) if (g != w if w is not None else g.split(" ")[0] == "0")]
        assert not bad, bad[:5]
        print("%d results agree" % len(rows))
