"""The device's QNAME parser and distance test, run on the CPU: elprep_amd/csrc/optical_name.hpp is host-and-device code, and
tests/optical_name_host.cpp builds it with the host compiler, fetching a name's bytes as metrics.hip's tile_info does (six words in front
of the parse for names of up to 48 bytes, a load per eight parsed bytes for longer ones).  Every name of the catalogues of
tests/test_optical_names_cpu.py goes through tile_parse and is compared with the restatement of Go's computeTileInfo
(tests/optical_names.py: go_tile_info); go_abs_diff and optical_close are compared with go_abs / go_close on the edge values."""
import ctypes as C
import os
import subprocess

import pytest

from tests import optical_names as on
from tests import test_optical_names_cpu as cat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tests", "liboptical_name_host.so")
LENGTHS = (0, 47, 48, 49, 56, 57)  # 0: the name as it is; the others pad it: the last word partial, full, one byte into the next


@pytest.fixture(scope="module")
def lib():
    src = os.path.join(ROOT, "tests", "optical_name_host.cpp")
    hdr = os.path.join(ROOT, "elprep_amd", "csrc", "optical_name.hpp")
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", SO, src])
    L = C.CDLL(SO)
    L.on_abs_diff.restype = C.c_longlong
    L.on_abs_diff.argtypes = [C.c_longlong, C.c_longlong]
    return L


def _tile(L, name: bytes):
    out = (C.c_longlong * 4)()
    L.on_tile_info(name, C.c_uint32(len(name)), out)
    return out[0], out[1], out[2], bool(out[3])


def _padded(name: bytes, length: int) -> bytes:
    """the name made `length` bytes long inside its first field (which is never a tile field); as it is if it is longer already"""
    return name if len(name) >= length else b"N" * (length - len(name)) + name


def _check(L, name: bytes):
    for length in LENGTHS:
        nm = _padded(name, length)
        assert length == 0 or len(nm) == max(length, len(name))
        assert _tile(L, nm) == on.go_tile_info(nm), nm


@pytest.mark.parametrize("where", ["x7", "t7", "y7", "x5"])
def test_hand_table(lib, where):
    """Every field of the hand table in the tile, x or y place of a 7-column name, or the x place of a 5-column one."""
    for field in cat.HAND_FIELDS + cat.BAD:
        t, x, y = b"1101", b"-42", b"+0042"
        if where[0] == "t":
            t = field
        elif where[0] == "x":
            x = field
        else:
            y = field
        _check(lib, on.tile_name(1, int(where[1]), t, x, y))


def test_values_at_the_range_ends(lib):
    """±2^63, 2^63 - 1, 18 / 19 / 20 digits and zero-padded values, for their value: the cases of the oracle's test."""
    cases = {b"9223372036854775807": on.I64_MAX, b"-9223372036854775808": on.I64_MIN, b"9223372036854775808": None,
             b"-9223372036854775809": None, b"999999999999999999": 10 ** 18 - 1, b"1000000000000000000": 10 ** 18,
             b"-1000000000000000000": -(10 ** 18), b"10000000000000000000": None, b"0000000000000000000000042": 42,
             b"-000000000000000000000042": -42, b"+000000000000000000000042": 42, b"0000009223372036854775807": on.I64_MAX}
    for f, v in cases.items():
        for length in LENGTHS:
            got = _tile(lib, _padded(b"a:b:1:" + f + b":" + f, length))
            assert got == ((1, v, v, False) if v is not None else (-1, -1, -1, True)), (f, length)
    for v in on.EDGE_VALUES:
        s = b"%d" % v
        assert _tile(lib, b"a:b:" + s + b":" + s + b":" + s) == (v, v, v, False)


@pytest.mark.parametrize("ncol", range(1, 11))
def test_column_counts(lib, ncol):
    """0..9 colons, empty columns, a trailing ':': only 5 and 7 columns are parsed, so a bad field elsewhere does not panic."""
    for body in (b"", b"x", b"7"):
        _check(lib, b":".join([body] * ncol))
    _check(lib, b":".join([b"1"] * (ncol - 1)) + b":" if ncol > 1 else b"")
    _check(lib, on.tile_name(3, ncol, b"12", b"34", b"56"))


def test_names_of_both_load_strategies(lib):
    """tile_name's own padding: names of 47, 48 (six words in front), 49, 56 and 57 bytes (a load per word) with tile fields at the
    edges of the int64 range."""
    for length in (47, 48, 49, 56, 57):
        for ncol in (5, 7):
            nm = on.tile_name(5, ncol, b"-07", b"9223372036854775807", b"+9", length=length)
            assert len(nm) == length and _tile(lib, nm) == (-7, on.I64_MAX, 9, False)
            bad = on.tile_name(5, ncol, b"1101", b"9223372036854775808", b"1", length=length)
            assert len(bad) == length and _tile(lib, bad) == (-1, -1, -1, True)


def test_random_names_sweep(lib):
    """The first 30 000 names of the oracle test's sweep (the same generator and seed), as they are and padded over the 48-byte step."""
    seen = {"short": 0, "long": 0, "panics": 0, "valid": 0}
    for k, (ncol, nm) in enumerate(cat.sweep_names(30_000)):
        if k % 3 == 0:
            nm = _padded(nm, 49 + k % 16)
        want = on.go_tile_info(nm)
        assert _tile(lib, nm) == want, nm
        seen["short" if len(nm) <= 48 else "long"] += 1
        seen["panics"] += want[3]
        seen["valid"] += ncol in (5, 7) and not want[3]
    assert min(seen.values()) > 1000, seen


def test_distance_on_edge_values(lib):
    """go_abs_diff against absInt on Go's wrapping int, and optical_close against isOpticalDuplicate, on every pair of edge values
    (both orders), for the distances of the oracle's test: the difference that wraps, and the one whose absolute value stays MinInt64."""
    tile = (C.c_longlong * 3)
    for a in on.EDGE_VALUES:
        for b in on.EDGE_VALUES:
            assert lib.on_abs_diff(a, b) == on.go_abs(on.wrap64(a - b)), (a, b)
            for dist in cat.DISTS:
                for ta, tb, rga, rgb in ((7, 7, 0, 0), (7, 8, 0, 0), (7, 7, 0, 1), (-1, -1, 0, 0)):
                    want = on.go_close((ta, a, b), (tb, b, a), rga, rgb, dist)
                    assert bool(lib.on_close(tile(ta, a, b), C.c_uint32(rga << 1), tile(tb, b, a), C.c_uint32(rgb << 1), C.c_longlong(dist))) == want
    # the strand is part of the list: the same read group on the other strand is never close
    assert not lib.on_close(tile(7, 0, 0), C.c_uint32(0), tile(7, 0, 0), C.c_uint32(1), C.c_longlong(100))
    assert lib.on_close(tile(7, on.I64_MIN, 0), C.c_uint32(2), tile(7, 0, 0), C.c_uint32(2), C.c_longlong(0))
