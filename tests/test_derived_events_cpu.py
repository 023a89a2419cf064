"""CPU test of the events of the context's invalidation table (elprep_amd/csrc/derived.hpp) that came after tests/test_derived_cpu.py:
starting from "everything valid", each leaves valid exactly what the header's comment table says.  The expected sets are written out by
hand from that table."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tests", "libderived_events_host.so")
ITEMS = ("keys", "scores", "sample", "apply_recs", "sorted", "sorted_qname", "presort", "marked", "qual_hint", "snapshot", "tile_index", "one_length")
ALL = frozenset(ITEMS)

EXPECTED = {
    "": ALL,
    # REFID / RNEXT / has_sr / n_ref: what fixed_fields_changed and header_changed spoil, and the snapshot (a rollback cannot restore refids);
    # what hangs on QUAL and the offsets stays
    "dictionary_replaced": frozenset({"qual_hint", "tile_index", "one_length"}),
    # FLAG's duplicate bit: the marks and any permutation - NOT keys, key passes made ahead, scores
    "duplicate_bit_cleared": ALL - {"sorted", "sorted_qname", "marked"},
}


@pytest.fixture(scope="module")
def lib():
    src = os.path.join(ROOT, "tests", "derived_events_host.cpp")
    hdr = os.path.join(ROOT, "elprep_amd", "csrc", "derived.hpp")
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", SO, src])
    L = C.CDLL(SO)
    L.derived_events_valid_after.restype = C.c_uint32
    L.derived_events_valid_after.argtypes = [C.c_char_p]
    return L


@pytest.mark.parametrize("event", sorted(EXPECTED))
def test_event_leaves_valid_what_the_table_says(lib, event):
    m = lib.derived_events_valid_after(event.encode())
    assert m != 0xFFFFFFFF
    got = frozenset(name for k, name in enumerate(ITEMS) if m >> k & 1)
    assert got == EXPECTED[event], (sorted(got - EXPECTED[event]), sorted(EXPECTED[event] - got))


def test_dictionary_replaced_spoils_what_its_two_parents_spoil(lib):
    got = lib.derived_events_valid_after(b"dictionary_replaced")
    for item in ("keys", "presort", "scores", "sorted", "marked", "apply_recs", "snapshot"):
        assert not got >> ITEMS.index(item) & 1, item
