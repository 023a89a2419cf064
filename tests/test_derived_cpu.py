"""CPU test of the context's invalidation table (elprep_amd/csrc/derived.hpp, built by the host compiler through tests/derived_host.cpp):
starting from "everything valid", each event leaves valid exactly the items the header's comment table says.  The expected sets below are
written out by hand from that table, not computed from the code."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tests", "libderived_host.so")

ITEMS = ("keys", "scores", "sample", "apply_recs", "sorted", "sorted_qname", "presort", "marked", "qual_hint", "snapshot", "tile_index", "one_length")
ALL = frozenset(ITEMS)

# event -> what it leaves valid
EXPECTED = {
    "": ALL,
    # count or any column
    "records_changed": frozenset(),
    # MAPQ / CIGAR / has_sr: keys (and the key passes made from them), scores, permutation, marks go; what hangs on QUAL and the offsets stays
    "fixed_fields_changed": frozenset({"qual_hint", "snapshot", "tile_index", "one_length"}),
    # QUAL: the scores with the score kernel's sample and ApplyBQSR's records, and the quality hint - NOT the keys, nor what was made from them
    "qual_changed": frozenset({"keys", "presort", "sorted", "sorted_qname", "marked", "snapshot", "tile_index", "one_length"}),
    # FLAG and QUAL restored from the snapshot: the offsets did not change, the snapshot is still the one to return to
    "flag_qual_restored": frozenset({"snapshot", "tile_index", "one_length"}),
    "split_changed": ALL - {"marked"},
    "radix_timed_out": ALL - {"sorted", "sorted_qname", "marked"},
    "qual_hint_refuted": ALL - {"qual_hint"},
    "header_changed": ALL - {"apply_recs"},
    "score_tuning_changed": ALL - {"scores", "sample", "apply_recs"},
    "hint_tuning_changed": ALL - {"qual_hint"},
    # the stages' own steps
    "adapt_begins": ALL - {"keys", "presort", "scores", "sample", "apply_recs"},
    "drop_sorted": ALL - {"sorted", "sorted_qname"},
    "set_sorted_coordinate": ALL - {"sorted_qname"},
    "drop_marked": ALL - {"marked"},
    "drop_presort": ALL - {"presort"},
}


@pytest.fixture(scope="module")
def lib():
    src = os.path.join(ROOT, "tests", "derived_host.cpp")
    hdr = os.path.join(ROOT, "elprep_amd", "csrc", "derived.hpp")
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", SO, src])
    L = C.CDLL(SO)
    L.derived_valid_after.restype = C.c_uint32
    L.derived_valid_after.argtypes = [C.c_char_p]
    return L


def _valid_after(L, event):
    m = L.derived_valid_after(event.encode())
    assert m != 0xFFFFFFFF, "unknown event " + event
    return frozenset(name for k, name in enumerate(ITEMS) if m >> k & 1)


@pytest.mark.parametrize("event", sorted(EXPECTED))
def test_event_leaves_valid_what_the_table_says(lib, event):
    got = _valid_after(lib, event)
    assert got == EXPECTED[event], "%s: unexpectedly valid %s, unexpectedly cleared %s" % (
        event or "(start)", sorted(got - EXPECTED[event]), sorted(EXPECTED[event] - got))


def test_qual_changed_keeps_the_keys(lib):
    """what lets a coordinate sort run behind elp_bqsr_apply - or beside it, on a thread of its own - without entering the adapt stage"""
    got = _valid_after(lib, "qual_changed")
    assert "keys" in got and "scores" not in got


def test_records_changed_leaves_nothing_valid(lib):
    assert _valid_after(lib, "records_changed") == frozenset()


def test_unknown_event_is_reported(lib):
    assert lib.derived_valid_after(b"no_such_event") == 0xFFFFFFFF
