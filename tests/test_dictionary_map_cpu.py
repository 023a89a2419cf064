"""CPU test of elp_host_dictionary_map (include/elprep_host.h): the host half of --replace-reference-sequences.  Every case is written
out by hand from the reference's two loops - filters/simple-filters.go:208-231 (AddREFID: dictTable[SN] = index, later entries of a name
overwrite earlier ones) for the map, :36-51 (ReplaceReferenceSequenceDictionary: utils.Find = the FIRST old entry of the name; entries not
found are skipped; the first found position that does not ascend sets SO to unknown and ends the walk) for the order verdict."""
import ctypes as C

import numpy as np
import pytest

from elprep_amd import _lib
from elprep_amd.engine import dictionary_map

CASES = [
    # (what, old names, new names, new_of_old, order_kept, the lines it follows)
    ("identity", ["1", "2", "X"], ["1", "2", "X"], [0, 1, 2], True, ":211-213 index of each name; :43-44 pos 0 < 1 < 2"),
    ("reversed", ["1", "2", "X"], ["X", "2", "1"], [2, 1, 0], False, ":42-48 pos 2, then 1 <= 2: unknown"),
    ("subset in order", ["1", "2", "3", "X"], ["2", "X"], [-1, 0, -1, 1], True, ":215-218 not found = -1; pos 1 < 3"),
    ("new contigs in front and in between", ["1", "2", "X"], ["d0", "1", "d1", "2", "d2", "X"], [1, 3, 5], True,
     ":42 pos < 0 is skipped; the found ones 0 < 1 < 2 ascend"),
    ("a name twice in the new dictionary", ["1", "2"], ["2", "1", "2"], [1, 2], False,
     ":211-213 the LAST index of '2' wins (2, not 0); walk: pos 1, then 0 <= 1: unknown"),
    ("a name twice in the new dictionary, in order", ["1", "2"], ["1", "1", "2"], [1, 2], False,
     "last index of '1' is 1; walk: pos 0, then 0 again - not GREATER (:43): unknown"),
    ("a name twice in the old dictionary", ["1", "2", "1"], ["1", "2"], [0, 1, 0], True,
     "both old ids of '1' map to new 0; utils.Find takes the first old entry: pos 0 < 1"),
    ("a name twice in the old one, second copy would break the order", ["2", "1", "2"], ["1", "2"], [1, 0, 1], False,
     "Find('1') = 1, Find('2') = 0 (the first, not 2): 0 <= 1: unknown"),
    ("an order violation behind a break point", ["1", "2", "3", "4"], ["1", "3", "2", "4"], [0, 2, 1, 3], False,
     "pos 0, 2, then 1 <= 2: unknown and break (:46-47) - the ascending '4' behind it does not matter"),
    ("only the entries behind the break ascend", ["1", "2", "3"], ["2", "1", "3"], [1, 0, 2], False, "pos 1, then 0 <= 1: unknown"),
    ("disjoint dictionaries", ["1", "2"], ["a", "b", "c"], [-1, -1], True, "no entry is found: previousPos is never compared"),
    ("empty new dictionary", ["1", "2"], [], [-1, -1], True, "both loops make no step"),
    ("empty old dictionary", [], ["1", "2"], [], True, "Find finds nothing"),
    ("both empty", [], [], [], True, ""),
    ("names that are prefixes of each other", ["chr1", "chr10", "chr"], ["chr", "chr1", "chr10"], [1, 2, 0], False,
     "whole names compare; pos 2, then 0 <= 2: unknown"),
    ("an empty name", ["", "1"], ["1", ""], [1, 0], False, "SN '' is a map key like any other"),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_dictionary_map_case(case):
    what, old, new, want_map, want_kept, why = case
    got_map, got_kept = dictionary_map(old, new)
    assert got_map.dtype == np.int32 and got_map.tolist() == want_map, (what, why)
    assert got_kept is want_kept, (what, why)


def test_dictionary_map_takes_bytes_and_str_alike():
    a = dictionary_map([b"chrA", "chrB"], ["chrB", b"chrA"])
    assert a[0].tolist() == [1, 0] and a[1] is False


def _raw_call(old_cat, old_off, n_old, new_cat, new_off, n_new, out, kept):
    return _lib.host().elp_host_dictionary_map(old_cat, old_off, n_old, new_cat, new_off, n_new, out, kept)


def test_dictionary_map_c_abi_edges():
    """order_kept_out may be NULL; negative counts, missing arrays and decreasing offsets are refused with -1 and write nothing"""
    names = np.frombuffer(b"abc", dtype=np.uint8)
    off = np.asarray([0, 1, 2, 3], dtype=np.uint32)
    out = np.full(3, 7, dtype=np.int32)
    vp = lambda a: C.c_void_p(a.ctypes.data)
    assert _raw_call(vp(names), vp(off), 3, vp(names), vp(off), 3, vp(out), None) == 0
    assert out.tolist() == [0, 1, 2]
    out[:] = 7
    kept = C.c_int(5)
    assert _raw_call(vp(names), vp(off), -1, vp(names), vp(off), 3, vp(out), C.byref(kept)) == -1
    assert _raw_call(vp(names), vp(off), 3, vp(names), vp(off), -1, vp(out), C.byref(kept)) == -1
    assert _raw_call(vp(names), C.c_void_p(0), 3, vp(names), vp(off), 3, vp(out), C.byref(kept)) == -1
    assert _raw_call(vp(names), vp(off), 3, vp(names), vp(off), 3, C.c_void_p(0), C.byref(kept)) == -1
    bad = np.asarray([0, 2, 1, 3], dtype=np.uint32)
    assert _raw_call(vp(names), vp(bad), 3, vp(names), vp(off), 3, vp(out), C.byref(kept)) == -1
    assert out.tolist() == [7, 7, 7] and kept.value == 5


def test_dictionary_map_of_a_large_dictionary():
    """hg38 with alts has 3366 contigs: every name found through the table, not by a scan per name that a test would wait for"""
    old = ["ctg%d" % k for k in range(3366)]
    new = old[::2]
    m, kept = dictionary_map(old, new)
    assert kept is True
    assert m[::2].tolist() == list(range(1683)) and (m[1::2] == -1).all()
