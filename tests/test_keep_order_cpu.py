"""CPU tests around elp_order_keep and the merge of unsorted splits: the entry points exist and refuse NULL contexts, the validity rules of
a keep permutation (elprep_amd/csrc/derived.hpp through tests/derived_keep_host.cpp), and the numpy / Batch restatements the GPU tests
compare against (tests/keep_ref.py, sfm.merge_splits_unsorted) on hand-written cases whose expected order is written out here."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from elprep_amd import _lib, sfm
from elprep_amd.batch import batch_from_records
from tests import keep_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tests", "libderived_keep_host.so")
NEW = ("elp_order_keep", "elp_emit_merged_bgzf", "elp_emit_concat_bam", "elp_emit_concat_bgzf")


# ---- the entry points
def test_the_four_entry_points_are_exported_and_listed():
    L = _lib.hip()
    for name in NEW:
        assert hasattr(L, name), name
        assert name in _lib.HIP_SYMBOLS, name


def test_the_new_entry_points_reject_null_contexts_without_a_gpu():
    """argument checks come in front of any device call: a NULL context is an error code, not a crash"""
    L = _lib.hip()
    null = C.c_void_p(0)
    n = C.c_uint64(0)
    assert L.elp_order_keep(null, 0) != 0 and L.elp_order_keep(null, 1) != 0
    for name in NEW[1:]:
        assert getattr(L, name)(null, null, null, 0, C.byref(n)) != 0, name


def test_the_no_permutation_messages_name_the_third_call():
    for src in ("ctx.hip", "emit.hip"):
        text = open(os.path.join(ROOT, "elprep_amd", "csrc", src)).read()
        assert "or elp_sort_queryname first" not in text
        assert "elp_sort_coordinate, elp_sort_queryname or elp_order_keep first" in text


def test_the_seam_sizes_of_the_gpu_tests_are_the_sources():
    import re
    src = lambda f: open(os.path.join(ROOT, "elprep_amd", "csrc", f)).read()
    assert int(re.search(r"constexpr uint32_t KEEP_W = (\d+);", src("keep.hip")).group(1)) == keep_ref.KEEP_W
    assert int(re.search(r"constexpr uint32_t MERGE_CHECK_W = (\d+);", src("split_merge.hip")).group(1)) == keep_ref.MERGE_CHECK_W
    radix = src("radix.hip")
    assert "constexpr int SCAN_TILE = 256 * SCAN_ITEMS;" in radix
    assert 256 * int(re.search(r"constexpr int SCAN_ITEMS = (\d+);", radix).group(1)) == keep_ref.SCAN_TILE


# ---- derived.hpp: what drops a keep permutation
ITEMS = ("sorted", "sorted_qname", "sorted_keep", "sorted_keep_by_split", "marked", "keys")
KEEP = frozenset({"sorted", "sorted_keep"})
KEEP_SPLIT = frozenset({"sorted", "sorted_keep", "sorted_keep_by_split"})
OTHER = frozenset({"marked", "keys"})

# event -> the permutation items it leaves, from a plain keep permutation and from one made by split; the two other items show that
# the event is the one meant.  Written out from the table at the top of derived.hpp.
AFTER = {
    "": (KEEP | OTHER, KEEP_SPLIT | OTHER),
    "records_changed": (frozenset(), frozenset()),
    "fixed_fields_changed": (frozenset(), frozenset()),          # has_sr: what the order was made from
    "flag_qual_restored": (frozenset(), frozenset()),
    "dictionary_replaced": (frozenset(), frozenset()),           # record states change
    "duplicate_bit_cleared": (frozenset({"keys"}), frozenset({"keys"})),  # conservative: every kind of permutation goes
    "radix_timed_out": (frozenset({"keys"}), frozenset({"keys"})),
    "drop_sorted": (OTHER, OTHER),
    "qual_changed": (KEEP | OTHER, KEEP_SPLIT | OTHER),          # drops nothing of it
    "split_changed": (KEEP | {"keys"}, frozenset({"keys"})),     # only the order that was made from the split ids
    "qual_hint_refuted": (KEEP | OTHER, KEEP_SPLIT | OTHER),
    "header_changed": (KEEP | OTHER, KEEP_SPLIT | OTHER),
    "score_tuning_changed": (KEEP | OTHER, KEEP_SPLIT | OTHER),
    "hint_tuning_changed": (KEEP | OTHER, KEEP_SPLIT | OTHER),
    "adapt_begins": (KEEP | {"marked"}, KEEP_SPLIT | {"marked"}),
    # the kinds replace each other
    "set_sorted_coordinate": (frozenset({"sorted"}) | OTHER,) * 2,
    "set_sorted_queryname": (frozenset({"sorted", "sorted_qname"}) | OTHER,) * 2,
    "set_sorted_keep": (KEEP | OTHER,) * 2,
    "set_sorted_keep_by_split": (KEEP_SPLIT | OTHER,) * 2,
}


@pytest.fixture(scope="module")
def lib():
    src = os.path.join(ROOT, "tests", "derived_keep_host.cpp")
    hdr = os.path.join(ROOT, "elprep_amd", "csrc", "derived.hpp")
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", SO, src])
    L = C.CDLL(SO)
    L.derived_keep_after.restype = C.c_uint32
    L.derived_keep_after.argtypes = [C.c_char_p, C.c_char_p]
    return L


def _after(L, start, event):
    m = L.derived_keep_after(start.encode(), event.encode())
    assert m != 0xFFFFFFFF, (start, event)
    return frozenset(name for k, name in enumerate(ITEMS) if m >> k & 1)


@pytest.mark.parametrize("event", sorted(AFTER))
def test_event_on_a_keep_permutation(lib, event):
    assert _after(lib, "keep", event) == AFTER[event][0], "plain"
    assert _after(lib, "keep_by_split", event) == AFTER[event][1], "by split"


def test_a_sort_clears_the_keep_bits_and_keep_clears_queryname(lib):
    for start in ("keep", "keep_by_split"):
        assert _after(lib, start, "set_sorted_coordinate") & KEEP_SPLIT == {"sorted"}
        assert _after(lib, start, "set_sorted_queryname") & (KEEP_SPLIT | {"sorted_qname"}) == {"sorted", "sorted_qname"}
    for ev in ("set_sorted_keep", "set_sorted_keep_by_split"):
        assert "sorted_qname" not in _after(lib, "queryname", ev)
        assert "sorted_keep" in _after(lib, "coordinate", ev)


def test_split_changed_leaves_the_sorts_permutations(lib):
    """elp_split_classify rewrites the split column: only the order made from it goes (tests/test_derived_cpu.py: queryname stays)"""
    assert {"sorted", "sorted_qname"} <= _after(lib, "queryname", "split_changed")
    assert "sorted" in _after(lib, "coordinate", "split_changed")
    assert "sorted" in _after(lib, "keep", "split_changed")
    assert "sorted" not in _after(lib, "keep_by_split", "split_changed")


def test_unknown_names_are_reported(lib):
    assert lib.derived_keep_after(b"keep", b"no_such_event") == 0xFFFFFFFF
    assert lib.derived_keep_after(b"no_such_start", b"") == 0xFFFFFFFF


# ---- the restatements, on hand-written cases
def test_keep_order_by_hand():
    #        0  1  2  3  4  5  6  7
    state = [0, 1, 0, 2, 0, 0, 1, 0]
    perm, n_out = keep_ref.keep_order(state)
    assert n_out == 5 and perm.dtype == np.uint32
    assert perm.tolist() == [0, 2, 4, 5, 7, 1, 3, 6]


def test_keep_order_by_split_by_hand():
    #        0  1  2  3  4  5  6  7  8
    state = [0, 0, 1, 0, 2, 0, 0, 1, 0]
    split = [3, 0, 0, 1, 1, 3, 0, 3, 1]
    perm, n_out = keep_ref.keep_order(state, split, by_split=True)
    assert n_out == 6
    # output: split 0 (1, 6), split 1 (3, 8), split 3 (0, 5); not output: split 0 (2), split 1 (4), split 3 (7)
    assert perm.tolist() == [1, 6, 3, 8, 0, 5, 2, 4, 7]
    # ids that descend in staging order, every record output: the split files in id order, staging order inside
    perm, _ = keep_ref.keep_order([0] * 6, [2, 2, 1, 1, 0, 0], by_split=True)
    assert perm.tolist() == [4, 5, 2, 3, 0, 1]
    # one id: staging order
    assert keep_ref.keep_order([0, 2, 0], [7, 7, 7], by_split=True)[0].tolist() == [0, 2, 1]
    assert keep_ref.keep_order([], [], by_split=True)[0].tolist() == [] and keep_ref.keep_order([])[1] == 0


def test_concat_stream_by_hand():
    #          0  1  2  3  4  5  6
    g_state = [0, 0, 1, 0, 0, 2, 0]
    g_split = [2, 0, 2, 1, 0, 1, 2]
    s_state = [0, 1, 0]
    got = keep_ref.concat_stream(g_state, g_split, s_state)
    assert got == [("g", 1), ("g", 4),            # the unmapped file
                   ("s", 0), ("s", 2),            # the spread file
                   ("g", 3), ("g", 0), ("g", 6)]  # group files 1, 2
    # no unmapped file, no spread
    assert keep_ref.concat_stream([0, 0, 0], [2, 1, 1], []) == [("g", 1), ("g", 2), ("g", 0)]
    assert keep_ref.concat_stream([1], [0], [0, 0]) == [("s", 0), ("s", 1)]


def _names(b):
    return [b.qname_of(i).decode() for i in range(b.n)]


def test_merge_splits_unsorted_by_hand():
    """MergeUnsortedFilesSplitPerChromosome: the unmapped file, the spread file, the group files in index order - each as it is"""
    g1 = batch_from_records([dict(qname="g1b", refid=0, pos=90, flag=0), dict(qname="g1a", refid=0, pos=10, flag=16)])
    g2 = batch_from_records([dict(qname="g2a", refid=2, pos=5, flag=0), dict(qname="g2c", refid=1, pos=7, flag=0), dict(qname="g2b", refid=1, pos=7, flag=0)])
    sp = batch_from_records([dict(qname="s2", refid=1, pos=50, flag=0), dict(qname="s1", refid=0, pos=1, flag=0)])
    un = batch_from_records([dict(qname="u2", flag=4), dict(qname="u1", flag=4)])
    out = sfm.merge_splits_unsorted([g1, g2], sp, un)
    assert _names(out) == ["u2", "u1", "s2", "s1", "g1b", "g1a", "g2a", "g2c", "g2b"]
    assert out.pos.tolist() == [0, 0, 50, 1, 90, 10, 5, 7, 7] and out.flag.tolist() == [4, 4, 0, 0, 0, 16, 0, 0, 0]
    # empty parts
    none = un.take(np.zeros(0, np.int64))
    assert _names(sfm.merge_splits_unsorted([g1], none, none)) == ["g1b", "g1a"]
    assert _names(sfm.merge_splits_unsorted([], sp, un)) == ["u2", "u1", "s2", "s1"]
    # the sorted merge of the same (sorted) files differs: it interleaves the spread reads and puts the unmapped file last
    g1s, g2s, sps = g1.take([1, 0]), g2.take([1, 2, 0]), sp.take([1, 0])
    assert _names(sfm.merge_splits([g1s, g2s], sps, un)) == ["s1", "g1a", "g1b", "g2c", "g2b", "s2", "g2a", "u2", "u1"]


def test_sfm_step_takes_an_order_argument():
    import inspect
    for fn in (sfm.SfmRank.step, sfm.SfmRank.emit_merged):
        assert inspect.signature(fn).parameters["order"].default == "coordinate"
    with pytest.raises(ValueError):
        sfm._order_call(None, "queryname")
