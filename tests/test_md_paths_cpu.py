"""The path read sets (tests/md_paths.py) are what they claim to be: their sizes, their mates' places, and at least one duplicate pair in
each - a path whose expected flags are all clear proves nothing.  Oracle only, no GPU."""
import numpy as np
import pytest

from tests import md_paths as mp

DUP = 0x400
SIZES = dict(fast=8, below_the_cut=6, listed=130, big_group=5, one_bucket=766, two_buckets=768)


@pytest.mark.parametrize("name", list(mp.RECORDS))
def test_size_and_duplicates(name):
    rs = mp.read_set(name)
    assert rs.b.n == SIZES[name]
    dup = (rs.expected[0] & DUP) != 0
    assert dup.any() and not dup.all()
    assert int(dup.sum()) % 2 == 0  # whole pairs


def _names(b):
    return [bytes(b.qname[b.qname_off[i]:b.qname_off[i + 1]]) for i in range(b.n)]


@pytest.mark.parametrize("name", ["fast", "below_the_cut", "one_bucket", "two_buckets"])
def test_adjacent_sets_are_runs_of_exactly_two(name):
    nm = _names(mp.read_set(name).b)
    assert all(nm[i] == nm[i + 1] for i in range(0, len(nm), 2)) and len(set(nm)) == len(nm) // 2


def test_listed_set_has_two_records_off_the_neighbour_path():
    """everybody but the x pair stands next to its mate; the x records stand 41 apart between whole pairs and are flagged through the table"""
    rs = mp.read_set("listed")
    nm = _names(rs.b)
    lo, hi = mp.SEPARATED_AT
    assert nm[lo] == nm[hi] == b"x" and nm.count(b"x") == 2 and hi - lo - 1 == 40
    rest = [s for s in nm if s != b"x"]
    assert all(rest[i] == rest[i + 1] for i in range(0, len(rest), 2)) and len(set(rest)) == 64
    assert nm[lo - 1] == nm[lo - 2] and nm[hi - 1] == nm[hi - 2]  # (neither splits a pair)
    assert 2 < rs.b.n // 8  # two table records are below the cut n / 8: the fixed-slot path with lists
    dup = (rs.expected[0] & DUP) != 0
    assert dup[lo] and dup[hi]


def test_big_group_is_three_records_of_one_name():
    rs = mp.read_set("big_group")
    assert _names(rs.b) == [b"a", b"a", b"t", b"t", b"t"]
    assert np.nonzero(rs.expected[0] & DUP)[0].tolist() == [2, 3]
