"""The hash-derived read sets (tests/md_bloom.py) are what they claim to be.  No GPU: the replica of the key hash, the launch plan
(elprep_amd/csrc/markdup_plan.hpp through tests/markdup_plan_host.cpp) and the oracle.

What is counted is counted from the batch's columns - which records the front pass sends to the table, which bits they announce, which
neighbour pairs hit one - not from the builders' bookkeeping.  That the replica is the device's hash is proved on the device: the retry
of tests/test_gpu_md_bloom.py happens only if every one of the Tm + 1 names reached the table."""
import numpy as np
import pytest

from tests import md_bloom as mb
import oracle as orc
from tests.test_markdup_plan_cpu import _mate, _sizes, lib  # noqa: F401  (the fixture builds the plan's host library)

DUP = 0x400


def test_replica_by_hand():
    """The numpy replica against the formula in Python's own integers, name by name: h0 = 0x9e3779b97f4a7c15 ^ length; per 8-byte
    little-endian word (the last holds only the name's bytes) h = ((h ^ w) * 0xff51afd7ed558ccd + (h >> 29)) mod 2^64; then mix64 with
    library and split at bits 48 and 24.  Names of one word, exactly one, one and a byte, five words, 32 words (the longest of BAM)."""
    M = (1 << 64) - 1

    def mix(x):
        x ^= x >> 30
        x = x * 0xbf58476d1ce4e5b9 & M
        x ^= x >> 27
        x = x * 0x94d049bb133111eb & M
        return x ^ (x >> 31)

    def ref(name, lib, split):
        h = 0x9e3779b97f4a7c15 ^ len(name)
        for k in range(0, len(name), 8):
            h = ((h ^ int.from_bytes(name[k:k + 8], "little")) * 0xff51afd7ed558ccd + (h >> 29)) & M
        return mix(h ^ (lib << 48) ^ (split << 24))

    for name in (b"A", b"abcdefgh", b"abcdefghi", b"x" * 33, b"Tn" + b"q" * 252):
        for lib_, split in ((0, 0), (1, 0), (0, 1), (0xFFFF, 7)):
            assert mb.key_hash(name, lib_, split) == ref(name, lib_, split)
            hi = ref(name, lib_, split) >> 32
            for bw in (1024, 2048):
                assert mb.filter_bit(name, lib_, split, bw) == ((hi >> 5) & (bw - 1)) * 32 + (hi & 31)


# n, bw, tab_cap, T (2 n + 16 rounded up to a power of two), mate_grid (n / 256 rounded up)
PLAN = {
    "full": (8192, 1024, 256, 32768, 32),
    "over": (8194, 1024, 256, 32768, 33),
    "over_split": (8194, 1024, 256, 32768, 33),
    "over_big": (8198, 1024, 256, 32768, 33),
    "over_2048": (24320, 2048, 512, 65536, 95),
}


@pytest.mark.parametrize("name", mb.SETS)
def test_plan(lib, name):  # noqa: F811
    """n_tab = 254 < n / 8: fixed and listed; the first table has 4096 slots, fewer than T; the lists hold more than list_n = 2 x 254 +
    4096 = 4604 members, so k_mate_table (18 workgroups) and k_pair_list_lists (3) go round more than once."""
    rs = mb.read_set(name)
    n, bw, tab_cap, T, mate_grid = PLAN[name]
    on_table, n_tab, _ = mb.table_keys(rs.b, bw)
    assert rs.b.n == n and n_tab == 254 == rs.n_tab
    S = _sizes(lib, n)
    assert (S["T"], S["bw"], S["tab_cap"], S["mate_grid"]) == (T, bw, tab_cap, mate_grid)
    assert rs.bw == bw
    P = _mate(lib, n, n_tab, 0, S["T"])
    assert P == dict(fixed=1, fast=0, listed=1, nfixed=(n + 1) // 2, Tm=mb.TM, list_n=4604)
    assert P["Tm"] < S["T"]
    assert _mate(lib, n, 255, 0, S["T"])["Tm"] == 8192  # (one table record more and the first table doubles)
    listed = sum(k in on_table for k in mb.mate_keys(rs.b))  # two rounds of 18 x 256 and of 3 x 2048 members
    assert 18 * 256 < listed <= 2 * 18 * 256 and 3 * 2048 < listed <= 2 * 3 * 2048
    # the full table (mate_path = 2) takes them all at once
    assert _mate(lib, n, n_tab, 2, S["T"]) == dict(fixed=0, fast=0, listed=0, nfixed=0, Tm=T, list_n=4604)


@pytest.mark.parametrize("name", mb.SETS)
def test_names_on_the_table_path(name):
    """Tm names for `full`, Tm + 1 for the others; every other neighbour pair's bit is not announced (it stays off the table)."""
    rs = mb.read_set(name)
    on_table, n_tab, announced = mb.table_keys(rs.b, rs.bw)
    assert len(on_table) == rs.n_names == (mb.TM if name == "full" else mb.TM + 1)
    assert len(announced) <= 127
    code, bits, keys = mb.classify(rs.b), mb.record_bits(rs.b, rs.bw), mb.mate_keys(rs.b)
    off = [i for i in range(rs.b.n) if code[i] == 2 and keys[i] not in on_table]
    assert all(int(bits[i]) not in announced for i in off)
    assert len(off) == (8063 if name == "over_2048" else 0)
    libs = [k[1] for k in on_table]
    assert min(libs.count(0), libs.count(1)) >= 1900  # about half of the hit names are library 1's
    if name == "over_split":
        splits = [k[0] for k in on_table]
        assert min(splits.count(0), splits.count(1)) >= 2000


@pytest.mark.parametrize("name", mb.SETS)
def test_neighbour_layout(name):
    """the records meant as neighbour pairs are runs of exactly two (leader, follower); everybody else is on the table path"""
    rs = mb.read_set(name)
    code = mb.classify(rs.b)
    ps = rs.pair_starts
    assert np.all(code[ps] == 2) and np.all(code[ps + 1] == 3)
    assert int((code == 1).sum()) == rs.b.n - 2 * len(ps) == rs.n_tab
    assert ps[0] in (126, 127) and np.all(code[:ps[0]] == 1)  # the front: nobody joins a neighbour


def test_lists_filled_to_capacity():
    """Workgroup 0 of k_mate_pairs (records 0 .. 255) is all table-bound: list 0 gets 256 members, tab_cap of the 1024-word sets.  In
    over_2048 workgroup 64 (records 16384 .. 16639) is too and shares list 0: 512 members, tab_cap there; the hit pairs start at record
    16383, across the workgroups' seam."""
    for name in mb.SETS:
        rs = mb.read_set(name)
        on_table = mb.table_keys(rs.b, rs.bw)[0]
        keys = mb.mate_keys(rs.b)
        listed = np.array([k in on_table for k in keys])
        per_wg = np.add.reduceat(listed, np.arange(0, rs.b.n, 256))
        per_list = np.bincount(np.arange(len(per_wg)) % 64, weights=per_wg, minlength=64)
        cap = 512 if name == "over_2048" else 256
        assert per_wg[0] == 256 and per_list[0] == cap and per_list.max() <= cap, name
        if name == "over_2048":
            assert per_wg[64] == 256 and listed[16383] and not listed[16382]
            assert not listed[257:16383].any() and listed[16383:].all()


@pytest.mark.parametrize("name", mb.SETS)
def test_duplicate_share(name):
    rs = mb.read_set(name)
    dup = (rs.expected[0] & DUP) != 0
    pairs = rs.b.n // 2
    assert int(dup.sum()) % 2 == 0  # whole pairs
    assert pairs / 4 <= int(dup.sum()) // 2 <= 3 * pairs / 4, (name, int(dup.sum()) // 2, pairs)


def test_over_big_thirds():
    """four keys of three records, in both arrival orders: third first or between (it pairs with the first end, the other end stays
    alone), third last (the pair stands, it stays alone)"""
    rs = mb.read_set("over_big")
    keys = mb.mate_keys(rs.b)
    where = {}
    for i, k in enumerate(keys):
        where.setdefault(k, []).append(i)
    big = sorted(v for v in where.values() if len(v) > 2)
    assert len(big) == 4 and all(len(v) == 3 for v in big)
    code = mb.classify(rs.b)
    shapes = sorted(tuple(int(code[i]) for i in v) for v in big)
    assert shapes == [(1, 1, 1), (1, 1, 1), (1, 2, 3), (2, 3, 1)]
    assert max(len(v) for v in where.values()) == 3


@pytest.mark.parametrize("bw,target", mb.SEAMS)
def test_seam_set(lib, bw, target):  # noqa: F811
    """one announcement, at exactly the target bit; the oracle's flags are not those of the false-negative outcome"""
    rs, other = mb.seam_set(bw, target), mb.seam_set(bw, target, True)
    b = rs.b
    name = mb.seam_name(bw, target)
    L = mb.SEAM_LENGTHS[mb.SEAMS.index((bw, target)) % 7]
    assert len(name) == L and mb.filter_bit(name, 0, 0, bw) == target
    assert b.n == (45 if bw == 1024 else 16401) and _sizes(lib, b.n)["bw"] == bw
    assert _mate(lib, b.n, 1, 0, _sizes(lib, b.n)["T"])["listed"] == 1
    code, bits = mb.classify(b), mb.record_bits(b, bw)
    assert code.tolist() == [1] + [2, 3] * ((b.n - 1) // 2)
    assert b.qname_of(0) == b.qname_of(b.n - 2) == b.qname_of(b.n - 1) == name
    assert int(bits[0]) == target == int(bits[b.n - 2]) and not np.any(bits[1:b.n - 2] == target)
    on_table, n_tab, announced = mb.table_keys(b, bw)
    assert n_tab == 1 and announced == {target} and len(on_table) == 1
    # (t2, t0) pair up and have a key of their own; under a false negative (t0, t1) do and lose against a
    flags = rs.expected[0]
    assert not (flags[[0, b.n - 2, b.n - 1]] & DUP).any()
    wrong = orc.mark_duplicates(other.b, mb.header())
    assert (wrong[[b.n - 2, b.n - 1]] & DUP).all() and not wrong[0] & DUP
    assert not np.array_equal(flags, wrong)
    assert len(mb.table_keys(other.b, bw)[0]) == 1  # (renamed, t2 is alone on the table)


def test_seam_lengths_cover_every_mask_regime():
    assert {len(mb.seam_name(bw, t)) for bw, t in mb.SEAMS} == set(mb.SEAM_LENGTHS)
