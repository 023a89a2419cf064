"""The seam read sets (tests/md_seams.py) are what they claim to be: every record of a motif at every phase of the front pass's workgroup,
same-name neighbours across every seam, and duplicate flags of both kinds everywhere the device test looks.  Oracle only, no GPU."""
import os
import re

import numpy as np
import pytest

from tests import kat_cases, md_seams as ms

DUP = 0x400
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _csrc(name):
    with open(os.path.join(ROOT, "elprep_amd", "csrc", name)) as f:
        return f.read()


def test_geometry_constants_are_the_kernels():
    src = _csrc("markdup_plan.hpp")  # (the constants the launch plan shares with the kernels)
    assert re.search(r"MF_THREADS = 320, MF_RECS = (\d+);", src).group(1) == str(ms.WG)
    assert re.search(r"MAX_QNAME = (\d+);", _csrc("common.hpp")).group(1) == str(ms.MAX_QNAME) == str(ms.LENGTHS[-1])
    for motif, (p, _) in ms.MOTIFS.items():
        assert np.gcd(p, ms.WG) == 1, motif
        named = sorted(s for v in ms.SLOTS[motif].values() for s in v)
        assert named == [s for s in range(p) if (motif, s) != ("announced", 8)]  # (that slot holds a fragment or a third record)


def test_names_have_their_length_and_differ_where_they_should():
    for L in ms.LENGTHS:
        a, b, c = ms.qname(10, L), ms.qname(11, L), ms.qname(12, L)
        assert len(a) == len(b) == len(c) == L and len({a, b, c}) == 3
        assert a[:-1] == b[:-1]  # twins: the last byte only
        if L >= 40:
            assert a[:32] == c[:32]  # only the loop behind the four masked words tells them apart
        if L > 4:
            r = ms.qname(10, L, first="R")
            assert r[1:] == a[1:] and r[0] != a[0]


@pytest.mark.parametrize("motif", list(ms.MOTIFS))
def test_every_record_at_every_phase_and_both_outcomes(motif):
    p, _ = ms.MOTIFS[motif]
    slots = ms.SLOTS[motif]
    for L in ms.LENGTHS:
        rs = ms.read_set(motif, L)
        b = rs.b
        assert b.n == p * ms.WG <= 3432
        ql = (b.qname_off[1:] - b.qname_off[:-1]).astype(np.int64)
        assert (ql == L).all()
        ph = ms.phases(b.n)
        slot = np.arange(b.n) % p
        for s in range(p):  # every record of the motif once at every phase (and so at both parities: 312 is even, p is odd)
            assert sorted(ph[slot == s].tolist()) == list(range(ms.WG)), (L, s)
            assert set((np.nonzero(slot == s)[0] & 1).tolist()) == {0, 1}
        names = [b.qname_of(i) for i in range(b.n)]
        if motif in ("triple", "quad"):
            # every pair of neighbouring same-name records of the run across the workgroup seam and every wave seam, in the kernel's u
            # (phase + 2) and - it costs nothing - in phases
            for s in slots["run"][:-1]:
                left = np.nonzero(slot == s)[0]
                assert all(names[i] == names[i + 1] for i in left), (L, s)
                at = set(ph[left].tolist())
                assert ms.WG - 1 in at
                assert {u - 2 for u in ms.WAVE_SEAMS_U} <= at and set(ms.WAVE_SEAMS_U) <= at
        flags = rs.expected[0]
        dup = (flags & DUP) != 0
        assert np.array_equal(flags & ~np.uint16(DUP), b.flag)
        for kind, ss in slots.items():  # pairs, fragments, the same-name run: some flagged, some not, each on its own
            sel = np.isin(slot, ss)
            assert dup[sel].any() and (~dup[sel]).any(), (L, kind)
        if motif == "announced":
            sel = (slot == 8) & ((np.arange(b.n) // p) % 3 == 0)  # its fragments share a slot with the third records
            assert dup[sel].any() and (~dup[sel]).any(), L
        edge = np.isin(ph, (0, 1, 2, 3, ms.WG - 2, ms.WG - 1))
        assert dup[edge].any() and (~dup[edge]).any(), L
        if motif == "plain":
            f0 = np.nonzero((slot == 2) & ((np.arange(b.n) // p) % 4 == 0))[0]
            assert dup[f0].all()  # a fragment on the key of a pair's end is a duplicate (classifyFragment)
        if motif == "announced":
            # the third record of a name is 1000 or more records from its pair
            where = {}
            for i in np.nonzero(slot >= 8)[0]:
                where.setdefault(names[i], []).append(int(i))
            far = [v for v in where.values() if len(v) == 3]
            assert len(far) >= 200
            for v in far:
                third = [i for i in v if i % p == 8][0]
                assert min(abs(third - i) for i in v if i != third) >= 1000


def test_triple_and_quad_open_with_the_toggling_cases():
    """the first two repetitions of motifs 2 and 3 carry kat_cases.toggling_cases' records: the flags derived by hand there"""
    cases = kat_cases.toggling_cases()
    assert [c[1] for c in cases] == [[2, 3], [], [2, 3], [], [2, 3]]  # a0 a1 t0 t1 ..: (t0, t1) lose against a, or (t2, t0) have their own key
    for L in ms.LENGTHS:
        d = (ms.read_set("triple", L).expected[0] & DUP) != 0
        # r = 0: t0 t1 t2 a0 a1 | pair;  r = 1: t2 t0 t1 | pair pair
        assert d[:5].tolist() == [True, True, False, False, False], L
        assert d[7:10].tolist() == [False, False, False], L
        d = (ms.read_set("quad", L).expected[0] & DUP) != 0
        # r = 0: t0 t1 t2 t1' a0 a1 f;  r = 1 (contig 1): t2 t1' t0 t1 a0 a1 f
        assert d[:7].tolist() == [True, True, False, False, False, False, False], L
        assert d[7:14].tolist() == [False, False, True, True, False, False, False], L


def test_short_names_and_prefixes():
    for L in ms.SHORT_LENGTHS:
        for s in ms.SHORT_SLIDES:
            b = ms.short_set(L, s).b
            assert ((b.qname_off[1:] - b.qname_off[:-1]) == L).all()
            cand = np.nonzero((b.flag & 0x1) != 0)[0]
            names = [b.qname_of(i) for i in cand]
            assert all(names.count(nm) == 2 for nm in set(names[:40])) and len(set(names)) * 2 == len(names)
            assert cand[0] == s and b.n == s + 5 * (46 if L == 1 else 90)
        d = (ms.short_set(L, 0).expected[0] & DUP) != 0
        assert d.any() and not d.all()
    # the pairs' first records pass the workgroup seam at both parities over the slides
    first = {(s + 5 * r + k) % ms.WG for s in ms.SHORT_SLIDES for r in range(46) for k in (0, 3)}
    assert {ms.WG - 1, 0, ms.WG - 2, 1} <= first
    full = ms.read_set("plain", ms.PREFIX_L).b
    for n in ms.PREFIX_NS:
        b = ms.prefix_set(n).b
        assert b.n == n and np.array_equal(b.flag, full.flag[:n]) and np.array_equal(b.qname, full.qname[:n * ms.PREFIX_L])
    assert ms.prefix_set(626).b.qname_of(625) != ms.prefix_set(626).b.qname_of(624)  # 625 = 5 * 125: a pair's first end, cut from its mate
    assert ms.prefix_set(625).b.qname_of(624) == ms.prefix_set(625).b.qname_of(623)
