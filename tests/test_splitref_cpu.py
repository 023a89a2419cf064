"""tests/splitref.py pinned with hand-written cases (no GPU): the yardstick of tests/test_gpu_split_out.py restates
SplitFilePerChromosome's loop body (sam/split-merge.go:280-293) and its single-end form (:696-707); here every decision of that body is
written out by hand, and the routing is cross-checked against sfm.split_records - the rule the project's host code routes by."""
import struct
from types import SimpleNamespace

import numpy as np

from elprep_amd import sfm
from tests import samref, splitref, tagref

GOF = [1, 1, 2, 3]                 # four contigs in three groups: contigs 0 and 1 share group 1
NAMES = [b"c0", b"c1", b"c2", b"c3"]
G = 3


def rec(refid, nref, fields=(), qname=b"q"):
    """a record without CIGAR, bases and qualities"""
    body = struct.pack("<iiBBHHHIiii", refid, 99 if refid >= 0 else -1, len(qname) + 1, 30, 4680, 0, 0, 0, nref, 199 if nref >= 0 else -1, 0)
    body += qname + b"\0" + b"".join(k + t + v for k, t, v in fields)
    return struct.pack("<I", len(body)) + body


SR1 = (b"sr", b"C", b"\x01")
NM = (b"NM", b"C", b"\x02")
XZ = (b"XZ", b"Z", b"text\0")


def _one(r, single_end=False):
    """the files of a one-record input as {file: [records]} without the empty ones"""
    files = splitref.split_files(r, GOF, G, single_end)
    assert len(files) == (G + 1 if single_end else G + 2)
    return {f: recs for f, recs in enumerate(files) if recs}


def test_rnext_equal_is_never_spread():
    for refid in range(4):
        r = rec(refid, refid, [NM])
        assert _one(r) == {GOF[refid]: [r]}


def test_unmapped_record_with_a_mapped_mate_goes_to_file_0_untagged():
    r = rec(-1, 2, [NM])
    assert _one(r) == {0: [r]}
    r = rec(-1, -1)
    assert _one(r) == {0: [r]}


def test_mapped_record_with_rnext_star_is_spread_and_tagged():
    r = rec(2, -1, [NM])
    assert _one(r) == {2: [rec(2, -1, [NM, SR1])], G + 1: [r]}


def test_mate_on_another_contig_of_the_same_group_is_not_spread():
    r = rec(0, 1, [NM])
    assert _one(r) == {1: [r]}
    r = rec(1, 0)
    assert _one(r) == {1: [r]}


def test_mate_in_another_group_is_spread_and_tagged():
    r = rec(1, 3, [NM, XZ])
    assert _one(r) == {1: [rec(1, 3, [NM, XZ, SR1])], G + 1: [r]}
    r = rec(3, 0)                                     # no optional field at all: the tagged copy has one
    assert _one(r) == {3: [rec(3, 0, [SR1])], G + 1: [r]}


def test_sr_already_present():
    # the first field, a middle field, the last field: replaced in place
    for fields, want in (([SR1, NM, XZ], [SR1, NM, XZ]), ([NM, (b"sr", b"C", b"\x07"), XZ], [NM, SR1, XZ]), ([NM, (b"sr", b"S", b"\x10\x27")], [NM, SR1])):
        got = _one(rec(2, 0, fields))
        assert got[2] == [rec(2, 0, want)]
        assert got[G + 1] == [splitref.written(rec(2, 0, fields))]   # the spread file's record keeps the value it came with
    # twice: Set takes the first, the later one stays as it is
    got = _one(rec(2, 0, [NM, (b"sr", b"C", b"\x05"), XZ, (b"sr", b"C", b"\x09")]))
    assert got[2] == [rec(2, 0, [NM, SR1, XZ, (b"sr", b"C", b"\x09")])]
    # type Z: whatever its type, the entry's value becomes int64(1)
    got = _one(rec(2, 0, [(b"sr", b"Z", b"yes\0"), NM]))
    assert got[2] == [rec(2, 0, [SR1, NM])]
    assert got[G + 1] == [rec(2, 0, [(b"sr", b"Z", b"yes\0"), NM])]
    # a record that is not spread keeps its sr field (a split file that is split again)
    r = rec(2, 2, [NM, (b"sr", b"C", b"\x01")])
    assert _one(r) == {2: [r]}
    # keys one byte off are other keys
    got = _one(rec(2, 0, [(b"sR", b"C", b"\x05"), (b"rs", b"C", b"\x05")]))
    assert got[2] == [rec(2, 0, [(b"sR", b"C", b"\x05"), (b"rs", b"C", b"\x05"), SR1])]


def test_integers_are_re_encoded_in_both_copies():
    fields = [tagref.int_field(b"XN", b"i", -3), tagref.int_field(b"XP", b"i", 300), tagref.int_field(b"sr", b"i", 1)]
    want = [(b"XN", b"c", b"\xfd"), (b"XP", b"S", b"\x2c\x01")]
    got = _one(rec(0, 3, fields))
    assert got[G + 1] == [rec(0, 3, want + [SR1])]    # sr:i:1 read as int64 1, written as type C
    assert got[1] == [rec(0, 3, want + [SR1])]
    got = _one(rec(0, 0, fields))
    assert got == {1: [rec(0, 0, want + [SR1])]}


def test_single_end():
    for refid, nref in ((2, 0), (2, -1), (-1, 1), (1, 1)):
        r = rec(refid, nref, [NM])
        assert _one(r, single_end=True) == {GOF[refid] if refid >= 0 else 0: [r]}   # no spread file, nothing tagged


def test_order_inside_the_files_and_rejected_records():
    recs = [rec(0, 2, qname=b"a"), rec(1, 1, qname=b"b"), rec(-1, -1, qname=b"c"), rec(1, 3, qname=b"d"), rec(2, 2, qname=b"e"), rec(0, 0, qname=b"f")]
    files = splitref.split_files(b"".join(recs), GOF, G)
    assert files[0] == [recs[2]]
    assert files[1] == [rec(0, 2, [SR1], qname=b"a"), recs[1], rec(1, 3, [SR1], qname=b"d"), recs[5]]   # tagged copies among the others
    assert files[2] == [recs[4]] and files[3] == []
    assert files[4] == [recs[0], recs[3]]
    files = splitref.split_files(b"".join(recs), GOF, G, rejected=[0, 4])
    assert files[1] == [recs[1], rec(1, 3, [SR1], qname=b"d"), recs[5]] and files[2] == [] and files[4] == [recs[3]]
    assert splitref.split_bytes(b"".join(recs), GOF, G)[4] == recs[0] + recs[3]


def test_sam_lines_of_the_files():
    r = rec(1, 3, [NM])
    lines = splitref.split_lines(r, GOF, G, NAMES)
    assert lines[1] == b"q\t0\tc1\t100\t30\t*\tc3\t200\t0\t\t\tNM:i:2\tsr:i:1\n"
    assert lines[G + 1] == b"q\t0\tc1\t100\t30\t*\tc3\t200\t0\t\t\tNM:i:2\n"
    assert lines[0] == lines[2] == lines[3] == b""
    assert lines[1] == samref.line(rec(1, 3, [NM, SR1]), NAMES)


def test_routing_equals_sfm_split_records_on_a_random_read_set():
    rng = np.random.default_rng(5)
    n, n_ref, n_groups = 4000, 23, 7
    gof = np.sort(rng.integers(1, n_groups + 1, n_ref)).astype(np.int32)
    refid = rng.integers(-1, n_ref, n).astype(np.int32)
    nref = np.where(rng.random(n) < 0.5, refid, rng.integers(-1, n_ref, n)).astype(np.int32)
    g, spread = sfm.split_records(SimpleNamespace(n=n, refid=refid, next_refid=nref), gof)
    assert spread.sum() > 500 and (~spread).sum() > 500 and (refid < 0).sum() > 50
    recs = [rec(int(r), int(m), qname=b"%d" % i) for i, (r, m) in enumerate(zip(refid, nref))]
    for i, r in enumerate(recs):
        assert splitref.route(r, gof) == (int(g[i]), bool(spread[i])), i
    files = splitref.split_files(b"".join(recs), gof, n_groups)
    for f in range(n_groups + 1):
        want = [rec(int(refid[i]), int(nref[i]), [SR1] if spread[i] else [], qname=b"%d" % i) for i in np.nonzero(g == f)[0]]
        assert files[f] == want, f
    assert files[n_groups + 1] == [recs[i] for i in np.nonzero(spread)[0]]
    single = splitref.split_files(b"".join(recs), gof, n_groups, single_end=True)
    assert single == [[recs[i] for i in np.nonzero(g == f)[0]] for f in range(n_groups + 1)]
