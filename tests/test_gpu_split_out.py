"""GPU tests (-m gpu) of the split files written on the device: elp_emit_split_bam, elp_emit_split_bgzf, elp_emit_split_sam
(Engine.emit_split, sfm.split_files_device).

The expected bytes are tests/splitref.py's files - SplitFilePerChromosome's loop body (sam/split-merge.go:280-293) and its single-end form
(:696-707) restated on BAM record bytes, pinned by tests/test_splitref_cpu.py - of the oracle's BAM records; the SAM form is
tests/samref.py's lines of the same records.  Every comparison is of bytes.

Two refusals of include/elprep_hip.h's list have no test: more than 2^31-16 staged records (two thousand million records), and malformed
optional fields (ELP_ERR_DATA) - staging refuses such records, so no staged context holds one."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest

import oracle as orc
from elprep_amd import sfm
from elprep_amd.batch import Batch
from elprep_amd.engine import ElpError, Engine
from tests import splitref, tagref
from tests.common import dataset
from tests.test_gpu_round4 import _members
from tests.test_gpu_tag_filters import _one_group_header

pytestmark = pytest.mark.gpu

ELP_ERR_ARG, ELP_ERR_UNSUPPORTED = -1, -5
# the three contigs of the "tiny" genome in n_groups groups: 1 = one group file (only RNEXT "*" spreads), 2 = two contigs share a group,
# 17 = every contig its own group, 300 = the file id needs the second radix pass (group files 256 and 300, n_files = 302)
GOF = {1: [1, 1, 1], 2: [1, 1, 2], 3: [1, 3, 3], 17: [3, 17, 9], 300: [256, 300, 7]}
COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 3000]   # every wavefront and workgroup seam of the list kernels; 3000 records
                                                                  # are 6000 slots: more than one radix tile of 4096 keys


def _with(b, **cols):
    c = {name: getattr(b, name) for name in b.__dataclass_fields__}
    c.update(cols)
    return Batch(**c)


@functools.lru_cache(maxsize=None)
def _reads(mix):
    """>= 3000 records of the tiny genome whose RNEXT is rewritten: "mixed" - about every third record gets a random mate contig or "*";
    "all" - mapped records only, every mate on the next contig; "none" - every mate on the record's own contig; "mapped" - "mixed"
    without the unmapped records"""
    cfg, b, h, refs, sites = dataset("tiny", 1700, 3, 0.03)
    rng = np.random.default_rng(17)
    if mix in ("all", "mapped"):
        b = b.take(np.nonzero(b.refid >= 0)[0])
    nref = b.next_refid.copy()
    if mix in ("mixed", "mapped"):
        pick = rng.random(b.n) < 0.35
        nref[pick] = rng.integers(-1, h.n_ref, int(pick.sum()))
    elif mix == "all":
        nref = ((b.refid + 1) % h.n_ref).astype(np.int32)
    else:
        nref = b.refid.copy()
    assert b.n >= 3000
    return _with(b, next_refid=nref.astype(np.int32)), h


@functools.lru_cache(maxsize=None)
def _case(mix, n):
    b, h = _reads(mix)
    b = b.take(np.arange(n))
    return b, h, (orc.bam_encode(b, h.rg_ids) if n else np.zeros(0, np.uint8))


@functools.lru_cache(maxsize=None)
def _want(mix, n, n_groups, single_end=False):
    b, h, raw = _case(mix, n)
    return splitref.split_bytes(raw.tobytes(), GOF[n_groups], n_groups, single_end), splitref.split_lines(raw.tobytes(), GOF[n_groups], n_groups, h.ref_names, single_end)


def _emit(e, n_groups, fmt="bam", single_end=False):
    return [a.tobytes() for a in e.emit_split(np.asarray(GOF[n_groups], np.int32), n_groups, fmt=fmt, single_end=single_end)]


def _call(e, fmt, gof, n_groups, single_end, out, cap):
    """the C call itself -> (return code, n_bytes, offsets)"""
    fn = getattr(e.L, "elp_emit_split_" + fmt)
    g = np.asarray(gof, np.int32)
    off = np.full(n_groups + (2 if single_end else 3), 2 ** 64 - 1, np.uint64)
    n = C.c_uint64(12345)
    rc = fn(e.h, C.c_void_p(g.ctypes.data), n_groups, int(single_end), C.c_void_p(out.ctypes.data if out is not None else 0), cap, C.c_void_p(off.ctypes.data), C.byref(n))
    return rc, int(n.value), off


def _staged(h, raw):
    e = Engine(h)
    e.set_read_group_ids(h.rg_ids)
    e.stage_bam(raw)
    return e


# ---- 1. record counts x group counts
@pytest.mark.parametrize("n_groups", [1, 2, 17, 300])
def test_files_at_every_seam_of_the_list(n_groups):
    b, h = _reads("mixed")
    e = Engine(h)
    try:
        e.set_read_group_ids(h.rg_ids)
        for n in COUNTS:
            bn, _, raw = _case("mixed", n)
            want_bam, want_sam = _want("mixed", n, n_groups)
            if n:
                e.stage_bam(raw)
            assert _emit(e, n_groups) == want_bam, n
            assert _emit(e, n_groups, "sam") == want_sam, n
            assert len(want_bam) == n_groups + 2
            want_single, _ = _want("mixed", n, n_groups, True)
            assert _emit(e, n_groups, single_end=True) == want_single and len(want_single) == n_groups + 1, n
            if n == 3000:
                g, sp = sfm.split_records(bn, np.asarray(GOF[n_groups], np.int32))
                assert sp.sum() > 200 and (g == 0).sum() > 5                           # the case has spread and unmapped records
                assert len(tagref.records(want_bam[-1])) == int(sp.sum())
                assert b"".join(want_single) != b"".join(want_bam[:-1])                # ... and tagged copies, which single-end has not
            e.reset()
    finally:
        e.close()


# ---- 2. the spread mix and empty files
@pytest.mark.parametrize("mix,n_groups,empty", [("all", 17, [0]), ("none", 17, [18]), ("mapped", 3, [0, 2]), ("mixed", 3, [2])])
def test_spread_mix_and_empty_files(mix, n_groups, empty):
    """all records spread (and no unmapped file), none spread (an empty spread file), a group file empty in the middle"""
    n = 513
    b, h, raw = _case(mix, n)
    want_bam, want_sam = _want(mix, n, n_groups)
    for f in range(n_groups + 2):
        assert (want_bam[f] == b"") == (f in empty or (n_groups == 17 and f not in (0, 3, 9, 17, 18))), f
    if mix == "all":
        assert len(tagref.records(want_bam[-1])) == n and b"".join(want_bam[:-1]).count(b"srC\x01") >= n
    e = _staged(h, raw)
    try:
        assert _emit(e, n_groups) == want_bam
        assert _emit(e, n_groups, "sam") == want_sam
        bz = _emit(e, n_groups, "bgzf")
        assert [b"".join(m for _, m in _members(z)) for z in bz] == want_bam
        assert [z == b"" for z in bz] == [w == b"" for w in want_bam]              # an empty file is zero bytes
        assert [a.tobytes() for a in sfm.split_files_device(e, np.asarray(GOF[n_groups], np.int32), n_groups, "bam")] == want_bam
    finally:
        e.close()


# ---- 3. rejected records
def test_rejected_records_appear_nowhere():
    b, h, raw = _case("mixed", 513)
    rejected = np.nonzero(b.mapq < 30)[0]
    assert 20 < rejected.size < 500
    e = _staged(h, raw)
    try:
        assert e.filter_records(min_mapq=30) == rejected.size
        for n_groups in (2, 17):
            assert _emit(e, n_groups) == splitref.split_bytes(raw.tobytes(), GOF[n_groups], n_groups, rejected=rejected)
            assert _emit(e, n_groups, "sam") == splitref.split_lines(raw.tobytes(), GOF[n_groups], n_groups, h.ref_names, rejected=rejected)
            assert _emit(e, n_groups, single_end=True) == splitref.split_bytes(raw.tobytes(), GOF[n_groups], n_groups, True, rejected=rejected)
    finally:
        e.close()


# ---- 4. SmallMap.Set on records that hold sr fields already (state 1), and re-encoded integers
def _sr_variant(fields, i):
    sr = lambda ty, v: tagref.int_field(b"sr", ty, v)
    k = i % 8
    if k == 0:
        return fields                                                    # no sr field: appended behind the last field
    if k == 1:
        return [sr(b"C", 1)] + fields                                    # the first field
    if k == 2:
        return fields[:2] + [sr(b"S", 10000)] + fields[2:]               # a middle field, another value and type
    if k == 3:
        return fields + [sr(b"i", 1)]                                    # the last field, type i: re-encoded as C where it stays
    if k == 4:
        return fields[:1] + [sr(b"C", 5)] + fields[1:] + [sr(b"C", 9)]   # twice: the later one stays
    if k == 5:
        return [(b"sr", b"Z", b"yes\0")] + fields                        # type Z
    if k == 6:
        return fields + [tagref.int_field(b"XN", b"i", -3), tagref.int_field(b"XM", b"i", -40000), (b"sR", b"C", b"\x07")]  # negative ints; a key one byte off
    return []                                                            # no optional field at all


def test_set_sr_on_records_with_sr_fields():
    b, h, raw = _case("mixed", 513)
    recs = tagref.records(raw.tobytes())
    raw2 = b"".join(tagref.with_fields(r, _sr_variant(tagref.parse_fields(r), i)) for i, r in enumerate(recs))
    g, sp = sfm.split_records(b, np.asarray(GOF[17], np.int32))
    assert all((sp[k::8]).any() and (~sp[k::8]).any() for k in range(8))            # every variant both tagged and untagged
    e = _staged(h, np.frombuffer(raw2, np.uint8))
    try:
        assert e.n - e.n_sorted == sum(1 for i in range(b.n) if i % 8 in (1, 2, 3, 4, 5))   # state 1: staged with an sr field
        for n_groups in (17, 2):
            assert _emit(e, n_groups) == splitref.split_bytes(raw2, GOF[n_groups], n_groups)
            assert _emit(e, n_groups, "sam") == splitref.split_lines(raw2, GOF[n_groups], n_groups, h.ref_names)
        assert _emit(e, 17, single_end=True) == splitref.split_bytes(raw2, GOF[17], 17, True)
        # a split file that is split again keeps its sr fields
        again = _emit(e, 17)[3]
        e.reset()
        e.stage_bam(np.frombuffer(again, np.uint8))
        assert _emit(e, 17, single_end=True)[3] == again and again.count(b"srC\x01") > 20
    finally:
        e.close()


# ---- 5. device passes
def test_passes_end_inside_a_file_at_a_file_boundary_and_behind_every_record():
    n, n_groups = 257, 3
    b, h, raw = _case("mixed", n)
    want_bam, want_sam = _want("mixed", n, n_groups)
    counts = [len(tagref.records(w)) for w in want_bam]
    assert counts[2] == 0 and counts[0] >= 1 and min(counts[1], counts[3], counts[4]) > 2
    e = _staged(h, raw)
    try:
        e.set_tuning("bgzf_stored", 1)
        for per_pass in (1, counts[1], counts[1] // 2, 97):      # one record per pass; file 1 ends with a pass; passes end inside the files
            e.set_tuning("emit_pass", per_pass)
            assert _emit(e, n_groups) == want_bam, per_pass
            assert _emit(e, n_groups, "sam") == want_sam, per_pass
            assert [b"".join(m for _, m in _members(z)) for z in _emit(e, n_groups, "bgzf")] == want_bam, per_pass
    finally:
        e.set_tuning("emit_pass", 0)
        e.set_tuning("bgzf_stored", 0)
        e.close()


# ---- 6. BGZF
@pytest.mark.parametrize("stored", [0, 1])
def test_bgzf_files_are_framed_on_their_own(stored):
    """files larger than one member beside an empty one; members of 65280 bytes wherever the passes end; nothing crosses a file boundary"""
    n, n_groups = 3000, 3
    b, h, raw = _case("mixed", n)
    want_bam, _ = _want("mixed", n, n_groups)
    assert want_bam[2] == b"" and len(want_bam[1]) > 2 * 65280 and len(want_bam[3]) > 65280
    e = _staged(h, raw)
    try:
        e.set_tuning("bgzf_stored", stored)
        for per_pass in (0, 700):
            e.set_tuning("emit_pass", per_pass)
            bz = _emit(e, n_groups, "bgzf")
            for f, z in enumerate(bz):
                mem = _members(z)
                assert b"".join(m for _, m in mem) == want_bam[f], (f, per_pass)
                assert all(len(m) == 65280 for _, m in mem[:-1]) and all(0 < len(m) <= 65280 for _, m in mem), (f, per_pass)
                assert (z == b"") == (want_bam[f] == b"")
            rc, bound, off = _call(e, "bgzf", GOF[n_groups], n_groups, False, None, 0)       # the size query: the stored form's bound
            assert rc == 0 and bound >= sum(len(z) for z in bz)
            assert all(int(off[f + 1] - off[f]) >= len(z) for f, z in enumerate(bz)) and int(off[-1]) == bound
    finally:
        e.set_tuning("emit_pass", 0)
        e.set_tuning("bgzf_stored", 0)
        e.close()


# ---- 7. size queries and the buffer's size
@pytest.mark.parametrize("fmt", ["bam", "sam"])
def test_size_query_is_exact_and_a_short_buffer_is_refused(fmt):
    n, n_groups = 513, 17
    b, h, raw = _case("mixed", n)
    want = _want("mixed", n, n_groups)[0 if fmt == "bam" else 1]
    total = sum(len(w) for w in want)
    want_off = np.cumsum([0] + [len(w) for w in want]).astype(np.uint64)
    e = _staged(h, raw)
    try:
        if fmt == "sam":
            e._header_names()
        rc, size, off = _call(e, fmt, GOF[n_groups], n_groups, False, None, 0)
        assert rc == 0 and size == total and np.array_equal(off, want_off)
        out = np.full(total + 8, 0xAA, np.uint8)
        rc, size, off = _call(e, fmt, GOF[n_groups], n_groups, False, out, total - 1)
        assert rc == ELP_ERR_ARG and size == 0 and b"too small" in e.L.elp_last_error(e.h)   # nothing counted as written
        rc, size, off = _call(e, fmt, GOF[n_groups], n_groups, False, out, total)
        assert rc == 0 and size == total and np.array_equal(off, want_off)
        assert out[:total].tobytes() == b"".join(want) and (out[total:] == 0xAA).all()
    finally:
        e.close()


# ---- 8. refusals
def test_refusals():
    n_groups = 2
    b, h, raw = _case("mixed", 65)
    gof = np.asarray(GOF[n_groups], np.int32)
    off = np.zeros(n_groups + 2, np.uint64)
    nb = C.c_uint64()
    vp = lambda a: C.c_void_p(a.ctypes.data)
    e = _staged(h, raw)
    try:
        err = lambda: e.L.elp_last_error(e.h)
        for fmt in ("bam", "bgzf", "sam"):
            fn = getattr(e.L, "elp_emit_split_" + fmt)
            assert fn(C.c_void_p(0), vp(gof), n_groups, 0, C.c_void_p(0), 0, vp(off), C.byref(nb)) == ELP_ERR_ARG
            assert fn(e.h, C.c_void_p(0), n_groups, 0, C.c_void_p(0), 0, vp(off), C.byref(nb)) == ELP_ERR_ARG and b"must be given" in err()
            assert fn(e.h, vp(gof), n_groups, 0, C.c_void_p(0), 0, C.c_void_p(0), C.byref(nb)) == ELP_ERR_ARG and b"must be given" in err()
            assert fn(e.h, vp(gof), n_groups, 0, C.c_void_p(0), 0, vp(off), None) == ELP_ERR_ARG and b"must be given" in err()
            for bad in (0, -1, 65534):
                assert fn(e.h, vp(gof), bad, 0, C.c_void_p(0), 0, vp(off), C.byref(nb)) == ELP_ERR_ARG and b"n_groups" in err(), bad
            for bad in ([1, 3, 2], [1, -1, 2]):
                assert _call(e, fmt, bad, n_groups, False, None, 0)[0] == ELP_ERR_ARG and b"group_of_ref" in err(), bad
        big = np.zeros(65533 + 3, np.uint64)                       # the largest group count is taken
        assert e.L.elp_emit_split_bam(e.h, vp(gof), 65533, 0, C.c_void_p(0), 0, vp(big), C.byref(nb)) == 0
        assert int(big[-1]) == int(nb.value) == sum(len(w) for w in splitref.split_bytes(raw.tobytes(), GOF[n_groups], 65533))
        # a tag filter: `elprep split` has no such option
        e.set_tag_filter(remove=["NM"])
        for fmt in ("bam", "bgzf", "sam"):
            assert _call(e, fmt, gof, n_groups, False, None, 0)[0] == ELP_ERR_ARG and b"tag filter" in err()
        e.set_tag_filter()
        assert _call(e, "bam", gof, n_groups, False, None, 0)[0] == 0
        # an H field
        recs = tagref.records(raw.tobytes())
        recs[5] = tagref.with_fields(recs[5], tagref.parse_fields(recs[5]) + [(b"XH", b"H", b"1AE3\0")])
        e.reset()
        e.stage_bam(np.frombuffer(b"".join(recs), np.uint8))
        e._header_names()
        for fmt in ("bam", "bgzf", "sam"):
            assert _call(e, fmt, gof, n_groups, False, None, 0)[0] == ELP_ERR_UNSUPPORTED and b"H-typed" in err()
        # records staged as columns: no bytes to write
        e.reset()
        e.stage(b)
        for fmt in ("bam", "bgzf", "sam"):
            assert _call(e, fmt, gof, n_groups, False, None, 0)[0] == ELP_ERR_ARG and b"elp_stage_bam" in err()
    finally:
        e.close()
    # a replacing read group
    h1 = _one_group_header(h)
    e = Engine(h1)
    try:
        e.set_replace_read_group("new")
        e.stage_bam(raw)
        for fmt in ("bam", "bgzf", "sam"):
            assert _call(e, fmt, gof, n_groups, False, None, 0)[0] == ELP_ERR_ARG and b"replacing read group" in e.L.elp_last_error(e.h)
    finally:
        e.close()
    # SAM without reference names (a header no other test uses: a pooled context of it never had names)
    h2 = copy.copy(h)
    h2.ref_len = h.ref_len.copy()
    h2.ref_len[0] += 1
    e = _staged(h2, raw)
    try:
        assert _call(e, "sam", gof, n_groups, False, None, 0)[0] == ELP_ERR_ARG and b"names are not set" in e.L.elp_last_error(e.h)
        assert _call(e, "bam", gof, n_groups, False, None, 0)[0] == 0
        with pytest.raises(ElpError):
            e.emit_split(gof[:2], n_groups)
        with pytest.raises(KeyError):
            e.emit_split(gof, n_groups, fmt="cram")
    finally:
        e.close()


# ---- 9. nothing is invalidated
def test_the_call_invalidates_nothing():
    b, h, raw = _case("mixed", 3000)
    want_bam, want_sam = _want("mixed", 3000, 2)
    e = _staged(h, raw)
    try:
        flags = e.mark_duplicates(True)
        perm = e.sort_coordinate()
        before = e.emit_sorted_bam().tobytes()
        for fmt, want in (("bam", want_bam), ("sam", want_sam)):
            # (the files carry the duplicate flags as they are now: FLAG is a column)
            marked = tagref.records(orc.bam_encode(b, h.rg_ids, flags=flags).tobytes())
            raw_marked = b"".join(marked)
            ref = splitref.split_bytes(raw_marked, GOF[2], 2) if fmt == "bam" else splitref.split_lines(raw_marked, GOF[2], 2, h.ref_names)
            assert _emit(e, 2, fmt) == ref
        assert len(_emit(e, 2, "bgzf")) == 4
        assert np.array_equal(e.permutation(), perm) and np.array_equal(e.flags(), flags)
        assert e.emit_sorted_bam().tobytes() == before
        assert np.array_equal(e.dup_metrics(100), e.dup_metrics(100))
        keep = e.order_keep()
        before = e.emit_sorted_bam().tobytes()
        _emit(e, 17)
        assert np.array_equal(e.permutation(), keep) and e.emit_sorted_bam().tobytes() == before
        split, spread, counts = e.split_classify(np.asarray(GOF[2], np.int32), 2)   # needs none, and works behind one
        assert [len(tagref.records(w)) for w in _emit(e, 2)] == [int(c) for c in counts]
    finally:
        e.close()


# ---- 10. split -> filter -> merge
def test_round_trip_of_the_files_against_routed_contexts():
    """the group files staged again (split id = file) and the spread file in a context of its own hold what elp_copy_records delivers:
    the same marks, order, counts and metrics, the oracle's marks on sfm.with_sr's records, and the same merged stream"""
    n_groups = 2
    b, h, raw = _case("mixed", 3000)
    gof = np.asarray(GOF[n_groups], np.int32)
    g, sp = sfm.split_records(b, gof)
    idx = [np.nonzero(g == f)[0] for f in range(n_groups + 1)]
    want = Batch.concat([sfm.with_sr(b, sp, g).take(i) for i in idx])
    want_spread = b.take(np.nonzero(sp)[0])
    engines = [Engine(h) for _ in range(5)]
    reader, groups, spread, routed, routed_spread = engines
    try:
        for e in engines:
            e.set_read_group_ids(h.rg_ids)
        reader.stage_bam(raw)
        files = reader.emit_split(gof, n_groups)
        for f in range(n_groups + 1):
            groups.stage_bam(files[f], split_id=f)
        spread.stage_bam(files[n_groups + 1])
        reader.split_classify(gof, n_groups)
        for f in range(n_groups + 1):
            routed.copy_records_from(reader, idx[f].astype(np.uint32) | (sp[idx[f]].astype(np.uint32) << np.uint32(31)), tag_sr=2)
        routed_spread.copy_records_from(reader, np.nonzero(sp)[0].astype(np.uint32), new_split=0)
        assert groups.n == routed.n == want.n and spread.n == routed_spread.n == want_spread.n > 200
        oflags = orc.mark_duplicates(want, h)
        assert np.array_equal(groups.mark_duplicates(True), oflags) and np.array_equal(routed.mark_duplicates(True), oflags)
        assert np.array_equal(spread.mark_duplicates(True), orc.mark_duplicates(want_spread, h))
        assert np.array_equal(routed_spread.mark_duplicates(True), spread.flags())
        assert np.array_equal(groups.sort_coordinate(), routed.sort_coordinate())
        assert np.array_equal(spread.sort_coordinate(), routed_spread.sort_coordinate())
        assert groups.n_sorted == routed.n_sorted == want.n - int(want.has_sr.sum()) and int(want.has_sr.sum()) == int(sp.sum())
        assert np.array_equal(groups.dup_metrics(100), routed.dup_metrics(100))
        assert np.array_equal(spread.dup_metrics(100), routed_spread.dup_metrics(100))
        merged = groups.emit_merged_bam(spread).tobytes()
        assert merged == routed.emit_merged_bam(routed_spread).tobytes() and len(tagref.records(merged)) == b.n
    finally:
        for e in engines:
            e.close()
