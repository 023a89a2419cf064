"""GPU tests (-m gpu) of the options that touch a record's optional fields: elp_set_tag_filter (--remove-optional-fields /
--keep-optional-fields), elp_filter_exact_strict (--filter-non-exact-mapping-reads-strict), elp_set_replace_read_group
(--replace-read-group) and elp_clear_duplicate_flag (--clear-duplicate-flag).

The oracle's BAM encoder writes a fixed set of optional fields, so the input records get more fields appended (tests/tagref.py:
X0 .. XG in several integer types, a second NM field, a second RG field where RG is replaced, a key one byte off an existing one) and the expected bytes are
the oracle's records (its flags, order and recalibrated qualities) with the same fields appended as formatBamTag writes them and
tagref's restatement of the option applied record by record."""
import ctypes as C

import numpy as np
import pytest

import oracle as orc
from elprep_amd.batch import Batch, Header
from elprep_amd.engine import BqsrTables, ElpError, Engine
from tests import tagref
from tests.common import dataset
from tests.test_gpu_round4 import _members

pytestmark = pytest.mark.gpu

ELP_ERR_ARG, ELP_ERR_DATA = -1, -4
NIL16 = 0xFFFF
PRESENT = ["NM", "RG", "AS", "XT", "XL", "XB", "MD", "X0", "X1", "XM", "XO", "XG", "Xt"]  # every key the test records carry


def _extra(i, second_rg=False):
    """the fields appended to staging record i, in types another writer might choose; second_rg: some records get another RG field
    (only where RG fields are not looked up: staging resolves every RG:Z field it meets)"""
    f = []
    if i % 4 != 3:      # exact by the strict filter: X0 = 1 in three integer types
        f += [tagref.int_field(b"X0", (b"C", b"s", b"I")[i % 3], 1), tagref.int_field(b"X1", b"i", 0), tagref.int_field(b"XM", b"C", 0),
              tagref.int_field(b"XO", b"c", 0), tagref.int_field(b"XG", b"S", 0)]
    else:               # rejected, each for another reason
        how = (i // 4) % 5
        x0 = [] if how == 0 else [tagref.int_field(b"X0", b"C", 2 if how in (1, 4) else 1)]
        if how == 4:
            x0.append(tagref.int_field(b"X0", b"C", 1))  # the first X0 field counts
        f += x0 + [tagref.int_field(b"X1", b"C", 0), tagref.int_field(b"XM", b"i", 1 if how == 2 else 0), tagref.int_field(b"XO", b"C", 0)]
        if how != 3:
            f.append(tagref.int_field(b"XG", b"C", 0))
    if i % 6 == 0:
        f.append(tagref.int_field(b"NM", b"i", 9))       # a second field of a key the record has
    if i % 5 == 1:
        f.append((b"Xt", b"Z", b"near XT\0"))            # one byte off XT
    if second_rg and i % 9 == 0:
        f.append((b"RG", b"Z", b"zz\0"))                 # a second (or, without the oracle's, the only) RG field
    return f


def _case(n_pairs, seed, rg_ids=None, batch=None, second_rg=False):
    cfg, b, h, refs, sites = dataset("tiny", n_pairs, seed, 0.03)
    b = b if batch is None else batch(b)
    extra = [_extra(i, second_rg) for i in range(b.n)]
    raw = np.frombuffer(tagref.append_fields(orc.bam_encode(b, rg_ids or h.rg_ids).tobytes(), extra), np.uint8)
    return cfg, b, h, refs, sites, extra, raw


def _names(b):
    q, off = b.qname.tobytes(), b.qname_off.tolist()
    return [q[off[i]:off[i + 1]] for i in range(b.n)]


def _oracle_path(b, h, refs, sites, order="coordinate"):
    oflags = orc.mark_duplicates(b, h)
    if order == "coordinate":
        operm = orc.sort_coordinate(b, oflags)
    else:
        names = _names(b)
        operm = np.asarray(sorted(range(b.n), key=lambda i: names[i]), dtype=np.uint32)
    oq, oc, ox = orc.bqsr_gather(b, h, orc.BqsrRef(refs, sites), oflags, 500)
    oqual = orc.BqsrFinal(oq, oc, ox, 500).apply(b, h, 0)
    return oflags, operm, (oq, oc, ox), oqual


def _device_path(e, h, refs, sites, order="coordinate"):
    flags = e.mark_duplicates(True)
    perm = e.sort_coordinate() if order == "coordinate" else e.sort_queryname()
    for r in range(h.n_ref):
        e.set_reference(r, refs[r])
        e.set_known_sites(r, sites[r])
    qt, ct, xt = e.recalibrate(500)
    lut, present = BqsrTables(qt, ct, xt, 500).finalize().build_lut(0)
    qual = e.apply_bqsr(lut, present, 500)
    return flags, perm, (qt, ct, xt), qual


def _expected_records(b, rg_ids, order, flags, qual, extra):
    recs = tagref.records(orc.bam_encode(b, rg_ids, order=order, flags=flags, qual=qual, normalize_tags=True).tobytes())
    assert len(recs) == len(order)
    return [tagref.with_fields(r, tagref.parse_fields(r) + tagref.normalize(extra[int(i)])) for r, i in zip(recs, order)]


def _size_query(e, fn="elp_emit_sorted_bam"):
    n = C.c_uint64()
    e._check(getattr(e.L, fn)(e.h, C.c_void_p(0), 0, C.byref(n)))
    return int(n.value)


FILTERS = [
    dict(remove=["XT", "MD", "X0"]),
    dict(keep=["NM", "RG", "XB"]),
    dict(remove=["NM", "XL"], keep=["NM", "AS", "XL", "X1", "MD"]),
    dict(remove="all"),
    dict(keep="none"),
    dict(remove=["ZZ", "zz"], keep=PRESENT + ["Q1"]),      # lists that change nothing
    dict(remove=PRESENT),                                   # every field: a record ends behind its qualities
    dict(remove=["Nm", "nM", "XU", "YT", "RH", "x0", "X2"]),  # keys one byte off present ones
]


# ---- 1. output bytes
@pytest.mark.parametrize("n_pairs,seed", [(150, 3), (4000, 5)])
@pytest.mark.parametrize("order", ["coordinate", "queryname"])
def test_tag_filter_output_bytes(n_pairs, seed, order):
    cfg, b, h, refs, sites, extra, raw = _case(n_pairs, seed)
    oflags, operm, otabs, oqual = _oracle_path(b, h, refs, sites, order)
    want0 = _expected_records(b, h.rg_ids, operm, oflags, oqual, extra)
    e = Engine(h)
    try:
        e.set_read_group_ids(h.rg_ids)
        e.stage_bam(raw)
        flags, perm, tabs, qual = _device_path(e, h, refs, sites, order)
        assert np.array_equal(flags, oflags) and np.array_equal(perm, operm) and np.array_equal(qual, oqual)
        for f in FILTERS:
            e.set_tag_filter(**f)
            want = [tagref.apply_tag_filter(r, **f) for r in want0]
            got = e.emit_sorted_bam().tobytes()
            assert got == b"".join(want), f
            assert _size_query(e) == len(got), f
            if f.get("remove") is PRESENT:
                assert all(len(r) == tagref.tags_at(r) for r in tagref.records(got))
        assert any(tagref.apply_tag_filter(r, remove=["Nm"]) != tagref.apply_tag_filter(r, remove=["NM"]) for r in want0)
        e.set_tag_filter()  # taken away again
        assert e.emit_sorted_bam().tobytes() == b"".join(want0)
    finally:
        e.close()


def test_tag_filter_list_limits():
    cfg, b, h, refs, sites, extra, raw = _case(150, 3)
    e = Engine(h)
    try:
        many = ["%c%c" % (33 + k // 90, 33 + k % 90) for k in range(4097)]
        with pytest.raises(ElpError) as ei:
            e.set_tag_filter(remove=many)
        assert ei.value.code == -5
        e.set_tag_filter(remove=many[:4096], keep=many[:4096])
    finally:
        e.close()


# ---- 2. BGZF, several passes, the merged stream
@pytest.mark.parametrize("f", [dict(keep=["NM", "X0", "MD"]), dict(keep="none"), dict(remove=["AS", "RG"])])
def test_tag_filter_through_bgzf_and_in_passes(f):
    cfg, b, h, refs, sites, extra, raw = _case(4000, 6)
    oflags = orc.mark_duplicates(b, h)
    operm = orc.sort_coordinate(b, oflags)
    want = b"".join(tagref.apply_tag_filter(r, **f) for r in _expected_records(b, h.rg_ids, operm, oflags, None, extra))
    e = Engine(h)
    try:
        e.set_read_group_ids(h.rg_ids)
        e.stage_bam(raw)
        e.mark_duplicates(True)
        e.sort_coordinate()
        e.set_tag_filter(**f)
        for per_pass in (0, 333, 1):
            e.set_tuning("emit_pass", per_pass)
            assert e.emit_sorted_bam().tobytes() == want, per_pass
            bound = _size_query(e, "elp_emit_sorted_bgzf")
            bz = e.emit_sorted_bgzf().tobytes()
            assert bound >= len(bz)
            mem = _members(bz)
            assert b"".join(m for _, m in mem) == want, per_pass
            assert len(mem) >= 3 and all(len(m) == 65280 for _, m in mem[:-1]) and 0 < len(mem[-1][1]) <= 65280
    finally:
        e.set_tuning("emit_pass", 0)
        e.close()


def test_tag_filter_on_the_merged_stream():
    """elp_emit_merged_bam takes the filter of `groups`; a `spread` context whose filter differs is refused"""
    from elprep_amd import sfm
    from oracle import simple_filters as sf
    from tests.test_sfm_cpu import _merge_reference
    cfg, b, h, refs, sites = dataset("tiny", 3000, 17, 0.03)
    n_groups, gof = orc.contig_groups(cfg.ref_len, 80000)
    osplit, ospread = sf.split_records(b, gof)
    tagged = sfm.with_sr(b, ospread.astype(bool), osplit)
    tagged.split[:] = 0
    sp = b.take(np.nonzero(ospread)[0])
    f = dict(remove=["AS", "XB"], keep=["NM", "AS", "RG", "MD", "X0", "sr"])
    eg, es = Engine(h), Engine(h)
    try:
        recs, keys = [], []
        for eng, batch in ((eg, tagged), (es, sp)):
            extra = [_extra(i) for i in range(batch.n)]
            eng.set_read_group_ids(h.rg_ids)
            eng.stage_bam(np.frombuffer(tagref.append_fields(orc.bam_encode(batch, h.rg_ids).tobytes(), extra), np.uint8))
            eng.mark_duplicates(True)
            eng.sort_coordinate()
            oflags = orc.mark_duplicates(batch, h)
            order = orc.sort_coordinate(batch, oflags)[:orc.num_sorted(batch)]
            recs.append([tagref.apply_tag_filter(r, **f) for r in _expected_records(batch, h.rg_ids, order, oflags, None, extra)])
            keys.append([(int(batch.refid[i]), int(batch.pos[i])) for i in order])
        rg, rs = recs
        n_mapped = sum(1 for k in keys[0] if k[0] >= 0)
        codes = _merge_reference(keys[0][:n_mapped], keys[1])
        want = b"".join([rg[c] if c >= 0 else rs[-c - 1] for c in codes] + rg[n_mapped:])
        eg.set_tag_filter(**f)
        with pytest.raises(ElpError) as ei:
            eg.emit_merged_bam(es)
        assert ei.value.code == ELP_ERR_ARG
        es.set_tag_filter(remove=["AS"])
        with pytest.raises(ElpError) as ei:
            eg.emit_merged_bam(es)
        assert ei.value.code == ELP_ERR_ARG
        es.set_tag_filter(**f)
        n = C.c_uint64()
        eg._check(eg.L.elp_emit_merged_bam(eg.h, es.h, C.c_void_p(0), 0, C.byref(n)))
        got = eg.emit_merged_bam(es).tobytes()
        assert got == want and int(n.value) >= len(got)
    finally:
        eg.close()
        es.close()


# ---- 3. the strict filter, records staged from BGZF
def _bgzf(stream: bytes) -> np.ndarray:
    from tests.test_gpu_round4 import _bgzf as make
    return np.frombuffer(make(stream, 6), np.uint8)


def test_filter_exact_strict_against_the_oracle_on_the_kept_records():
    cfg, b, h, refs, sites, extra, raw = _case(3000, 8)
    verdict = [tagref.strict_keep(r) for r in tagref.records(raw.tobytes())]
    assert "panics" not in verdict
    keep = np.asarray([v == "keep" for v in verdict])
    assert 0.1 * b.n < (~keep).sum() < 0.5 * b.n
    e = Engine(h)
    try:
        e.set_read_group_ids(h.rg_ids)
        e.stage_bgzf(_bgzf(raw.tobytes()))
        assert e.n == b.n
        assert e.filter_exact_strict() == int((~keep).sum())
        assert e.filter_exact_strict() == 0                       # nothing left to reject
        kept = np.nonzero(keep)[0]
        assert e.n_sorted == kept.size
        kb = b.take(kept)
        oflags, operm, otabs, oqual = _oracle_path(kb, h, refs, sites)
        flags = e.mark_duplicates(True)
        perm = e.sort_coordinate()
        ctr = e.dup_metrics(100)
        _, octr, _ = orc.dup_metrics(kb, h, operm, 100)
        assert np.array_equal(flags[kept], oflags)
        assert np.array_equal(perm[:kept.size], kept[operm]) and set(perm[kept.size:].tolist()) == set(np.nonzero(~keep)[0].tolist())
        assert np.array_equal(ctr, octr)
        for r in range(h.n_ref):
            e.set_reference(r, refs[r])
            e.set_known_sites(r, sites[r])
        tabs = e.recalibrate(500)
        assert all(np.array_equal(a, o) for a, o in zip(tabs, otabs))
        full = b.flag.copy()
        full[kept] = oflags                                        # (the oracle's fields of a record depend on its index in `b`)
        want = _expected_records(b, h.rg_ids, kept[operm], full, None, extra)
        assert e.emit_sorted_bam().tobytes() == b"".join(want)   # the rejected records are absent from the output
    finally:
        e.close()


def test_filter_exact_strict_adds_up_with_filter_records():
    from oracle import simple_filters as sf
    cfg, b, h, refs, sites, extra, raw = _case(1500, 9)
    first = sf.keep_mask(b, min_mapq=20)
    strict = np.asarray([tagref.strict_keep(r) == "keep" for r in tagref.records(raw.tobytes())])
    assert 0 < (~first).sum() and 0 < (first & ~strict).sum()
    e = Engine(h)
    try:
        e.set_read_group_ids(h.rg_ids)
        e.stage_bam(raw)
        assert e.filter_records(min_mapq=20) == int((~first).sum())
        assert e.filter_exact_strict() == int((first & ~strict).sum())  # records an earlier filter rejected are not counted again
        kept = np.nonzero(first & strict)[0]
        assert e.n_sorted == kept.size
        assert np.array_equal(e.mark_duplicates(True)[kept], orc.mark_duplicates(b.take(kept), h))
    finally:
        e.close()


def _two_records(b, fields0, fields1):
    two = b.take(np.arange(2))
    recs = tagref.records(orc.bam_encode(two, ["rg1", "rg2", "rg3", "rg4"]).tobytes())
    return two, np.frombuffer(tagref.with_fields(recs[0], fields0) + tagref.with_fields(recs[1], fields1), np.uint8)


def test_filter_exact_strict_panic_and_its_twin():
    cfg, b, h, refs, sites = dataset("tiny", 150, 3, 0.03)
    ok = [tagref.int_field(k, b"C", v) for k, v in ((b"X0", 1), (b"X1", 0), (b"XM", 0), (b"XO", 0), (b"XG", 0))]
    xm_a = [ok[0], ok[1], (b"XM", b"A", b"0"), ok[3], ok[4]]
    twin = [tagref.int_field(b"X0", b"C", 2)] + xm_a[1:]
    two, raw = _two_records(b, ok, xm_a)
    assert [tagref.strict_keep(r) for r in tagref.records(raw.tobytes())] == ["keep", "panics"]
    e = Engine(h)
    try:
        e.set_read_group_ids(h.rg_ids)
        e.stage_bam(raw)
        with pytest.raises(ElpError) as ei:
            e.filter_exact_strict()
        assert ei.value.code == ELP_ERR_DATA
        assert e.n_sorted == 2                                     # a failed call changes nothing
        e.reset()
        two, raw = _two_records(b, ok, twin)                       # X0 = 2 fails first: XM:A is never looked at
        assert [tagref.strict_keep(r) for r in tagref.records(raw.tobytes())] == ["keep", "reject"]
        e.stage_bam(raw)
        assert e.filter_exact_strict() == 1 and e.n_sorted == 1
        e.reset()
        e.stage(b)                                                 # columns only: no optional fields to read
        with pytest.raises(ElpError) as ei:
            e.filter_exact_strict()
        assert ei.value.code == ELP_ERR_ARG
    finally:
        e.close()


# ---- 4. replace-read-group
def _one_group_header(h, rg_id="new"):
    return Header.from_read_groups(h.ref_names, h.ref_len, [{"ID": rg_id, "LB": "libN", "PU": "FC9.1"}])


def _with_rgid(b, rgid):
    cols = {name: getattr(b, name) for name in b.__dataclass_fields__}
    cols["rgid"] = np.ascontiguousarray(rgid, dtype=np.uint16)
    return Batch(**cols)


def test_replace_read_group_whole_path_and_output():
    """records that name three read groups, some none, some with a second RG field; a header of the one new group: flags, order, tables
    and recalibrated qualities are the oracle's on the same reads all of read group 0, the output is SmallMap.Set's"""
    cfg, b_in, h4, refs, sites, extra, raw = _case(3000, 10, batch=lambda b: _with_rgid(b, np.where(b.rgid == 3, NIL16, b.rgid)), second_rg=True)
    assert set(np.unique(b_in.rgid).tolist()) == {0, 1, 2, NIL16}
    h1 = _one_group_header(h4)
    b0 = _with_rgid(b_in, np.zeros(b_in.n, np.uint16))
    oflags, operm, otabs, oqual = _oracle_path(b0, h1, refs, sites)
    want0 = [tagref.replace_read_group(r, "new") for r in _expected_records(b_in, h4.rg_ids, operm, oflags, oqual, extra)]
    e, other = Engine(h1), Engine(h1)
    try:
        e.set_replace_read_group("new")                            # no elp_set_read_group_ids: RG fields are not looked up
        e.stage_bam(raw)
        flags, perm, tabs, qual = _device_path(e, h1, refs, sites)
        assert np.array_equal(flags, oflags) and np.array_equal(perm, operm) and np.array_equal(qual, oqual)
        assert all(np.array_equal(a, o) for a, o in zip(tabs, otabs))
        got = e.emit_sorted_bam().tobytes()
        assert got == b"".join(want0) and _size_query(e) == len(got)
        assert b"".join(m for _, m in _members(e.emit_sorted_bgzf().tobytes())) == got
        for f in (dict(remove=["RG"]), dict(keep=["RG", "NM"])):   # the tag filter acts on the result
            e.set_tag_filter(**f)
            assert e.emit_sorted_bam().tobytes() == b"".join(tagref.apply_tag_filter(r, **f) for r in want0), f
        # the setting travels with nothing
        with pytest.raises(ElpError) as ei:
            other.copy_records_from(e, np.arange(10))
        assert ei.value.code == ELP_ERR_ARG and other.n == 0
        with pytest.raises(ElpError) as ei:
            e.set_replace_read_group("late")                       # records are staged
        assert ei.value.code == ELP_ERR_ARG
        other.set_replace_read_group("new")
        other.copy_records_from(e, np.arange(10))
        assert other.n == 10
    finally:
        e.close()
        other.close()


@pytest.mark.parametrize("id_len", [1, 40, 255])
def test_replace_read_group_records_that_grow(id_len):
    """a record whose RG value was one byte long, one whose RG field is of type A, and one without RG: each goes out 4 + id_len bytes
    longer at most, the largest staged record included"""
    cfg, b, h4, refs, sites = dataset("tiny", 150, 3, 0.03)
    three = _with_rgid(b.take(np.arange(3)), [0, NIL16, NIL16])
    recs = tagref.records(orc.bam_encode(three, ["a"]).tobytes())
    assert (b"RG", b"Z", b"a\0") in tagref.parse_fields(recs[0])
    recs[1] = tagref.with_fields(recs[1], parse1 := tagref.parse_fields(recs[1]) + [(b"RG", b"A", b"x")])
    assert not any(k == b"RG" for k, _, _ in tagref.parse_fields(recs[2])) and len(parse1) > 1
    new_id = ("g" * id_len)
    h1 = _one_group_header(h4, new_id)
    b0 = _with_rgid(three, [0, 0, 0])
    oflags = orc.mark_duplicates(b0, h1)
    operm = orc.sort_coordinate(b0, oflags)
    e = Engine(h1)
    try:
        e.set_replace_read_group(new_id)
        e.stage_bam(np.frombuffer(b"".join(recs), np.uint8))
        assert np.array_equal(e.mark_duplicates(True), oflags) and np.array_equal(e.sort_coordinate(), operm)
        enc = tagref.records(orc.bam_encode(three, ["a"], order=operm, flags=oflags, normalize_tags=True).tobytes())
        want, grow = [], []
        for r, i in zip(enc, operm):
            base = tagref.with_fields(r, tagref.parse_fields(r) + ([(b"RG", b"A", b"x")] if i == 1 else []))
            want.append(tagref.replace_read_group(base, new_id))
            grow.append(len(want[-1]) - len(base))
        assert sorted(grow) == sorted([id_len - 1, id_len, 4 + id_len])
        got = e.emit_sorted_bam().tobytes()
        assert got == b"".join(want) and _size_query(e) == len(got)
        assert b"".join(m for _, m in _members(e.emit_sorted_bgzf().tobytes())) == got
    finally:
        e.close()


def test_replace_read_group_call_order():
    cfg, b, h4, refs, sites = dataset("tiny", 150, 3, 0.03)
    e = Engine(h4)
    try:
        with pytest.raises(ElpError) as ei:
            e.set_replace_read_group("new")                        # a header of four read groups
        assert ei.value.code == ELP_ERR_ARG
        with pytest.raises(ElpError) as ei:
            e.set_replace_read_group(b"a\0b")
        assert ei.value.code == ELP_ERR_ARG
    finally:
        e.close()


# ---- 5. clear-duplicate-flag
def test_clear_duplicate_flag_in_front_of_mark_duplicates():
    cfg, b, h, refs, sites = dataset("tiny", 3000, 12, 0.03)
    was = b.flag | np.where(np.arange(b.n) % 3 == 0, 0x400, 0).astype(np.uint16)
    cols = {name: getattr(b, name) for name in b.__dataclass_fields__}
    cols["flag"] = was.astype(np.uint16)
    dirty = Batch(**cols)
    oflags = orc.mark_duplicates(b, h)                              # the oracle on the cleared batch
    assert (b.flag & 0x400).sum() == 0 and (((was & 0x400) != 0) & ((oflags & 0x400) == 0)).sum() > 100  # winners among the marked
    operm = orc.sort_coordinate(b, oflags)
    e = Engine(h)
    try:
        e.set_read_group_ids(h.rg_ids)
        e.stage_bam(orc.bam_encode(dirty, h.rg_ids))
        before = e.sort_coordinate()
        assert np.array_equal(before, orc.sort_coordinate(dirty))
        e.clear_duplicate_flag()
        assert np.array_equal(e.flags(), b.flag)
        with pytest.raises(ElpError) as ei:
            e.permutation()                                        # the order made with the old bits is not served
        assert ei.value.code == ELP_ERR_ARG
        assert np.array_equal(e.mark_duplicates(True), oflags)
        assert np.array_equal(e.sort_coordinate(), operm)
        assert e.emit_sorted_bam().tobytes() == orc.bam_encode(b, h.rg_ids, order=operm, flags=oflags, normalize_tags=True).tobytes()
        # behind mark duplicates: the marks go, every state's record is cleared (here: one rejected by a filter)
        e.filter_records(min_mapq=20)
        e.mark_duplicates(True)
        e.clear_duplicate_flag()
        assert (e.flags() & 0x400).sum() == 0
    finally:
        e.close()


@pytest.mark.parametrize("n", [1, 7, 8, 9, 4099])
def test_clear_duplicate_flag_lengths(n):
    cfg, b, h, refs, sites = dataset("tiny", 3000, 12, 0.03)
    part = b.take(np.arange(n))
    cols = {name: getattr(part, name) for name in part.__dataclass_fields__}
    cols["flag"] = (part.flag | 0x400).astype(np.uint16)
    e = Engine(h)
    try:
        e.stage(Batch(**cols))
        e.clear_duplicate_flag()
        assert np.array_equal(e.flags(), part.flag)
    finally:
        e.close()


# ---- 6. lifetime of the settings
def test_settings_end_with_reset_and_with_set_header():
    cfg, b, h4, refs, sites, extra, raw = _case(600, 4)
    oflags = orc.mark_duplicates(b, h4)
    operm = orc.sort_coordinate(b, oflags)
    plain = b"".join(_expected_records(b, h4.rg_ids, operm, oflags, None, extra))

    def emit(e):
        e.stage_bam(raw)
        e.mark_duplicates(True)
        e.sort_coordinate()
        return e.emit_sorted_bam().tobytes()

    e = Engine(h4)
    try:
        e.set_read_group_ids(h4.rg_ids)
        e.set_tag_filter(keep="none")
        assert len(emit(e)) < len(plain)
        e.reset()
        assert emit(e) == plain
        e.set_tag_filter(remove="all")
        hs = h4.as_struct()
        e._check(e.L.elp_set_header(e.h, C.byref(hs)))
        e.reset()
        assert emit(e) == plain
    finally:
        e.close()
    h1 = _one_group_header(h4)
    e = Engine(h1)
    try:
        for clear in ("reset", "set_header"):
            e.set_replace_read_group("new")
            e.stage_bam(raw)                                       # names rg1 .. rg4: not looked up
            assert e.n == b.n
            e.reset()
            if clear == "set_header":
                e.set_replace_read_group("new")
                hs = h1.as_struct()
                e._check(e.L.elp_set_header(e.h, C.byref(hs)))
            e.set_read_group_ids(["new"])
            with pytest.raises(ElpError) as ei:
                e.stage_bam(raw)                                   # RG is looked up again: the header does not know rg1
            assert ei.value.code == ELP_ERR_ARG and "read group" in str(ei.value)
            e.reset()
    finally:
        e.close()


# ---- 7. no new call made: the bytes of before
@pytest.mark.parametrize("order", ["coordinate", "queryname"])
def test_output_without_any_new_call_is_unchanged(order):
    cfg, b, h, refs, sites = dataset("tiny", 2500, 7, 0.03)
    oflags, operm, otabs, oqual = _oracle_path(b, h, refs, sites, order)
    e = Engine(h)
    try:
        e.set_read_group_ids(h.rg_ids)
        e.stage_bam(orc.bam_encode(b, h.rg_ids))
        _device_path(e, h, refs, sites, order)
        want = orc.bam_encode(b, h.rg_ids, order=operm, flags=oflags, qual=oqual, normalize_tags=True).tobytes()
        assert e.emit_sorted_bam().tobytes() == want
        assert b"".join(m for _, m in _members(e.emit_sorted_bgzf().tobytes())) == want
    finally:
        e.close()
