"""GPU tests (-m gpu) of elp_replace_reference_dictionary: --replace-reference-sequences on records staged under the OLD header.

The expected side is the oracle on a batch PREPARED on the host: the map applied to REFID / RNEXT with numpy, the records of contigs that
left the dictionary removed, a header with the new LN values, references and known sites re-keyed to the new refids
(ReplaceReferenceSequenceDictionary, filters/simple-filters.go:32-60, then AddREFID under the new header.SQ, :208-231).  The device side
stages the ORIGINAL records under the ORIGINAL header, calls the operator, and then runs the same whole path.  One test (not gpu) checks
with the oracle alone that the prepared inputs hold what the cases are about: kept records whose mate is on a dropped contig, and kept
unmapped records."""
import ctypes as C

import numpy as np
import pytest

import oracle as orc
from elprep_amd.batch import Batch, Header
from elprep_amd.engine import ElpError, Engine
from tests import tagref
from tests.common import dataset
from tests.test_gpu_round4 import _bgzf as _make_bgzf
from tests.test_gpu_round4 import _members
from tests.test_gpu_tag_filters import _device_path, _names, _oracle_path, _size_query

ELP_ERR_ARG = -1
REF_LDS = 256  # elprep_amd/csrc/bqsr_common.hpp: up to this many old contigs the map is held in LDS


# ---------------------------------------------------------------------------------------------------------------- inputs
def _with(b, **cols):
    c = {name: getattr(b, name) for name in b.__dataclass_fields__}
    c.update(cols)
    return Batch(**c)


def _header(h, names, ref_len):
    return Header(ref_len=np.asarray(ref_len, np.int32), rg_lib=h.rg_lib, rg_cov=h.rg_cov, n_lib=h.n_lib, n_cov=h.n_cov, ref_names=list(names),
                  rg_ids=h.rg_ids, lib_names=h.lib_names, cov_names=h.cov_names)


def _apply_map(col, m):
    """refid = refid < 0 ? -1 : new_of_old[refid]"""
    m = np.asarray(m, np.int32)
    return np.where(col < 0, -1, m[np.clip(col, 0, None)]).astype(np.int32)


class Case:
    """old side: b, h, refs, sites; new side: the map, header, references and sites under the new refids"""

    def __init__(self, name, n_pairs=3000, seed=21):
        cfg, b, h, refs, sites = dataset("tiny", n_pairs, seed, 0.03)
        assert h.n_ref == 3
        names, lens = list(h.ref_names), h.ref_len.tolist()
        extra_ref = lambda ln, s: np.random.default_rng(s).choice(np.frombuffer(b"ACGT", np.uint8), ln)
        none = np.zeros((0, 2), np.int32)
        if name == "many_contigs":  # more old contigs than the LDS map holds: the HBM table path (padding as test_gpu_ragged.test_many_contigs)
            pad = 260
            names = names + ["pad%d" % k for k in range(pad)]
            lens = lens + [500 + 7 * (k % 5) for k in range(pad)]
            refs = list(refs) + [extra_ref(lens[3 + k], 100 + k) for k in range(pad)]
            sites = list(sites) + [none] * pad
            h = _header(h, names, lens)
            assert h.n_ref > REF_LDS
            new_names = names[3:][::-1] + [names[2], names[0]]  # the padding reversed in front, chrC, chrA; chrB leaves
        else:
            new_names = {"identity": names, "reversed": names[::-1], "one_dropped": [names[0], names[2]], "first_and_last_dropped": [names[1]],
                         "two_in_front": ["extra0", "extra1"] + names, "all_dropped": ["other"]}[name]
        self.name, self.b, self.h, self.refs, self.sites = name, b, h, list(refs), list(sites)
        self.map = np.asarray([new_names.index(nm) if nm in new_names else -1 for nm in names], np.int32)
        self.dropped = np.nonzero(self.map < 0)[0]
        extra_len = {"extra0": 5000, "extra1": 7000, "other": 4000}
        new_len, self.new_refs, self.new_sites = [], [], []
        for j, nm in enumerate(new_names):
            if nm in names:
                r = names.index(nm)
                new_len.append(lens[r]); self.new_refs.append(self.refs[r]); self.new_sites.append(self.sites[r])
            else:
                new_len.append(extra_len[nm]); self.new_refs.append(extra_ref(extra_len[nm], 7 + j)); self.new_sites.append(none)
        self.new_h = _header(h, new_names, new_len)
        if self.dropped.size:
            self.b = self._redirect(self.b)
        b = self.b
        self.keep = (b.refid < 0) | (self.map[np.clip(b.refid, 0, None)] >= 0)
        self.kept = np.nonzero(self.keep)[0]
        self.full = _with(b, refid=_apply_map(b.refid, self.map), next_refid=_apply_map(b.next_refid, self.map))  # every record, new refids
        self.prepared = self.full.take(self.kept)

    def _mate_left(self, b):
        keep = (b.refid < 0) | (self.map[np.clip(b.refid, 0, None)] >= 0)
        return keep & (b.next_refid >= 0) & (self.map[np.clip(b.next_refid, 0, None)] < 0)

    def _redirect(self, b):
        """at least 1 % of the kept records must have their mate on a dropped contig: where the generator gave too few, RNEXT / PNEXT
        of every 40th kept, mapped, paired record (where no mapped record is kept: of every 3rd kept unplaced one) are pointed at a dropped contig"""
        keep = (b.refid < 0) | (self.map[np.clip(b.refid, 0, None)] >= 0)
        if self._mate_left(b).sum() >= 0.015 * keep.sum():
            return b
        paired = keep & ((b.flag & 0x1) != 0) & ~self._mate_left(b)
        cand = np.nonzero(paired & (b.refid >= 0))[0][::40]
        if cand.size == 0:  # every contig leaves: the kept records are the unplaced ones (RNAME *), and every 3rd of them gets a mate there
            cand = np.nonzero(paired)[0][::3]
        nr, pn = b.next_refid.copy(), b.pnext.copy()
        nr[cand] = self.dropped[np.arange(cand.size) % self.dropped.size]
        pn[cand] = 1 + (cand * 37) % 20000
        return _with(b, next_refid=nr, pnext=pn)

    def counts(self):
        return int(self._mate_left(self.b).sum()), int((self.keep & (self.b.refid < 0)).sum())


CASES = ["reversed", "one_dropped", "first_and_last_dropped", "two_in_front", "all_dropped", "many_contigs"]
DROPPING = ["one_dropped", "first_and_last_dropped", "many_contigs", "all_dropped"]  # every case that drops a contig


def _full_flags_qual(c, oflags, oqual):
    """the oracle's flags and qualities of the kept records, scattered to the original indices"""
    b = c.b
    flags = b.flag.copy()
    flags[c.kept] = oflags
    qual = b.qual.copy()
    lo, ln = b.qual_off[:-1].astype(np.int64)[c.kept], np.diff(b.qual_off.astype(np.int64))[c.kept]
    dst = np.repeat(lo - np.concatenate([[0], np.cumsum(ln)[:-1]]), ln) + np.arange(int(ln.sum()))
    if oqual is not None:
        qual[dst] = oqual
    return flags, qual, dst


def _refids_of(bam_bytes):
    recs = tagref.records(bam_bytes)
    return (np.asarray([int.from_bytes(r[4:8], "little", signed=True) for r in recs], np.int32),
            np.asarray([int.from_bytes(r[24:28], "little", signed=True) for r in recs], np.int32))


# ---------------------------------------------------------------------------------------------------------------- CPU: the inputs
@pytest.mark.parametrize("name", DROPPING)
def test_prepared_inputs_meet_the_condition(name):
    """oracle only: in every case that drops a contig >= 1 % of the KEPT records have their mate on a dropped contig and at least one
    kept record is unmapped with refid -1; the prepared batch goes through the oracle's path and its records carry the new refids"""
    c = Case(name)
    mate_left, unmapped = c.counts()
    assert mate_left >= 0.01 * c.kept.size and mate_left > 0, (mate_left, c.kept.size)
    assert (c.prepared.next_refid[(c.b.next_refid[c.kept] >= 0) & (c.map[np.clip(c.b.next_refid[c.kept], 0, None)] < 0)] == -1).all()
    if name == "all_dropped":
        assert (c.prepared.refid == -1).all() and (c.prepared.next_refid == -1).all() and (c.b.next_refid[c.kept] >= 0).sum() == mate_left
    assert unmapped >= 1
    assert 0 < c.kept.size < c.b.n
    assert c.prepared.refid.max() < c.new_h.n_ref and c.prepared.next_refid.max() < c.new_h.n_ref
    oflags = orc.mark_duplicates(c.prepared, c.new_h)
    operm = orc.sort_coordinate(c.prepared, oflags)
    assert sorted(operm.tolist()) == list(range(c.kept.size))
    rid, nrid = _refids_of(orc.bam_encode(c.full, c.h.rg_ids, order=c.kept[operm], flags=_full_flags_qual(c, oflags, None)[0], normalize_tags=True).tobytes())
    assert np.array_equal(rid, c.prepared.refid[operm]) and np.array_equal(nrid, c.prepared.next_refid[operm])


# ---------------------------------------------------------------------------------------------------------------- GPU: the whole path
def _stage(e, c, how):
    if how == "columns":
        e.stage(c.b)
        return
    e.set_read_group_ids(c.h.rg_ids)
    raw = orc.bam_encode(c.b, c.h.rg_ids)
    if how == "bam":
        e.stage_bam(raw)
    else:
        e.stage_bgzf(np.frombuffer(_make_bgzf(raw.tobytes(), 6), np.uint8))
    assert e.n == c.b.n


def _check_whole_path(c, how):
    oflags, operm, otabs, oqual = _oracle_path(c.prepared, c.new_h, c.new_refs, c.new_sites)
    _, octr, _ = orc.dup_metrics(c.prepared, c.new_h, operm, 100)
    full_flags, full_qual, qdst = _full_flags_qual(c, oflags, oqual)
    e = Engine(c.h)
    try:
        _stage(e, c, how)
        n_rej = e.replace_reference_dictionary(c.map, c.new_h.ref_len)
        assert n_rej == c.b.n - c.kept.size and e.n_sorted == c.kept.size and e.n == c.b.n
        flags = e.mark_duplicates(True)
        perm = e.sort_coordinate()
        ctr = e.dup_metrics(100)
        assert np.array_equal(flags[c.kept], oflags)
        assert np.array_equal(perm[:c.kept.size], c.kept[operm])
        assert set(perm[c.kept.size:].tolist()) == set(np.nonzero(~c.keep)[0].tolist())
        assert np.array_equal(ctr, octr)
        _, _, tabs, qual = _device_path(e, c.new_h, c.new_refs, c.new_sites)  # (marks and sorts again: same results; references under the NEW refids)
        assert all(np.array_equal(a, o) for a, o in zip(tabs, otabs))
        assert np.array_equal(qual[qdst], oqual)
        assert np.array_equal(e.flags()[c.kept], oflags) and np.array_equal(e.permutation()[:c.kept.size], c.kept[operm])
        if how == "columns":
            return
        want = orc.bam_encode(c.full, c.h.rg_ids, order=c.kept[operm], flags=full_flags, qual=full_qual, normalize_tags=True).tobytes()
        got = e.emit_sorted_bam().tobytes()
        assert got == want and _size_query(e) == len(got)
        rid, nrid = _refids_of(got)  # refID at byte 4 and next_refID at byte 24 of each record (block_size in front): the NEW dictionary's
        assert np.array_equal(rid, c.prepared.refid[operm]) and np.array_equal(nrid, c.prepared.next_refid[operm])
        assert b"".join(m for _, m in _members(e.emit_sorted_bgzf().tobytes())) == want
        # queryname order of the same records
        names = _names(c.prepared)
        qperm = np.asarray(sorted(range(c.kept.size), key=lambda i: names[i]), dtype=np.uint32)
        assert np.array_equal(e.sort_queryname()[:c.kept.size], c.kept[qperm])
        assert e.emit_sorted_bam().tobytes() == orc.bam_encode(c.full, c.h.rg_ids, order=c.kept[qperm], flags=full_flags, qual=full_qual,
                                                               normalize_tags=True).tobytes()
    finally:
        e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_replace_dictionary_whole_path_from_bam(name):
    c = Case(name)
    if name in DROPPING:
        mate_left, unmapped = c.counts()
        assert mate_left >= 0.01 * c.kept.size and unmapped >= 1
    _check_whole_path(c, "bam")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["one_dropped", "two_in_front"])
def test_replace_dictionary_whole_path_from_bgzf(name):
    _check_whole_path(Case(name), "bgzf")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["reversed", "first_and_last_dropped", "many_contigs"])
def test_replace_dictionary_whole_path_from_columns(name):
    _check_whole_path(Case(name), "columns")


def _plain_run(e, c):
    e.set_read_group_ids(c.h.rg_ids)
    e.stage_bam(orc.bam_encode(c.b, c.h.rg_ids))
    return e


def _columns(e):
    """every column the call may write, as the host can read them: FLAG, and REFID / RNEXT / the record states through a sort and the emitter"""
    e.sort_queryname()
    return e.flags().tobytes(), e.emit_sorted_bam().tobytes(), e.n_sorted, _size_query(e)


@pytest.mark.gpu
def test_identity_map_equals_a_run_without_the_call():
    c = Case("identity")
    assert c.map.tolist() == [0, 1, 2] and c.kept.size == c.b.n
    outs = []
    for call in (False, True):
        e = _plain_run(Engine(c.h), c)
        try:
            if call:
                assert e.replace_reference_dictionary(c.map, c.h.ref_len) == 0
            flags, perm, tabs, qual = _device_path(e, c.h, c.refs, c.sites)
            outs.append((flags.tobytes(), perm.tobytes(), [t.tobytes() for t in tabs], qual.tobytes(), e.emit_sorted_bam().tobytes(),
                         b"".join(m for _, m in _members(e.emit_sorted_bgzf().tobytes()))))
        finally:
            e.close()
    assert outs[0] == outs[1]


# ---------------------------------------------------------------------------------------------------------------- GPU: interplay
@pytest.mark.gpu
def test_clean_sam_in_front_clips_against_the_old_length():
    """CleanSam stands in front of the replacement in filters1 (cmd/filter.go:747-749, :752-755) and clips against the OLD LN: a new
    dictionary whose LN is shorter than many reads' ends changes neither the clip count nor a CIGAR"""
    from oracle import simple_filters as sf
    cfg, b, h, refs, sites = dataset("tiny", 8000, 9, 0.03)
    cut = np.array([41000, 30000, 22000], np.int32)   # (the construction of test_gpu_round4.test_clean_sam_against_the_oracle)
    keep = np.nonzero((b.refid < 0) | (b.pos <= cut[np.clip(b.refid, 0, None)] - 140))[0]
    over = np.nonzero((b.refid >= 0) & (b.pos > cut[np.clip(b.refid, 0, None)] - 140) & (b.pos <= cut[np.clip(b.refid, 0, None)] - 20))[0]
    bb = b.take(np.sort(np.concatenate([keep, over])))
    h_old = _header(h, h.ref_names, cut)
    short = np.array([9000, 8000, 7000], np.int32)
    assert ((bb.refid >= 0) & (bb.pos > short[np.clip(bb.refid, 0, None)])).sum() > 1000  # reads that lie behind the NEW ends altogether
    want, n_changed = sf.clean_sam(bb, cut)
    assert n_changed > 30
    oflags = orc.mark_duplicates(want, h_old)
    operm = orc.sort_coordinate(want, oflags)
    want_bytes = orc.bam_encode(want, h.rg_ids, order=operm, flags=oflags, normalize_tags=True).tobytes()
    outs = []
    for call in (False, True):
        e = Engine(h_old)
        try:
            e.set_read_group_ids(h.rg_ids)
            e.stage_bam(orc.bam_encode(bb, h.rg_ids))
            assert e.clean_sam() == n_changed
            if call:
                assert e.replace_reference_dictionary([0, 1, 2], short) == 0
            assert np.array_equal(e.mark_duplicates(True), oflags) and np.array_equal(e.sort_coordinate(), operm)
            outs.append(e.emit_sorted_bam().tobytes())
        finally:
            e.close()
    assert outs[0] == want_bytes and outs[1] == want_bytes


@pytest.mark.gpu
def test_filter_records_in_front_counts_add_up():
    from oracle import simple_filters as sf
    c = Case("one_dropped")
    first = sf.keep_mask(c.b, min_mapq=20)
    assert 0 < (~first & ~c.keep).sum() and 0 < (first & ~c.keep).sum() and 0 < (~first & c.keep).sum()
    e = Engine(c.h)
    try:
        _plain_run(e, c)
        assert e.filter_records(min_mapq=20) == int((~first).sum())
        assert e.replace_reference_dictionary(c.map, c.new_h.ref_len) == int((first & ~c.keep).sum())  # a record rejected twice is counted once
        live = np.nonzero(first & c.keep)[0]
        assert e.n_sorted == live.size
        assert e.filter_records(min_mapq=20) == 0
        pb = c.full.take(live)
        oflags = orc.mark_duplicates(pb, c.new_h)
        operm = orc.sort_coordinate(pb, oflags)
        assert np.array_equal(e.mark_duplicates(True)[live], oflags)
        assert np.array_equal(e.sort_coordinate()[:live.size], live[operm])
        full_flags = c.b.flag.copy()
        full_flags[live] = oflags
        assert e.emit_sorted_bam().tobytes() == orc.bam_encode(c.full, c.h.rg_ids, order=live[operm], flags=full_flags, normalize_tags=True).tobytes()
    finally:
        e.close()


@pytest.mark.gpu
def test_sr_tagged_copies_are_renumbered_and_not_counted_again():
    c = Case("one_dropped")
    sr = (np.arange(c.b.n) % 5 == 0).astype(np.uint8)
    b = _with(c.b, has_sr=sr)
    e = Engine(c.h)
    try:
        e.stage(b)
        assert e.n_sorted == int((sr == 0).sum())
        assert e.replace_reference_dictionary(c.map, c.new_h.ref_len) == int(((sr == 0) & ~c.keep).sum())
        assert e.n_sorted == int(((sr == 0) & c.keep).sum())
        pb = _with(c.full, has_sr=sr).take(c.kept)
        assert np.array_equal(e.mark_duplicates(True)[c.kept], orc.mark_duplicates(pb, c.new_h))
    finally:
        e.close()


@pytest.mark.gpu
def test_tag_filter_and_replace_read_group_with_the_replacement():
    c = Case("one_dropped")
    h1_old = Header.from_read_groups(c.h.ref_names, c.h.ref_len, [{"ID": "new", "LB": "libN", "PU": "FC9.1"}])
    h1_new = Header.from_read_groups(c.new_h.ref_names, c.new_h.ref_len, [{"ID": "new", "LB": "libN", "PU": "FC9.1"}])
    zero = np.zeros(c.b.n, np.uint16)
    prepared0 = _with(c.full, rgid=zero).take(c.kept)
    oflags, operm, otabs, oqual = _oracle_path(prepared0, h1_new, c.new_refs, c.new_sites)
    full_flags, full_qual, qdst = _full_flags_qual(c, oflags, oqual)
    want0 = [tagref.replace_read_group(r, "new") for r in
             tagref.records(orc.bam_encode(c.full, c.h.rg_ids, order=c.kept[operm], flags=full_flags, qual=full_qual, normalize_tags=True).tobytes())]
    e = Engine(h1_old)
    try:
        e.set_replace_read_group("new")
        e.stage_bam(orc.bam_encode(c.b, c.h.rg_ids))
        e.set_tag_filter(remove=["XT"])                          # set in front of the call: it stays
        assert e.replace_reference_dictionary(c.map, h1_new.ref_len) == c.b.n - c.kept.size
        flags, perm, tabs, qual = _device_path(e, h1_new, c.new_refs, c.new_sites)
        assert np.array_equal(flags[c.kept], oflags) and np.array_equal(perm[:c.kept.size], c.kept[operm])
        assert all(np.array_equal(a, o) for a, o in zip(tabs, otabs)) and np.array_equal(qual[qdst], oqual)
        assert e.emit_sorted_bam().tobytes() == b"".join(tagref.apply_tag_filter(r, remove=["XT"]) for r in want0)
        for f in (dict(keep=["RG", "NM"]), dict(remove=["RG", "AS"])):
            e.set_tag_filter(**f)
            assert e.emit_sorted_bam().tobytes() == b"".join(tagref.apply_tag_filter(r, **f) for r in want0), f
        e.set_tag_filter()
        assert e.emit_sorted_bam().tobytes() == b"".join(want0)
    finally:
        e.close()


@pytest.mark.gpu
def test_two_calls_equal_one_call_with_the_composed_map():
    c = Case("two_in_front")                                     # old 3 -> 5 contigs: [2, 3, 4]
    second = np.asarray([3, -1, 0, -1, 1], np.int32)             # extra0 -> 3, extra1 leaves, chrA -> 0, chrB leaves, chrC -> 1
    len2 = np.asarray([60000, 30000, 777, 5000], np.int32)
    composed = _apply_map(c.map, second)
    assert composed.tolist() == [0, -1, 1]
    outs = []
    for two in (True, False):
        e = _plain_run(Engine(c.h), c)
        try:
            if two:
                n_rej = e.replace_reference_dictionary(c.map, c.new_h.ref_len) + e.replace_reference_dictionary(second, len2)
            else:
                n_rej = e.replace_reference_dictionary(composed, len2)
            flags = e.mark_duplicates(True)
            perm = e.sort_coordinate()
            outs.append((n_rej, e.n_sorted, flags.tobytes(), perm.tobytes(), e.emit_sorted_bam().tobytes()))
        finally:
            e.close()
    assert outs[0] == outs[1] and outs[0][0] == int((c.b.refid == 1).sum())


# ---------------------------------------------------------------------------------------------------------------- GPU: errors and state
@pytest.mark.gpu
def test_bad_arguments_change_nothing():
    c = Case("one_dropped")
    e = _plain_run(Engine(c.h), c)
    try:
        before = _columns(e)
        for bad_map, n_new in (([0, 2, 1], 2), ([0, -2, 1], 2), ([0, 1, 5], 3)):
            ln = np.asarray([60000, 30000, 100][:n_new], np.int32)
            with pytest.raises(ElpError) as ei:
                e.replace_reference_dictionary(bad_map, ln)
            assert ei.value.code == ELP_ERR_ARG, bad_map
        m = np.asarray([0, -1, 1], np.int32)
        n = C.c_uint64(99)
        assert e.L.elp_replace_reference_dictionary(e.h, C.c_void_p(m.ctypes.data), -1, C.c_void_p(0), C.byref(n)) == ELP_ERR_ARG
        assert e.L.elp_replace_reference_dictionary(e.h, C.c_void_p(0), 2, C.c_void_p(m.ctypes.data), C.byref(n)) == ELP_ERR_ARG
        assert e.L.elp_replace_reference_dictionary(e.h, C.c_void_p(m.ctypes.data), 2, C.c_void_p(0), C.byref(n)) == ELP_ERR_ARG
        assert _columns(e) == before
        e.stage_bam(orc.bam_encode(c.b.take(np.arange(10)), c.h.rg_ids))   # no call went through: staging is still allowed
        assert e.n == c.b.n + 10
    finally:
        e.close()


@pytest.mark.gpu
@pytest.mark.fresh_only
def test_missing_header_is_refused():
    from elprep_amd import _lib
    L = _lib.hip()
    h = C.c_void_p()
    assert L.elp_create(0, C.byref(h)) == 0
    try:
        m = np.zeros(1, np.int32)
        assert L.elp_replace_reference_dictionary(h, C.c_void_p(m.ctypes.data), 1, C.c_void_p(m.ctypes.data), None) == ELP_ERR_ARG
        assert b"elp_set_header" in L.elp_last_error(h)
    finally:
        L.elp_destroy(h)


@pytest.mark.gpu
def test_staging_is_refused_until_reset_and_reset_restores_the_header():
    c = Case("first_and_last_dropped")
    raw = orc.bam_encode(c.b, c.h.rg_ids)
    plain = Engine(c.h)
    try:
        _plain_run(plain, c)
        want = _device_path(plain, c.h, c.refs, c.sites)
        want_bytes = plain.emit_sorted_bam().tobytes()
    finally:
        plain.close()
    e = _plain_run(Engine(c.h), c)
    try:
        e.replace_reference_dictionary(c.map, c.new_h.ref_len)
        for stage in (lambda: e.stage_bam(raw), lambda: e.stage(c.b), lambda: e.stage_columns(c.b),
                      lambda: e.stage_bgzf(np.frombuffer(_make_bgzf(raw.tobytes(), 6), np.uint8))):
            with pytest.raises(ElpError) as ei:
                stage()
            assert ei.value.code == ELP_ERR_ARG and "dictionary" in str(ei.value)
        assert e.n == c.b.n
        with pytest.raises(ElpError):
            e.set_reference(1, c.refs[1])                        # the new dictionary has one contig
        e.reset()
        e.stage_bam(raw)                                         # the next file of the same header, without the call
        got = _device_path(e, c.h, c.refs, c.sites)
        assert all(np.array_equal(a, b) for a, b in zip((got[0], got[1], *got[2], got[3]), (want[0], want[1], *want[2], want[3])))
        assert e.emit_sorted_bam().tobytes() == want_bytes
        # elp_set_header ends the state too
        e.replace_reference_dictionary(c.map, c.new_h.ref_len)
        hs = c.h.as_struct()
        e._check(e.L.elp_set_header(e.h, C.byref(hs)))
        e.reset()
        e.set_read_group_ids(c.h.rg_ids)
        e.stage_bam(raw)
        assert np.array_equal(e.mark_duplicates(True), want[0])
    finally:
        e.close()


@pytest.mark.gpu
def test_merged_emit_between_a_replaced_and_an_unreplaced_context_is_refused():
    c = Case("reversed")
    groups, spread = _plain_run(Engine(c.h), c), Engine(c.h)
    try:
        spread.set_read_group_ids(c.h.rg_ids)
        spread.stage_bam(orc.bam_encode(c.b.take(np.arange(50)), c.h.rg_ids))
        groups.replace_reference_dictionary(c.map, c.new_h.ref_len)
        for e in (groups, spread):
            e.mark_duplicates(True)
            e.sort_coordinate()
        with pytest.raises(ElpError) as ei:
            groups.emit_merged_bam(spread)
        assert ei.value.code == ELP_ERR_ARG and "dictionary" in str(ei.value)
        with pytest.raises(ElpError) as ei:
            spread.emit_merged_bam(groups)
        assert ei.value.code == ELP_ERR_ARG and "dictionary" in str(ei.value)
        spread.replace_reference_dictionary(c.map, c.new_h.ref_len)   # both replaced, with equal results: the stream is made
        spread.mark_duplicates(True)
        spread.sort_coordinate()
        got = tagref.records(groups.emit_merged_bam(spread).tobytes())
        assert len(got) == groups.n_sorted + spread.n_sorted
    finally:
        groups.close()
        spread.close()


@pytest.mark.gpu
def test_python_face_checks_the_length_of_the_map():
    c = Case("two_in_front")
    e = _plain_run(Engine(c.h), c)
    try:
        with pytest.raises(ElpError) as ei:
            e.replace_reference_dictionary([0, 1], c.h.ref_len)          # the dictionary in force has three contigs
        assert ei.value.code == ELP_ERR_ARG
        e.replace_reference_dictionary(c.map, c.new_h.ref_len)           # ... now five
        with pytest.raises(ElpError) as ei:
            e.replace_reference_dictionary([0, 1, 2], c.h.ref_len)
        assert ei.value.code == ELP_ERR_ARG
        e.reset()                                                        # ... and three again
        e.stage_bam(orc.bam_encode(c.b, c.h.rg_ids))
        assert e.replace_reference_dictionary([0, 1, 2], c.h.ref_len) == 0
    finally:
        e.close()


@pytest.mark.gpu
def test_set_header_behind_a_replacement_drops_the_references():
    """references set under the new refids do not pass into the next header's numbering: the gather asks for them again"""
    c = Case("reversed")
    e = _plain_run(Engine(c.h), c)
    try:
        e.replace_reference_dictionary(c.map, c.new_h.ref_len)
        for r in range(c.new_h.n_ref):
            e.set_reference(r, c.new_refs[r])
            e.set_known_sites(r, c.new_sites[r])
        hs = c.h.as_struct()
        e._check(e.L.elp_set_header(e.h, C.byref(hs)))
        e.reset()
        e.set_read_group_ids(c.h.rg_ids)
        e.stage_bam(orc.bam_encode(c.b, c.h.rg_ids))
        e.mark_duplicates(True)
        with pytest.raises(ElpError) as ei:
            e.recalibrate(500)
        assert ei.value.code == ELP_ERR_ARG and "reference" in str(ei.value)
    finally:
        e.close()


@pytest.mark.gpu
def test_copy_between_a_replaced_and_an_unreplaced_context_is_refused():
    c = Case("reversed")
    a, other = _plain_run(Engine(c.h), c), Engine(c.h)
    try:
        a.replace_reference_dictionary(c.map, c.new_h.ref_len)
        with pytest.raises(ElpError) as ei:
            other.copy_records_from(a, np.arange(10))
        assert ei.value.code == ELP_ERR_ARG and other.n == 0
        # two contexts that both replaced theirs, with equal results, pass
        other.set_read_group_ids(c.h.rg_ids)
        other.stage_bam(orc.bam_encode(c.b.take(np.arange(5)), c.h.rg_ids))
        other.replace_reference_dictionary(c.map, c.new_h.ref_len)
        other.copy_records_from(a, np.arange(10))
        assert other.n == 15
        assert np.array_equal(other.flags()[5:], c.b.flag[:10])
    finally:
        a.close()
        other.close()


@pytest.mark.gpu
def test_a_permutation_made_before_the_call_is_not_served():
    c = Case("reversed")
    e = _plain_run(Engine(c.h), c)
    try:
        e.mark_duplicates(True)
        stale = e.sort_coordinate()
        e.snapshot()
        e.replace_reference_dictionary(c.map, c.new_h.ref_len)
        oflags = orc.mark_duplicates(c.prepared, c.new_h)
        fresh = orc.sort_coordinate(c.prepared, oflags)
        assert not np.array_equal(stale, fresh)
        try:
            got = e.permutation()
        except ElpError as err:
            assert err.code == ELP_ERR_ARG                       # the sort is required again
        else:
            assert np.array_equal(got, fresh)
        with pytest.raises(ElpError) as ei:
            e.rollback()                                         # a rollback cannot restore refids: the snapshot went
        assert ei.value.code == ELP_ERR_ARG
        assert np.array_equal(e.mark_duplicates(True), oflags) and np.array_equal(e.sort_coordinate(), fresh)
    finally:
        e.close()


@pytest.mark.gpu
def test_kernel_is_timed_under_its_own_name():
    c = Case("one_dropped")
    e = _plain_run(Engine(c.h), c)
    try:
        e.profile_enable(True)
        e.replace_reference_dictionary(c.map, c.new_h.ref_len)
        prof = e.profile()
        e.profile_enable(False)
        assert prof["replace_dictionary"][0] == 1 and prof["replace_dictionary"][1] > 0
    finally:
        e.close()
