"""The filters' kernels at the seams of their waves (64 lanes) and workgroups (256 threads): the reject counters of elp_filter_records
and elp_filter_exact_strict, which share one counting helper (one atomic per wave and counter), elp_split_classify's per-split counts
and elp_clean_sam's rebuilt CIGAR column - each against the oracle's restatement (oracle/simple_filters.py, tests/tagref.py).

Five kinds of record follow each other with period 5 - kept, rejected, rejected sr-tagged copy (state 1), already rejected by an earlier
filter (state 2), kept sr-tagged copy - and the test runs the five rotations of the pattern, so that every kind stands in front of and
behind every multiple of 64 and 256 in one of them."""
import numpy as np
import pytest

import oracle as orc
from elprep_amd.batch import Batch
from elprep_amd.engine import Engine
from oracle import simple_filters as sf
from tests import tagref
from tests.common import dataset
from tests.test_gpu_tag_filters import _expected_records

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 255, 256, 257, 513)
KEPT, REJECTED, REJECTED_TAGGED, ALREADY, KEPT_TAGGED = range(5)
MIN_MAPQ = 20
GOOD = [tagref.int_field(b"X0", b"C", 1), tagref.int_field(b"X1", b"i", 0), tagref.int_field(b"XM", b"C", 0), tagref.int_field(b"XO", b"c", 0),
        tagref.int_field(b"XG", b"S", 0)]
BAD = [GOOD[1:], [tagref.int_field(b"X0", b"C", 2)] + GOOD[1:], GOOD[:4], GOOD[:2] + [tagref.int_field(b"XM", b"s", -1)] + GOOD[3:]]


@pytest.fixture(scope="module")
def data():
    cfg, b, h, refs, sites = dataset("tiny", 300, 4, 0.03)
    assert b.n >= max(SIZES)
    return b, h


def _with(b, **over):
    cols = {name: getattr(b, name) for name in b.__dataclass_fields__}
    cols.update(over)
    return Batch(**cols)


def _pattern(b, n, shift):
    """-> the first n records made into the five kinds (the kind of record i is (i + shift) % 5), and the kinds.  A record that is to be
    rejected has MAPQ 5 (elp_filter_records, min_mapq 20) and misses one of the strict filter's conditions; one that an earlier filter
    rejected has FLAG 0x400 (remove_duplicates runs first), with and without the sr tag."""
    kind = (np.arange(n) + shift) % 5
    t = b.take(np.arange(n))
    rej = (kind == REJECTED) | (kind == REJECTED_TAGGED)
    flag = (t.flag & ~np.uint16(0x400)) | np.where(kind == ALREADY, 0x400, 0).astype(np.uint16)
    mapq = np.where(rej | ((kind == ALREADY) & (np.arange(n) % 2 == 0)), 5, 60).astype(np.uint8)
    has_sr = ((kind == REJECTED_TAGGED) | (kind == KEPT_TAGGED) | ((kind == ALREADY) & (np.arange(n) // 5 % 2 == 1))).astype(np.uint8)
    return _with(t, flag=flag, mapq=mapq, has_sr=has_sr), kind, has_sr


@pytest.mark.parametrize("n", SIZES)
def test_reject_counters_at_wave_and_workgroup_seams(data, n):
    b0, h = data
    e = Engine(h)
    try:
        for shift in range(5):
            b, kind, has_sr = _pattern(b0, n, shift)
            extra = [BAD[i % len(BAD)] if kind[i] in (REJECTED, REJECTED_TAGGED) else GOOD for i in range(n)]
            raw = np.frombuffer(tagref.append_fields(orc.bam_encode(b, h.rg_ids).tobytes(), extra), np.uint8)
            recs = tagref.records(raw.tobytes())
            # the oracle's word on every record, for either filter
            by_mapq = ~sf.keep_mask(b, min_mapq=MIN_MAPQ)
            by_fields = np.asarray([tagref.strict_keep(r) == "reject" for r in recs])
            dup = ~sf.keep_mask(b, remove_duplicates=True)
            assert np.array_equal(dup, kind == ALREADY)
            kept = np.nonzero((kind == KEPT))[0]
            want = _expected_records(b, h.rg_ids, kept[orc.sort_coordinate(b.take(kept))], None, None, extra) if kept.size else None
            for which, rejects in (("records", by_mapq), ("strict", by_fields)):
                live = ~dup  # what the filter under test still looks at
                assert np.array_equal(rejects & live, (kind == REJECTED) | (kind == REJECTED_TAGGED))
                e.reset()
                e.set_read_group_ids(h.rg_ids)
                e.stage_bam(raw)
                assert e.filter_records(remove_duplicates=True) == int((dup & (has_sr == 0)).sum())
                got = e.filter_records(min_mapq=MIN_MAPQ) if which == "records" else e.filter_exact_strict()
                assert got == int((rejects & live & (has_sr == 0)).sum()) == int((kind == REJECTED).sum()), (which, n, shift)
                assert e.n_sorted == kept.size, (which, n, shift)
                if want is not None:  # (no record is output otherwise: n_sorted has said so)
                    e.sort_coordinate()
                    assert e.emit_sorted_bam().tobytes() == b"".join(want), (which, n, shift)
                # nothing is left for a second call to reject
                assert (e.filter_records(min_mapq=MIN_MAPQ) if which == "records" else e.filter_exact_strict()) == 0
    finally:
        e.close()


@pytest.mark.parametrize("n_groups", (1, 3))
@pytest.mark.parametrize("n", SIZES)
def test_split_classify_at_the_seams(data, n, n_groups):
    """Split, spread and the per-split counts against split_records: RNAME and RNEXT walk through "*" and every contig with different
    periods, so that spread and plain records of every group stand on both sides of the seams."""
    b0, h = data
    i = np.arange(n)
    refid = ((i * 7) % (h.n_ref + 1) - 1).astype(np.int32)
    next_refid = (((i // 3) * 5 + i) % (h.n_ref + 1) - 1).astype(np.int32)
    b = _with(b0.take(i), refid=refid, next_refid=next_refid)
    gof = (np.arange(h.n_ref) % n_groups + 1).astype(np.int32)
    want_split, want_spread = sf.split_records(b, gof)
    e = Engine(h)
    try:
        e.stage(b)
        split, spread, counts = e.split_classify(gof, n_groups)
        assert np.array_equal(split, want_split) and np.array_equal(spread, want_spread)
        want_counts = [int((want_split == g).sum()) for g in range(n_groups + 1)] + [int(want_spread.sum())]
        assert counts.tolist() == want_counts and sum(want_counts[:-1]) == n
    finally:
        e.close()


def test_clean_sam_rewrites_at_the_seams(data):
    """257 records of which the first of the first workgroup, its last and the first of the second hang over their reference's end: the
    rebuilt CIGAR column (lengths, scan, copy) against the oracle's, through the emitted records."""
    b0, h = data
    n, at = 257, np.array([0, 255, 256])
    t = b0.take(np.arange(n))
    refid, pos, flag = t.refid.copy(), t.pos.copy(), t.flag.copy()
    refid[at] = 0
    pos[at] = h.ref_len[0] - 10
    flag[at] &= ~np.uint16(0x4)
    b = _with(t, refid=refid, pos=pos, flag=flag)
    want, changed = sf.clean_sam(b, h.ref_len)
    rewritten = [k for k in range(n) if not np.array_equal(want.cigar[int(want.cigar_off[k]):int(want.cigar_off[k + 1])],
                                                             b.cigar[int(b.cigar_off[k]):int(b.cigar_off[k + 1])])]
    assert changed == 3 and rewritten == at.tolist()
    e = Engine(h)
    try:
        e.set_read_group_ids(h.rg_ids)
        e.stage_bam(orc.bam_encode(b, h.rg_ids))
        assert e.clean_sam() == 3
        e.sort_coordinate()
        perm = orc.sort_coordinate(want)
        assert e.emit_sorted_bam().tobytes() == orc.bam_encode(want, h.rg_ids, order=perm[:orc.num_sorted(want)], normalize_tags=True).tobytes()
    finally:
        e.close()
