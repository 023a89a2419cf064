"""The coordinate sort's long runs (-m gpu): the host branches of the tie-break that no other test reaches - more run bounds than
the first read-back brings, more live positions than the rank keys take, exactly one long run, a run without a live position.

Every case is compared with the oracle's stable sort (sam/sam-types.go:425-473, :639-641) for exact equality, and the path taken is
read from the launch counts of the tie-break's kernels.  The counts are those of the sort as it stood before its host code was split
into phases (sort_plan.hpp), worked out from that code in the docstrings."""
import numpy as np
import pytest

import oracle as orc
from elprep_amd.batch import Header, batch_from_records
from elprep_amd.engine import Engine

pytestmark = pytest.mark.gpu

TIE_KERNELS = ("tie_scan", "tie_small", "large_fill", "iota", "material_rows", "material_live", "material_values", "material_keys",
               "large_ties", "large_scatter", "seg_keys")
# what every sort with a long run launches before its rounds: the scan, the short runs, the members, their strings, the live positions
MEMBERS = dict(tie_scan=1, tie_small=1, large_fill=1, iota=1, material_rows=1, material_live=1)
HEADER = Header(ref_len=np.array([100000, 100000], np.int32), rg_lib=np.array([0], np.uint16), rg_cov=np.array([0], np.uint16))


def _rec(name, pos, refid=0):
    """a forward, unpaired record: beside the name every field of the comparator is the same for all of them"""
    return dict(qname=name, flag=0, refid=refid, pos=pos, cigar="10M", mapq=30, next_refid=-1, pnext=0, tlen=0, seq="A" * 10, qual=[30] * 10, rgid=0)


def _letters(rng, n, length):
    return ["".join(map(chr, row)) for row in rng.integers(ord("a"), ord("z") + 1, (n, length))]


def many_runs():
    """260 positions x 50 records, names of 10 random letters, shuffled: 260 long runs"""
    rng = np.random.default_rng(5)
    names = _letters(rng, 260 * 50, 10)
    recs = [_rec(names[k], 100 + 7 * (k // 50)) for k in range(260 * 50)]
    return batch_from_records([recs[i] for i in rng.permutation(len(recs))])


def wide_names():
    """one run of 200 records with names of 120 random letters, and 60 records alone at their positions"""
    rng = np.random.default_rng(6)
    recs = [_rec(name, 5000) for name in _letters(rng, 200, 120)] + [_rec("s%d" % k, 10 + k) for k in range(60)]
    return batch_from_records([recs[i] for i in rng.permutation(len(recs))])


def seam_runs():
    """a run of 49 records (long) beside a run of 48 (the longest that is ranked by comparison), names of 6 random letters"""
    rng = np.random.default_rng(7)
    names = _letters(rng, 97, 6)
    recs = [_rec(names[k], 300) for k in range(49)] + [_rec(names[49 + k], 301) for k in range(48)] + [_rec("s%d" % k, 10 + k) for k in range(20)]
    return batch_from_records([recs[i] for i in rng.permutation(len(recs))])


def equal_members(runs):
    """`runs` runs of 100 records that agree in the name and in every field, between records alone at their positions"""
    rng = np.random.default_rng(8)
    recs = [_rec("same:name", 400 + r) for r in range(runs) for _ in range(100)] + [_rec("s%d" % k, 10 + k) for k in range(30)]
    return batch_from_records([recs[i] for i in rng.permutation(len(recs))])


def sort_and_count(b, tuning=None):
    """-> the permutation, {tie-break kernel: launches}"""
    e = Engine(HEADER, tuning=tuning)
    try:
        e.stage(b)
        e.profile_enable(True)
        e.profile_reset()
        perm = e.sort_coordinate()
        e.sync()
        ran = {k: v[0] for k, v in e.profile().items() if v[0] and k in TIE_KERNELS}
    finally:
        e.close()
    return perm, ran


@pytest.fixture(scope="module")
def wide():
    b = wide_names()
    return b, orc.sort_coordinate(b)


@pytest.mark.parametrize("tie_rounds", [0, 1])
def test_more_long_runs_than_the_first_read_back_brings(tie_rounds):
    """260 runs > TIE_HEAD = 256: the bounds come with a second copy.  Ten live positions of 26 values: 5 bits each, 50 bits, beside a
    run id of 9 bits (260 < 512).  tie_rounds 0: 59 bits fit one key, which holds every live position - one key kernel, one scatter, no
    comparison of groups and no round on the run id.  tie_rounds 1: the 50 bits are one LSD round, then the round on the run id."""
    b = many_runs()
    perm, ran = sort_and_count(b, {"tie_rounds": tie_rounds})
    assert np.array_equal(perm, orc.sort_coordinate(b))
    assert ran == dict(MEMBERS, material_values=1, material_keys=1, large_scatter=1, **({"seg_keys": 1} if tie_rounds else {}))


@pytest.mark.parametrize("tie_rounds", [0, 1])
def test_more_live_positions_than_the_rank_keys_take(wide, tie_rounds):
    """120 live positions > TIE_MAX_PACKED = 96: no value sets, rounds on the bytes themselves, eight positions each: ceil(120 / 8) = 15
    key kernels whatever tie_rounds says.  One long run: no round on the run id."""
    b, want = wide
    perm, ran = sort_and_count(b, {"tie_rounds": tie_rounds})
    assert np.array_equal(perm, want)
    assert ran == dict(MEMBERS, material_keys=15, large_scatter=1)


@pytest.mark.parametrize("tie_rounds", [0, 1])
def test_one_long_run_beside_the_longest_short_run(tie_rounds):
    """49 records are a long run, 48 are ranked by comparison.  Six live positions of at most 5 bits and no run id: one key holds them
    (tie_rounds 0), or one LSD round does (1) - one key kernel and one scatter either way, and no round on the run id."""
    b = seam_runs()
    perm, ran = sort_and_count(b, {"tie_rounds": tie_rounds})
    assert np.array_equal(perm, orc.sort_coordinate(b))
    assert ran == dict(MEMBERS, material_values=1, material_keys=1, large_scatter=1)


@pytest.mark.parametrize("runs", [1, 2])
def test_long_runs_of_equal_members_keep_staging_order(runs):
    """no live position: no value sets, no key kernel, no round but - two runs - the one on the run id; the members leave in staging order"""
    b = equal_members(runs)
    perm, ran = sort_and_count(b)
    assert np.array_equal(perm, orc.sort_coordinate(b))
    for r in range(runs):
        members = perm[np.nonzero(b.pos[perm] == 400 + r)[0]]
        assert members.size == 100 and np.all(np.diff(members.astype(np.int64)) > 0)
    assert ran == dict(MEMBERS, large_scatter=1, **({"seg_keys": 1} if runs > 1 else {}))
