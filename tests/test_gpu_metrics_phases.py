"""GPU tests (-m gpu): the early exits of the duplication-metrics pass's phases (metrics.hip: counters -> groups -> small sets -> large
sets -> origins -> read back).  Five read sets, each ending the pass at another phase, on ONE context in the order below - every later
and smaller call finds the larger call's scratch behind it - and once more on fresh contexts.  Every case: counters and all three
histograms (8 bins) against the oracle's dup_metrics, pile-ups from tests/optical_names.py, and the `mx_*` launches that show the
exit was the one meant."""
import numpy as np
import pytest

import oracle as orc
from elprep_amd import sfm
from elprep_amd.engine import Engine
from tests import optical_names as on

pytestmark = pytest.mark.gpu

DIST = 100


def _tile_pile(n, uid0, with_tiles=True, rng=None):
    """a set of n listed reads over two read groups and both strands: on two tiles, x in steps of 60 (neighbours are optical
    duplicates at distance 100), or - without tiles - with names of four colon fields, which carry no tile"""
    rng = rng or np.random.default_rng(uid0)
    if with_tiles:
        names = [on.tile_name(uid0 + k, 7 if k % 2 else 5, b"%d" % (1101 + k % 2), b"%d" % (1000 + 60 * (k // 2)), b"2000") for k in range(n)]
    else:
        names = [on.tile_name(uid0 + k, 4, b"1101", b"%d" % (1000 + k), b"2000") for k in range(n)]
    return on.Pile(names, rng.random(n) < 0.6, rng.integers(0, 2, n))


def _every_phase():
    """a set of 33 listed reads with tiles (the cooperative kernels find candidates) and sets of 2, 3 and 4"""
    return [_tile_pile(33, 0), _tile_pile(2, 100), _tile_pile(3, 200), _tile_pile(4, 300)], ()


def _large_without_candidates():
    """a set of 33 whose names have four colon fields: members of a large set, none that can have an optical partner"""
    return [_tile_pile(33, 1000, with_tiles=False), _tile_pile(2, 1100)], ()


def _small_sets_only():
    """sets of 2 to 32: registers (2, 3), the one-thread union-find (4 .. 32), nothing for the cooperative kernels"""
    return [_tile_pile(n, 2000 + 100 * n) for n in (2, 3, 4, 32)], ()


def _no_duplicates():
    """paired reads, every pair alone on its key: no losing pair; the origins are the only histogram content"""
    return [], [(on.tile_name(3000 + k, 7, b"1101", b"%d" % k, b"7"), k % 2) for k in range(40)]


# (case, read set, launches that must be there, launches that must not)
CASES = [
    ("every_phase", _every_phase, ("mx_counters", "mx_opt_heads", "mx_opt_eval", "mx_large_list", "large_union", "mx_large_final", "mx_origin_count"), ()),
    ("large_without_candidates", _large_without_candidates, ("mx_opt_eval", "mx_large_list", "mx_large_final"), ("large_union", "large_roots")),
    ("small_sets_only", _small_sets_only, ("mx_opt_slots", "mx_opt_fill", "mx_opt_eval", "mx_origin_count"), ("mx_large_list", "mx_large_final")),
    ("no_duplicates", _no_duplicates, ("mx_counters", "mx_origin_count"), ("mx_opt_heads", "mx_opt_eval")),
    ("no_records", None, (), ("mx_",)),
]


@pytest.fixture(scope="module")
def expected():
    """the oracle's counters and histograms of every case, computed once"""
    h = on.header(2)
    out = {}
    for name, make, _, _ in CASES:
        b = on.batch(*make()) if make else sfm.empty_batch()
        _, ctr, hist = orc.dup_metrics(b, h, None, DIST, hist_len=8)
        out[name] = (b, ctr, hist)
    return out


def _launches(e, hist_len):
    e.profile_enable(True)
    e.profile_reset()
    got = e.dup_metrics(DIST, hist_len=hist_len)
    e.sync()
    ran = {k: v[0] for k, v in e.profile().items() if v[0] and "mx_" in k}
    e.profile_enable(False)
    return got, ran


def _run_case(e, case, expected):
    name, _, present, absent = case
    b, octr, ohist = expected[name]
    if b.n:
        e.stage(b)
    e.mark_duplicates(True)
    (ctr, hist), ran = _launches(e, 8)
    print(name, sorted(ran.items()))
    assert np.array_equal(ctr, octr), name
    assert np.array_equal(hist, ohist), name
    for k in present:
        assert any(k in r for r in ran), (name, k, ran)
    for k in absent:
        assert not any(k in r for r in ran), (name, k, ran)
    ctr, ran = _launches(e, 0)  # without histograms: the same counters, and no count of the origins
    assert np.array_equal(ctr, octr), name
    assert not any("mx_origin_count" in r for r in ran), (name, ran)


def test_expected_shapes(expected):
    """The read sets are what the cases say: optical duplicates in the first and third, a large set in the first two, none in the third,
    no duplicate at all in the fourth (40 origins in bin 1 of the first two histograms), nothing in the last; a few hundred records."""
    opt = {name: int(expected[name][1][0, 6]) for name, *_ in CASES}
    assert opt["every_phase"] > 0 and opt["small_sets_only"] > 0 and opt["no_duplicates"] == 0
    assert expected["every_phase"][2][0, 0, 7] == 1 and expected["large_without_candidates"][2][0, 0, 7] == 1  # the set of 33: last bin
    assert expected["small_sets_only"][2][0, 0].tolist() == [0, 0, 1, 1, 1, 0, 0, 1]  # 2, 3, 4 and 32
    assert expected["no_duplicates"][2][0, 0].tolist() == [0, 40, 0, 0, 0, 0, 0, 0] and expected["no_duplicates"][2][0, 2].sum() == 0
    assert expected["no_records"][1].sum() == 0 and expected["no_records"][2].sum() == 0
    assert sum(expected[name][0].n for name, *_ in CASES) < 1000


def test_phases_on_one_context(expected):
    """All five on one context, the largest first: a later call's smaller layout lies inside the scratch the earlier ones left."""
    e = Engine(on.header(2))
    try:
        for case in CASES:
            e.reset()
            _run_case(e, case, expected)
    finally:
        e.close()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_phases_on_a_fresh_context(case, expected):
    e = Engine(on.header(2))
    try:
        _run_case(e, case, expected)
    finally:
        e.close()
