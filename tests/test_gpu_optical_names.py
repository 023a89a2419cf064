"""GPU tests (-m gpu): the optical-duplicate count on QNAMEs at the edges of Go's parser and int arithmetic, against the oracle
(which tests/test_optical_names_cpu.py pins to a restatement of strconv.ParseInt and absInt).  Duplicate pile-ups with names under
the test's control (tests/optical_names.py): set sizes on both evaluation paths (one thread up to OPT_SMALL = 32 listed reads, the
cooperative union-find beyond), names of 5 and 7 fields and of counts without tile info, lengths on both sides of the 48-byte fast
path, fields with signs, leading zeros, 19 digits and the int64 ends, coordinates whose difference overflows int64; and where the
reference panics: a bad field in a strand list of 2 to 300000 entries (filters/mark-optical-duplicates.go:327-368) and nowhere else."""
import numpy as np
import pytest

import oracle as orc
from elprep_amd.engine import Engine, ElpError
from tests import optical_names as on

pytestmark = pytest.mark.gpu

DISTS = [0, 1, 100, 2500, (1 << 31) - 1, -5]
SIZES = [2, 3, 4, 32, 33]
# (columns, length): 0 = as short as the fields make it; 8 = ':c:t:x:y' (five fields in eight bytes)
SHAPES = [(7, 0), (5, 0), (4, 0), (6, 0), (8, 0), (5, 8), (7, 47), (7, 48), (5, 49), (7, 56), (5, 64), (7, 200)]
SHORT = [0, 1, 7, 1101, 99999, -1, -99999, 123456789, -123456789]  # values that keep a name under 48 bytes


class _Uid:
    def __init__(self):
        self.k = 0
        self.short = iter([b":%c:%d:%d:%d" % (c, t, x, y) for c in b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ" for t in (1, 2)
                           for x in range(10) for y in range(10)])

    def __call__(self):
        self.k += 1
        return self.k


def _offsets(dist, rng):
    d = abs(dist)
    pool = [0, d, -d, d + 1, -d - 1, 1 << 63, int(rng.integers(-3 * d - 3, 3 * d + 4))]
    return pool[int(rng.integers(0, len(pool)))]


def _edge_pile(n, shape, dist, rng, uid):
    ncol, length = shape
    fwd = rng.random(n) < 0.6
    rg = rng.integers(0, 2, n)
    names = []
    if length == 8:
        for _ in range(n):
            nm = next(uid.short)
            names.append(nm)
        return on.Pile(names, fwd, rg)
    vals = SHORT if 0 < length < 50 else on.EDGE_VALUES
    t0 = [1101, 0, on.I64_MAX, on.I64_MIN, -1][int(rng.integers(0, 5))] if length == 0 or length > 50 else 1101
    x0, y0 = vals[int(rng.integers(0, len(vals)))], vals[int(rng.integers(0, len(vals)))]
    for _ in range(n):
        t = t0 if rng.random() < 0.85 else t0 + 1
        if 0 < length < 50:  # plain or lightly padded spellings, so that the name fits the length
            x = x0 + int(rng.integers(-min(abs(dist), 999) - 1, min(abs(dist), 999) + 2))
            y = y0 + int(rng.integers(-2, 3))
            sp = lambda v: (b"%d" % v) if rng.random() < 0.7 else on.spell(v, rng, len(b"%d" % v) + 3)
            names.append(on.tile_name(uid(), ncol, b"%d" % t, sp(x), sp(y), length))
        else:
            x, y = on.wrap64(x0 + _offsets(dist, rng)), on.wrap64(y0 + _offsets(dist, rng))
            names.append(on.tile_name(uid(), ncol, on.spell(on.wrap64(t), rng), on.spell(x, rng), on.spell(y, rng), length))
    return on.Pile(names, fwd, rg)


def _compare(e, b, h, dist, hist_len=8):
    """flags, counters and histograms of the device against the oracle's; returns the oracle's counters"""
    oflags, octr, ohist = orc.dup_metrics(b, h, None, dist, hist_len=hist_len)
    flags = e.mark_duplicates(True)
    assert np.array_equal(flags, oflags)
    ctr, hist = e.dup_metrics(dist, hist_len=hist_len)
    assert np.array_equal(ctr, octr)
    assert np.array_equal(hist, ohist)
    assert np.array_equal(e.dup_metrics(dist), octr)
    return octr, ohist


def _edge_piles(dist, seed):
    rng = np.random.default_rng(seed)
    uid = _Uid()
    piles = [_edge_pile(n, shape, dist, rng, uid) for shape in SHAPES for n in SIZES]
    # the last record of the QNAME pool: a name of 200 bytes with its tile fields at the end
    piles.append(_edge_pile(5, (7, 200), dist, rng, uid))
    return piles


@pytest.mark.parametrize("dist", DISTS)
def test_edge_names_against_the_oracle(dist):
    """Sixty duplicate sets of 2, 3, 4, 32 and 33 listed reads over two read groups and both strands, every name shape, fields
    spelled with signs and leading zeros (up to 26 characters), values from 0 to the int64 ends, coordinates at +-dist, dist + 1
    and 2^63 from the set's base; counters and histograms against the oracle, and the oracle against the restatement.  On the parent
    commit the device refused the whole read set (ELP_ERR_DATA: fields of 19 digits and more, leading zeros past 18 characters)."""
    piles = _edge_piles(dist, 100 + dist % 977)
    lens = {len(nm) for p in piles for nm in p.names}
    assert {8, 47, 48, 49, 56, 64, 200} <= lens
    b = on.batch(piles)
    assert len(piles[-1].names[-1]) == 200 and int(b.qname_off[-1]) == b.qname.size
    h = on.header(2)
    opt, hist, panics = on.expected_metrics(piles, dist, 8)
    assert not panics
    e = Engine(h)
    e.stage(b)
    octr, ohist = _compare(e, b, h, dist)
    e.close()
    assert octr[0, 6] == opt and np.array_equal(ohist[0, :, 2:], hist[:, 2:])
    if dist >= 0:
        assert opt > 20


@pytest.mark.parametrize("dist", [100, (1 << 31) - 1])
def test_a_few_thousand_members_at_the_int64_ends(dist):
    """Two sets of 2500 listed reads (the cooperative kernels) on three tiles at the int64 ends, coordinates within a few dist of
    each other across the wrap-around, names padded with leading zeros; against the oracle."""
    rng = np.random.default_rng(dist % 1000)
    piles = []
    for s, (x0, y0) in enumerate(((on.I64_MAX, on.I64_MIN), (on.I64_MIN + 2, 0))):
        n = 2500
        names = []
        for k in range(n):
            t = [on.I64_MAX, on.I64_MIN, 7][int(rng.integers(0, 3))]
            x = on.wrap64(x0 + int(rng.integers(-3 * dist, 3 * dist)))
            y = on.wrap64(y0 + int(rng.integers(-3 * dist, 3 * dist)))
            names.append(on.tile_name(10_000 * s + k, 7 if k % 3 else 5, on.spell(t, rng), on.spell(x, rng), on.spell(y, rng)))
        piles.append(on.Pile(names, rng.random(n) < 0.5, rng.integers(0, 2, n)))
    b = on.batch(piles)
    h = on.header(2)
    e = Engine(h)
    e.stage(b)
    octr, _ = _compare(e, b, h, dist, hist_len=4096)
    e.close()
    assert octr[0, 6] > 500


BAD = {"syntax": b"12x", "range": b"9223372036854775808", "empty": b"", "negrange": b"-9223372036854775809"}


def _bad_pile(n, bad, uid0, at=1, fwd=None, rg=None):
    names = [on.tile_name(uid0 + k, 7, b"1101", b"%d" % (1000 + 10 * (k % 50)), b"%d" % (2000 + k // 50)) for k in range(n)]
    names[at] = on.tile_name(uid0 + at, 7, b"1101", b"1000", bad)
    return on.Pile(names, [True] * n if fwd is None else fwd, [0] * n if rg is None else rg)


@pytest.mark.parametrize("kind", sorted(BAD))
@pytest.mark.parametrize("n", [2, 3, 4, 32, 33, 3000])
def test_bad_field_in_a_parsed_list_raises(kind, n):
    """A field the reference cannot parse, on a member of a strand list of 2..300000 entries: the reference panics, the oracle and
    the device raise; the same context then runs a clean read set (every output equal to the oracle's).  On the parent commit the
    raise passed (the range cases only through its 18-digit limit) and the clean read set of edge names failed with ELP_ERR_DATA."""
    h = on.header(2)
    b = on.batch([_bad_pile(n, BAD[kind], 0, at=n - 1)])
    with pytest.raises(RuntimeError, match="reference would panic"):
        orc.dup_metrics(b, h, None, 100)
    e = Engine(h)
    e.stage(b)
    e.mark_duplicates(True)
    with pytest.raises(ElpError, match="QNAME"):
        e.dup_metrics(100)
    with pytest.raises(ElpError, match="QNAME"):
        e.dup_metrics(100, hist_len=8)
    e.reset()
    clean = on.batch(_edge_piles(100, 5))
    e.stage(clean)
    _compare(e, clean, h, 100)
    e.close()


@pytest.mark.parametrize("kind", sorted(BAD))
def test_bad_field_where_the_reference_parses_nothing(kind):
    """The same bad names where computeTileInfo never runs: alone on their strand list (sets of 2, 3, 5, 33 and 40 whose other
    members are listed on the other strand) and on pairs in no duplicate set.  The reference does not panic; nothing raises and
    every output equals the oracle's.  Failed on the parent commit: the device parsed every member of every set, and failed the call."""
    h = on.header(2)
    piles = []
    for s, n in enumerate((2, 3, 5, 33, 40)):
        fwd = [False] * n
        fwd[s % n] = True
        piles.append(_bad_pile(n, BAD[kind], 1000 * s, at=s % n, fwd=fwd, rg=[k % 2 for k in range(n)]))
    singles = [(on.tile_name(90_000, 7, b"1", BAD[kind], b"1"), 1), (on.tile_name(90_001, 5, BAD[kind], b"x", b""), 0)]
    b = on.batch(piles, singles)
    opt, _, panics = on.expected_metrics(piles, 100, 8)
    assert not panics and opt > 0
    e = Engine(h)
    e.stage(b)
    octr, _ = _compare(e, b, h, 100)
    e.close()
    assert octr[0, 6] == opt


def test_bad_field_in_the_capped_list():
    """The shape of test_large_duplicate_sets_and_the_list_cap: 300040 pairs listed forward (more than 300000: the reference keeps
    300001, parses none and counts 0) with a bad name among them, and 700 valid ones listed reverse.  No panic; every output equal to
    the oracle's.  Failed on the parent commit (the device parsed the capped list's names and failed the call)."""
    rng = np.random.default_rng(300_040)
    n_fwd, n_rev = 300_040, 700
    n = n_fwd + n_rev
    fwd = np.zeros(n, bool)
    fwd[:n_fwd] = True
    rng.shuffle(fwd)
    fwd[0] = True
    tile, x, y = rng.integers(1101, 1109, n), rng.integers(1000, 3000, n), rng.integers(1000, 3000, n)
    names = [b"P%d:1:FC:1:%d:%d:%d" % (k, tile[k], x[k], y[k]) for k in range(n)]
    at = int(np.nonzero(fwd)[0][1000])
    names[at] = b"P%d:1:FC:1:%d:%d:9223372036854775808" % (at, tile[at], x[at])
    b = on.batch([on.Pile(names, fwd, rng.integers(0, 2, n))])
    h = on.header(2)
    e = Engine(h)
    e.stage(b)
    octr, ohist = _compare(e, b, h, 100)
    e.close()
    assert octr[0, 6] > 100 and ohist[0, 0, 7] == 1


def test_names_from_the_bam_decoder():
    """The edge names staged as BAM (orc.bam_encode -> elp_stage_bam): the QNAME pool the decoder writes; then a bad name in a
    parsed list raises from a BAM-staged read set too."""
    h = on.header(2)
    piles = _edge_piles(100, 77)
    b = on.batch(piles)
    e = Engine(h)
    e.set_read_group_ids(h.rg_ids)
    e.stage_bam(orc.bam_encode(b, h.rg_ids))
    _compare(e, b, h, 100)
    e.reset()
    bad = on.batch([_bad_pile(4, BAD["range"], 0, at=2)])
    e.stage_bam(orc.bam_encode(bad, h.rg_ids))
    e.mark_duplicates(True)
    with pytest.raises(ElpError, match="QNAME"):
        e.dup_metrics(100)
    e.close()


def test_sfm_rank_carries_the_error_across_the_side_lane():
    """SfmRank.gather runs mark duplicates and then the metrics pass of each split on the context's side lane: a bad name in a parsed
    list raises ElpError out of gather (before the BQSR pass); valid edge names give the oracle's counters through the rank's context."""
    from elprep_amd import sfm
    h = on.header(2)
    bad = on.batch([_bad_pile(3, BAD["syntax"], 0, at=0)])
    rk = sfm.SfmRank(h, 0, sfm.Comm())
    try:
        rk.stage(0, bad)
        with pytest.raises(ElpError, match="QNAME"):
            rk.gather(500, 100)
    finally:
        rk.close()
    good = on.batch(_edge_piles(2500, 9))
    rk = sfm.SfmRank(h, 0, sfm.Comm())
    try:
        rk.stage(0, good)
        _compare(rk.engines[0], good, h, 2500)
    finally:
        rk.close()
