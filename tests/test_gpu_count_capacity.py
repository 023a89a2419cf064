"""GPU tests (-m gpu) that drive the private LDS tables of the two BQSR count kernels to the capacity of their packed counters and through
their in-loop flushes.  A cycle cell is 16 | 16 bits (observations | mismatches; in the general kernel's MG form two 16-bit observation
cells of neighbouring cycles share a word), and only the flush schedule keeps one half from carrying into the other:
  k_bqsr_count   (bqsr_count.hip)   flushes at the end of the first 32768-byte index tile behind which more than 30000 reads have started since
                              the last flush: at most 30000 + 32768 = 62768 counts per cell;
  k_bqsr_count3  (count3.hip) flushes every 30000 / (RPI + 1) + 1 trips of RPI = 1024 / ceil(len / 16) reads: at most flush_every x RPI
                              (30720 for reads of up to 16 bases) per cell, and at every segment's end under the covariate split.
The reads here have ONE quality (30) and the base A (reference: all A) or C, so that every read adds to the same few cells: a threshold
that is too high, a flush that loses or keeps counts, a carry into the neighbouring half or cycle all show as a wrong table.  Every case
is compared bit for bit with the oracle AND with a closed form written here (_expected), which does not go through the oracle.

Not covered: the `bases_since_flush > 2^31` guard of the 32 | 32-bit context cells - it needs 2 G bases in one workgroup."""
import functools

import numpy as np
import pytest

import oracle as orc
from elprep_amd.batch import Batch, Header
from elprep_amd.engine import Engine

pytestmark = pytest.mark.gpu

MAXC = 160          # --max-cycle of every case (reads have at most 150 bases)
Q = 30
REF = np.full(1000, ord("A"), np.uint8)
TILE = 32768        # FL_TILE (flat.hpp)
VARIANTS = ("match", "mismatch", "half")  # no read mismatches / every read does (both halves of a cell at their maximum) / a random half


def _header(n_rg):
    return Header.from_read_groups(["c0"], [REF.size], [{"ID": "rg%d" % k, "LB": "lib", "PU": "pu%d" % k} for k in range(n_rg)])


def _mism(variant, n, seed):
    if variant == "match":
        return np.zeros(n, bool)
    if variant == "mismatch":
        return np.ones(n, bool)
    return np.random.default_rng(seed).random(n) < 0.5


def _batch(lens, mism, rgid, clip=None, quals=None):
    """unpaired forward mapped reads, read i of lens[i] bases that are all A (mism[i] false) or all C, CIGAR <len>M - or 1S<len-1>M where
    clip[i] -, quality 30 everywhere unless quals = {read index: array} says otherwise.  Built column by column: nothing is padded, so
    qual_off of the batch IS the staged layout."""
    lens = np.asarray(lens, np.int64)
    n = lens.size
    clip = np.zeros(n, bool) if clip is None else np.asarray(clip, bool) & (lens > 1)
    qual_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    qual = np.full(int(qual_off[-1]), Q, np.uint8)
    for i, q in (quals or {}).items():
        qual[int(qual_off[i]):int(qual_off[i + 1])] = q
    sb = (lens + 1) // 2
    seq_off = np.concatenate([[0], np.cumsum(sb)]).astype(np.uint64)
    seq4 = np.repeat(np.where(mism, 0x22, 0x11).astype(np.uint8), sb)  # first base in the high nibble: A = 1, C = 2
    odd = (lens & 1) == 1
    seq4[(seq_off[1:][odd] - 1).astype(np.int64)] &= 0xF0
    nops = np.where(clip, 2, 1)
    cigar_off = np.concatenate([[0], np.cumsum(nops)]).astype(np.uint64)
    cigar = np.zeros(int(cigar_off[-1]), np.uint32)
    first = cigar_off[:-1].astype(np.int64)
    cigar[first] = np.where(clip, (1 << 4) | 4, lens << 4)
    cigar[first[clip] + 1] = (lens[clip] - 1) << 4
    return Batch(refid=np.zeros(n, np.int32), pos=(1 + np.arange(n) % 500).astype(np.int32), next_refid=np.full(n, -1, np.int32), pnext=np.zeros(n, np.int32),
                 tlen=np.zeros(n, np.int32), flag=np.zeros(n, np.uint16), mapq=np.full(n, 60, np.uint8), rgid=np.asarray(rgid, np.uint16),
                 has_sr=np.zeros(n, np.uint8), l_seq=lens.astype(np.uint32), qname_off=np.arange(n + 1, dtype=np.uint64), qname=np.full(n, ord("r"), np.uint8),
                 cigar_off=cigar_off, cigar=cigar, seq_off=seq_off, seq4=seq4, qual_off=qual_off, qual=qual)


def _expected(h, b, mism, clip=None, quals=None):
    """The tables in closed form.  Base k (from 0) of a forward unpaired read is cycle k + 1 (a leading soft clip is cut off first) and
    mismatches iff it is C; from the second base on it has the context (previous base | base << 2): AA = 0, CC = 5.  So cell (cov, 30,
    cycle c) = {reads of the covariate with at least c bases, those of them that are C}; the reads listed in `quals` are added base by base."""
    lens = b.l_seq.astype(np.int64)
    eff = lens - (np.zeros(b.n, bool) if clip is None else (np.asarray(clip, bool) & (lens > 1)))
    cov = h.rg_cov[b.rgid].astype(np.int64)
    ct = np.zeros((h.n_cov, 94, 2 * MAXC + 1, 2), np.int64)
    xt = np.zeros((h.n_cov, 94, 16, 2), np.int64)
    plain = np.ones(b.n, bool)
    for i in (quals or {}):
        plain[i] = False
    lmax = int(eff.max())
    for cv in range(h.n_cov):
        for m in (0, 1):
            sel = plain & (cov == cv) & (mism == bool(m))
            ge = np.bincount(eff[sel], minlength=lmax + 2)[::-1].cumsum()[::-1]  # ge[c] = reads with at least c bases
            ct[cv, Q, MAXC + 1:MAXC + 1 + lmax, 0] += ge[1:lmax + 1]
            ct[cv, Q, MAXC + 1:MAXC + 1 + lmax, 1] += m * ge[1:lmax + 1]
            with_ctx = int(np.maximum(eff[sel] - 1, 0).sum())
            xt[cv, Q, 5 * m, 0] += with_ctx
            xt[cv, Q, 5 * m, 1] += m * with_ctx
    for i, q in (quals or {}).items():
        m = int(mism[i])
        for k, qk in enumerate(np.asarray(q)[int(lens[i] - eff[i]):]):
            assert qk >= 6
            ct[cov[i], qk, MAXC + 1 + k] += (1, m)
            if k:
                xt[cov[i], qk, 5 * m] += (1, m)
    return ct.sum(axis=2), ct, xt


def _reference(h, b, mism, clip=None, quals=None):
    """(oracle's tables, closed form) - equal, or the test's own construction is off"""
    for i in list(range(0, b.n, max(1, b.n // 50))) + [b.n - 1]:
        assert orc.recalibrate_aln(b, h, i)
    o = orc.bqsr_gather(b, h, orc.BqsrRef([REF], [np.zeros((0, 2), np.int32)]), None, MAXC)
    x = _expected(h, b, mism, clip, quals)
    for a, e, what in zip(o, x, ("quality", "cycle", "context")):
        assert np.array_equal(a, e), "oracle and closed form disagree on the %s table" % what
    return x


def _gather(h, b, tuning, launches=None, twice=False):
    """the device's tables of the batch under `tuning`.  count3_grid is NOT among the keys tests/conftest.py resets on a pooled context:
    whoever sets it must set it back to 0 before close(), or a later [reused] test inherits it - hence the finally."""
    e = Engine(h, tuning=tuning)
    try:
        e.stage(b)
        e.set_reference(0, REF)
        e.set_known_sites(0, np.zeros((0, 2), np.int32))
        e.profile_enable(True)
        e.profile_reset()
        out = [np.array(t) for t in e.recalibrate(MAXC)]
        if launches is not None:
            assert e.profile()["bqsr_count"][0] == launches
        if twice:
            again = e.recalibrate(MAXC)
            for a, t in zip(again, out):
                assert np.array_equal(a, t), "the second gather on the same context differs from the first"
    finally:
        e.profile_enable(False)
        e.set_tuning("count3_grid", 0)
        e.close()
    return out


def _same(got, want):
    for g, w, what in zip(got, want, ("quality", "cycle", "context")):
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)
            raise AssertionError("%s table: %d cells differ, first %s: %d, expected %d" % (what, len(bad), tuple(bad[0]), g[tuple(bad[0])], w[tuple(bad[0])]))


# ------------------------------------------------------------------------------------------------------------------ the general kernel
# Everything lies in ONE 256 KiB step of the flat index, so one workgroup counts it all (the grid is min(steps, ...)):
#   tile 0   r reads of one and two bases that fill exactly 32768 QUAL bytes (2 r - 32768 of one base, 32768 - r of two), shuffled
#   tile 1   32768 reads of one base
#   tile 2   500 reads of one base, 100 of two, then the FORM's long reads (150 bases, other qualities and read groups)
# r = 29999 / 30000: no flush behind tile 0, cell (30, cycle 1) holds 62767 / 62768 - the design's maximum - at the end of tile 1;
# r = 30001 / 32768: a flush behind tile 0 and one behind tile 1; 32768 = two full tiles is the one that a threshold above a tile's
# reads (or a flush at the end of the step only) overflows: 65536 counts.
# Private-table forms (count_general_plan, bqsr_plan.hpp), by (read groups, qualities of the long reads); rows of 352 words at 150 bases:
FORMS = {
    "wg512": (1, 5),    # 9 rows of 1408 B: three 512-thread workgroups per CU
    "big": (2, 20),     # 2 x 24 rows = 68 KB: more than half a CU's LDS -> one 1024-thread workgroup, 16 | 16 cells, one pass
    "mg": (4, 39),      # 4 x 42 rows: 237 KB as 16 | 16 cells -> MG, observation cells two per word (768 B rows: 129 KB), one pass
    "passes": (4, 40),  # 4 x 43 rows do not fit as MG rows either: two passes
}
SWEEP = (29999, 30000, 30001, 32768)


@functools.lru_cache(maxsize=None)
def _general_case(r, variant, form):
    n_rg, n_q = FORMS[form]
    rng = np.random.default_rng(r + n_q)
    tile0 = rng.permutation(np.concatenate([np.ones(2 * r - TILE, np.int64), np.full(TILE - r, 2, np.int64)]))
    n_long = 2 * n_rg
    lens = np.concatenate([tile0, np.ones(TILE, np.int64), np.ones(500, np.int64), np.full(100, 2, np.int64), np.full(n_long, 150, np.int64)])
    n = lens.size
    mism = _mism(variant, n, r)
    rgid = np.zeros(n, np.uint16)
    quals = {}
    for j in range(n_long):
        i = n - n_long + j
        rgid[i] = j % n_rg
        quals[i] = (6 + (np.arange(150) + 7 * j) % n_q).astype(np.uint8)  # qualities 6 .. 6 + n_q - 1, every one of them in every read
    h = _header(n_rg)
    b = _batch(lens, mism, rgid, quals=quals)
    # the layout the kernel sees, read off the batch: tile 0 and tile 1 start r and 32768 reads, nothing straddles a tile's end
    starts = b.qual_off[:-1].astype(np.int64)
    assert int(b.qual_off[-1]) <= 8 * TILE and int(b.qual_off[r]) == TILE and int(b.qual_off[r + TILE]) == 2 * TILE
    assert np.array_equal(np.bincount(starts // TILE)[:2], [r, TILE])
    return h, b, _reference(h, b, mism, quals=quals)


def _general(r, variant, form, launches):
    h, b, want = _general_case(r, variant, form)
    assert want[1][0, Q, MAXC + 1, 0] >= r + TILE
    _same(_gather(h, b, None, launches=launches), want)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("r", SWEEP)
def test_general_tile_sweep_wg512(r, variant):
    """form: 512-thread workgroups, 16 | 16 cells (the plan: 6 qualities x 1 covariate, three workgroups per CU)"""
    _general(r, variant, "wg512", 1)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("r", SWEEP)
def test_general_tile_sweep_big(r, variant):
    """form: one 1024-thread workgroup per CU, 16 | 16 cells (the plan: 21 qualities x 2 covariates - more than the 19 slots of half a CU - in one pass)"""
    _general(r, variant, "big", 1)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("r", SWEEP)
def test_general_tile_sweep_mg(r, variant):
    """form: MG - 1024 threads, observation cells two per word: cycles 1 and 2 of the one- and two-base reads share a word, a carry
    out of cycle 1 would be a wrong count at cycle 2 (the plan: 39 qualities x 4 covariates, two passes of 16 | 16 rows, one of MG rows)"""
    _general(r, variant, "mg", 1)


@pytest.mark.parametrize("r", SWEEP)
def test_general_tile_sweep_two_passes(r):
    """4 read groups x 40 qualities: two passes over quality subsets (1024 threads, 16 | 16 rows, 20 qualities each: MG rows would need
    two passes as well) while the capacity reads stay in cell (30, cycle 1): in the pass that does not count quality 30 they fill the
    row of the qualities that are not counted"""
    _general(r, "half", "passes", 2)


# --------------------------------------------------------------------------------------------------------------- the one-length kernel
# count3_grid = 1: ONE workgroup takes every trip of a launch, so ~300 K reads give it ten in-loop flushes.  Reads that are one run of
# matches go to launch 1 and its 64 class-1 segments; reads with 1S<len-1>M all go to the one "other" segment of launch 2, whose trips are
# full: its cells reach flush_every x RPI (30720 up to 16 bases, 30208 at 17, 29784 at 150 bases: 45 MB of QUAL).
LENGTHS = (1, 8, 16, 17, 150)


def _n_reads(length):
    return 300_000


@functools.lru_cache(maxsize=None)
def _one_length_case(length, clipped, variant, n_rg):
    n = _n_reads(length)
    mism = _mism(variant, n, 100 * length + n_rg)
    rgid = (np.arange(n) % n_rg).astype(np.uint16) if n_rg > 1 else np.zeros(n, np.uint16)
    clip = np.full(n, bool(clipped))
    h = _header(n_rg)
    b = _batch(np.full(n, length, np.int64), mism, rgid, clip=clip)
    return h, b, _reference(h, b, mism, clip=clip)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("clipped", (False, True), ids=("run", "clip"))
@pytest.mark.parametrize("length", LENGTHS)
def test_one_length_one_workgroup(length, clipped, variant):
    h, b, want = _one_length_case(length, clipped, variant, 1)
    _same(_gather(h, b, {"count3_grid": 1}, launches=2), want)


@pytest.mark.parametrize("clipped", (False, True), ids=("run", "clip"))
@pytest.mark.parametrize("length", LENGTHS)
def test_one_length_covariate_split(length, clipped):
    """count_kernel = 3, three read groups: the table is flushed at every covariate segment's end as well as inside the loop"""
    h, b, want = _one_length_case(length, clipped, "half", 3)
    _same(_gather(h, b, {"count3_grid": 1, "count_kernel": 3}, launches=2), want)


@pytest.mark.parametrize("grid", (2, 0))
@pytest.mark.parametrize("length", LENGTHS)
def test_one_length_grids_agree(length, grid):
    """two workgroups, and the default of one per CU: the same tables as one workgroup gives"""
    h, b, want = _one_length_case(length, True, "half", 1)
    _same(_gather(h, b, {"count3_grid": grid}, launches=2), want)


def test_one_length_gather_twice():
    """the second gather on the same context starts from cleared tables"""
    h, b, want = _one_length_case(16, True, "mismatch", 1)
    _same(_gather(h, b, {"count3_grid": 1}, launches=2, twice=True), want)


def test_count3_grid_rejects_negative_values():
    e = Engine(_header(1))
    try:
        with pytest.raises(Exception, match="count3_grid"):
            e.set_tuning("count3_grid", -1)
    finally:
        e.set_tuning("count3_grid", 0)
        e.close()
