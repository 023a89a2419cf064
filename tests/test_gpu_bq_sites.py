"""BQSR known sites on the device at every seam of flags, buckets and skip bits: the read sets of tests/bq_sites.py - a site for every phase of
the packed reference's 8-base words, at every 64-base bucket seam, at every bit phase of the skip column's 32-bit words, around the
thresholds that choose between the reference window and the column, on every CIGAR shape of the three prologues - through the gather,
the three tables bit for bit against the oracle.

Every read set runs with descriptors (count_kernel = 1) and with records (2, 3, and 0 = the library's choice, which must be the one-length
kernel for a one-length set), staged in one call and in three, on a fresh context and on a reused one (tests/conftest.py).  The device's
error word must stay 0 - bit 1024 says that rec_simple and make_rec disagree - : a set bit makes the gather raise.  Then the site lists
change under a staged read set (bits a read had must go), and the reference and the sites are set in either order.

A cell that differs is decoded to (family, probe class, base index) in the failure message."""
import numpy as np
import pytest

from elprep_amd.engine import Engine
from tests import bq_sites as bs

pytestmark = pytest.mark.gpu

KERNELS = (1, 2, 3, 0)
CHUNKS = (1, 3)


def _context(case, tuning, chunks=1):
    e = Engine(case.h, tuning=dict(tuning))
    cuts = np.linspace(0, case.b.n, chunks + 1).astype(int)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        e.stage(case.b if chunks == 1 else case.b.take(np.arange(lo, hi)))
    assert e.n == case.b.n
    return e


def _set(e, case, which, reference=True, sites_first=False):
    for r in range(case.h.n_ref):
        if sites_first:
            e.set_known_sites(r, case.sites_of(which)[r])
        if reference:
            e.set_reference(r, case.refs[r])
        if not sites_first:
            e.set_known_sites(r, case.sites_of(which)[r])


def _same(case, got, which, where):
    for k, what in ((1, "cycle"), (2, "context"), (0, "quality")):  # (the cycle table first: its cells name the base)
        g, w = got[k], case.expected(which)[k]
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)
            cov, q, x = (int(v) for v in bad[0][:3])
            whose = case.decode(cov, q, x) if what == "cycle" else "case %s, family %s, probes = %d mod %d" % (case.name, case.families[cov], q - 6, case.nq)
            raise AssertionError("%s, list %s: %s table: %d cells differ, first %s: %d, expected %d - %s" % (
                where, which, what, len(bad), tuple(bad[0]), g[tuple(bad[0])], w[tuple(bad[0])], whose))


def _gather(e, case, records=None):
    """the tables of the staged reads; records: True / False = the record form (the one-length kernel) must / must not have been taken.  An
    error word other than 0 raises ElpError here."""
    e.profile_enable(True)
    e.profile_reset()
    try:
        out = [np.array(t) for t in e.recalibrate(case.max_cycle)]
        ran = {k: v[0] for k, v in e.profile().items() if v[0]}
    finally:
        e.profile_enable(False)
    if records is not None:  # (the record segments' offsets are laid out only in front of the one-length kernel: rec_buffers, bqsr.hip)
        assert ("bqsr_seg_offsets" in ran) == records, (case.name, ran)
    return out


@pytest.mark.parametrize("name", list(bs.CASES))
def test_known_sites_every_form_and_staging(name):
    case = bs.CASES[name]()
    for kernel in KERNELS:
        for chunks in CHUNKS:
            e = _context(case, {"count_kernel": kernel}, chunks)
            _set(e, case, "A")
            records = False if kernel == 1 or name not in bs.RECORD_CASES else (True if kernel == 0 else None)
            _same(case, _gather(e, case, records), "A", (name, "count_kernel", kernel, "chunks", chunks))
            e.close()


STALE_CASES = ("ruler37", "ruler101", "indels40", "indels37", "indels101", "adaptor", "many_contigs")
ORDER = ("A", "B", "A", "C", "0")  # the lists in turn: B takes the sites away from the reads that had them, C moves every site by one base


@pytest.mark.parametrize("name", STALE_CASES)
@pytest.mark.parametrize("forms", [(1,), (0,), (0, 1), (1, 0)], ids=["descriptors", "records", "records_first", "descriptors_first"])
def test_site_lists_replaced_under_staged_reads(name, forms):
    """gathers on ONE context while the lists change: each equals the oracle for its list.  In the record form nobody clears the skip column
    but the reads that use it (clear_skip_bits), and the flags inside the packed reference are taken back by k_ref_clear_site_flags."""
    case = bs.CASES[name]()
    e = _context(case, {"count_kernel": forms[0]})
    _set(e, case, ORDER[0])
    for k, which in enumerate(ORDER):
        kernel = forms[k % len(forms)]
        if k:
            e.set_tuning("count_kernel", kernel)
            _set(e, case, which, reference=False)
        _same(case, _gather(e, case, kernel == 0), which, (name, "gather", k, "count_kernel", kernel))
    e.close()


@pytest.mark.parametrize("kernel", [1, 0])
@pytest.mark.parametrize("sites_first", [False, True])
def test_reference_and_sites_in_either_order(kernel, sites_first):
    """the ruler's contigs - one with an empty list, one with a site that ends past LN - with set_known_sites in front of set_reference
    and behind it; then the reference alone set again (the flags inside it must come back)"""
    case = bs.ruler(37)
    e = _context(case, {"count_kernel": kernel})
    _set(e, case, "A", sites_first=sites_first)
    _same(case, _gather(e, case, kernel == 0), "A", ("ruler37", "sites first", sites_first, "count_kernel", kernel))
    for r in range(case.h.n_ref):
        e.set_reference(r, case.refs[r])
    _same(case, _gather(e, case, kernel == 0), "A", ("ruler37", "reference set again", "count_kernel", kernel))
    e.close()
