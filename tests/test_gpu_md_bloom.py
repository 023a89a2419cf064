"""Mark duplicates' mate-table overflow retry (md_mates, csrc/markdup.hip) and the Bloom filter's word, bit, line and coarse-word
indexing, on read sets derived from the key hash (tests/md_bloom.py): the duplicate flags and the metrics' counters bit for bit against
the oracle, and, from the profile's launch counts, the kernels that ran.

The retry.  In aligner order the first mate table has Tm slots, sized by an estimate.  The sets `over*` send Tm + 1 names to it: they cannot
fit, whatever the interleaving, so k_mate_table sets bit 2 of err[1] and the host clears it, refills mate, rep_of, the table, the pair
counter and the lists' counters and runs k_mate_pairs and k_mate_table again with all T slots - two launches of each, where `full` (Tm
names: the table ends exactly full) has one.  The count of two is also the proof that the replica in tests/md_bloom.py is the device's
hash: it happens only if all Tm + 1 names, the searched ones included, really reached the table.

What a retry that forgets a refill looks like (each tried once on a scratch build, on over_big; for `over` read off the code):
  the err[1] clear   bit 2 outlives the second pass and the call ends with "mate table overflow" (over_big failed so; the host code
                     is the same for every `over*` set);
  the mate fill      a representative that was paired in the first pass is not EMPTY, so every claim fails and every table pair
                     becomes a "big group", which md_big_groups pairs up again in arrival order - the same pairs, the same flags
                     (over_big passed).  It shows only in md_big_collect, which must not run where no key has three records: the
                     count asserted below for `over`, `over_split` and `over_2048`;
  the rep_of fill    nothing fails, and nothing can: rep_of is read by md_big_collect alone, every record that claims writes its own
                     entry again, a key with three records has three in both passes and gets MATE_BIG again, and a representative's stale
                     entry points at a record of its own key whose entry is a record index, not MATE_BIG.  The fill is belt and braces.

The same sets fill list 0 of the deferred inserts to tab_cap exactly (workgroup 0 is all table-bound; in over_2048 workgroups 0 and 64 share
the list, tab_cap = 512) and hold more list members than the host's list_n, so k_mate_table and k_pair_list_lists go round twice.

The seam sets hold one announcement each, t2's, at the first or last bit of a word, a 64-byte line, a coarse word or the filter, and the
neighbours t0 t1 of that name behind it.  A filter false negative pairs (t0, t1), a duplicate of pair a; the oracle pairs (t2, t0).  That
t0 and t1 went to the table shows in md_big_collect: three records of one key.

Not reached, and not to be reached: the final "mate table overflow" error (Tm == T).  T holds all n records at half load."""
import numpy as np
import pytest

from elprep_amd.engine import Engine
from tests import md_bloom as mb
from tests import md_paths as mp

pytestmark = pytest.mark.gpu

ORDERS = ("markdup_first", "adapt_sort_first")
RETRY = dict(md_mate_pairs=2, md_mate_table=2, md_bloom_coarse=1, md_front=1, md_pair_bucket=1)


def _mark(e, rs, what, order="markdup_first", behind=False):
    """stage, mark duplicates under the profile, compare flags and counters (behind: adapted() and the sort as well) -> launch counts"""
    oflags, oupos, oscore, operm0, operm, octr = rs.expected
    e.stage(rs.b)
    assert e.n == rs.b.n
    if order == "adapt_sort_first":
        up, sc = e.adapted()
        assert np.array_equal(up, oupos) and np.array_equal(sc, oscore), what
        assert np.array_equal(e.sort_coordinate(), operm0), what
    e.profile_enable(True)
    e.profile_reset()
    flags = e.mark_duplicates(True)
    e.sync()
    ran = {k: v[0] for k, v in e.profile().items() if v[0]}
    e.profile_enable(False)
    print(what, order, sorted(ran.items()))
    assert np.array_equal(flags, oflags), (what, order, np.nonzero(flags != oflags)[0][:16].tolist())
    assert np.array_equal(e.dup_metrics(100), octr), (what, order)
    if behind or order == "adapt_sort_first":
        up, sc = e.adapted()
        assert np.array_equal(up, oupos) and np.array_equal(sc, oscore), (what, order)
        assert np.array_equal(e.sort_coordinate(), operm), (what, order)
    return ran


def _run(rs, what, tuning=None, **kw):
    e = Engine(mb.header(), tuning=dict(tuning or {}))
    try:
        return _mark(e, rs, what, **kw)
    finally:
        e.close()


def _counts(ran, want):
    return {k: ran.get(k, 0) for k in want}


def test_full_table_is_no_retry():
    """Tm names in Tm slots: every probe sequence ends at a free slot at the latest after Tm probes"""
    ran = _run(mb.read_set("full"), "full")
    assert _counts(ran, RETRY) == dict(RETRY, md_mate_pairs=1, md_mate_table=1), ran


@pytest.mark.parametrize("name", mb.SETS[1:])
def test_overflow_retry(name):
    ran = _run(mb.read_set(name), name, behind=name == "over")
    assert _counts(ran, RETRY) == RETRY, (name, ran)
    assert ran.get("md_big_collect", 0) == (1 if name == "over_big" else 0), (name, ran)


def test_over_through_the_full_table():
    """mate_path = 2: all T slots at once - one pass, no list, the same flags"""
    ran = _run(mb.read_set("over"), "over, mate_path 2", tuning={"mate_path": 2})
    assert ran.get("md_mate_pairs", 0) == 1 and ran.get("md_mate_table", 0) == 0 and ran.get("md_bloom_coarse", 0) == 1, ran


def test_over_behind_adapt_and_sort():
    """(mark duplicates first: test_overflow_retry)"""
    ran = _run(mb.read_set("over"), "over", order="adapt_sort_first")
    assert _counts(ran, RETRY) == RETRY, ran


@pytest.mark.parametrize("bw,target", mb.SEAMS)
def test_filter_seam(bw, target):
    rs = mb.seam_set(bw, target)
    for order in ORDERS:
        ran = _run(rs, ("seam", bw, target), order=order)
        want = dict(md_mate_pairs=1, md_mate_table=1, md_bloom_coarse=1, md_front=1, md_big_collect=1)
        assert _counts(ran, want) == want, (bw, target, order, ran)


@pytest.mark.parametrize("first", ("over", "listed"))
def test_one_context_both_ways(first):
    """A retry, reset(), a call without one - and the reverse - on one context: scratch slots are grow-only (the second call of the
    reverse order regrows the table under a context that has run) and the counters and the error word are per call."""
    sets = {"over": (mb.read_set("over"), RETRY), "listed": (mp.read_set("listed"), dict(RETRY, md_mate_pairs=1, md_mate_table=1))}
    e = Engine(mb.header())
    try:
        for k, which in enumerate((first, "listed" if first == "over" else "over")):
            if k:
                e.reset()
            rs, want = sets[which]
            ran = _mark(e, rs, (first, which))
            assert _counts(ran, want) == want, (first, which, ran)
    finally:
        e.close()
