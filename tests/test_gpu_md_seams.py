"""Mark duplicates' front pass (k_md_front) at every lane and workgroup seam: the read sets of tests/md_seams.py - every record of a motif
at every phase of the 312-record workgroup, pairs at both parities, same-name runs of three and four, near-joins, every mask regime of
the name comparison - through the device, bit for bit against the oracle: duplicate flags, unclipped positions and scores, the
coordinate sort's permutation (in front of and behind the duplicate bits) and the metrics' counters.

Every read set runs under the library's own choice of the mate path and under mate_path = 2 (every candidate through the table), with
mark duplicates first (k_md_front<true> writes the sort keys and the unclipped positions) and behind adapted() + sort_coordinate()
(k_md_front<false>), staged in one call and in three.  (The md_fused key is retired - the passes it selected are gone and any value
but 0 is refused, test_set_tuning_rejects_unknown_keys_and_bad_values - so there is no third tuning.)

What can go wrong here: the kernel's classification is safe towards the table.  A neighbour test that fails where it should hold sends
both records to the table, which pairs them all the same; a record wrongly made leader or follower next to a longer run has a
table-bound neighbour of its key, whose Bloom announcement sends it to the table too (the filter has no false negatives); a hole that
is missing in a run of three is rewritten by k_mate_pairs, which every run of three calls.  Wrong flags come from a neighbour test that
HOLDS where it should not (two strangers become a pair: the interleaved near-joins are there for that - in the block form X0 X1 X0' X1'
the whole run joins and goes to the table) and from two writers of one slot (the plain motif at both parities)."""
import numpy as np
import pytest

from elprep_amd.engine import Engine
from tests import md_seams as ms

pytestmark = pytest.mark.gpu

TUNINGS = ({}, {"mate_path": 2})
ORDERS = ("markdup_first", "adapt_sort_first")
CHUNKS = (1, 3)


def _run(rs, what):
    """one read set under every tuning, call order and staging -> number of device runs"""
    b, h = rs.b, ms.header()
    oflags, oupos, oscore, operm0, operm, octr = rs.expected
    runs = 0
    for tuning in TUNINGS:
        for order in ORDERS:
            for chunks in CHUNKS:
                if chunks > b.n:
                    continue
                where = (what, tuning, order, chunks)
                e = Engine(h, tuning=dict(tuning))
                cuts = np.linspace(0, b.n, chunks + 1).astype(int)
                for lo, hi in zip(cuts[:-1], cuts[1:]):
                    e.stage(b if chunks == 1 else b.take(np.arange(lo, hi)))
                assert e.n == b.n
                if order == "adapt_sort_first":
                    up, sc = e.adapted()
                    assert np.array_equal(up, oupos) and np.array_equal(sc, oscore), where
                    assert np.array_equal(e.sort_coordinate(), operm0), where
                flags = e.mark_duplicates(True)
                assert np.array_equal(flags, oflags), (where, np.nonzero(flags != oflags)[0][:16].tolist())
                up, sc = e.adapted()
                assert np.array_equal(up, oupos) and np.array_equal(sc, oscore), where
                assert np.array_equal(e.sort_coordinate(), operm), where  # the sort sees the duplicate bits (sam/sam-types.go:447-452)
                assert np.array_equal(e.dup_metrics(100), octr), where
                e.close()
                runs += 1
    return runs


@pytest.mark.parametrize("motif", list(ms.MOTIFS))
def test_md_front_seams_motif(motif):
    for L in ms.LENGTHS:
        assert _run(ms.read_set(motif, L), (motif, L)) == 8


@pytest.mark.parametrize("L", ms.SHORT_LENGTHS)
def test_md_front_seams_names_of_one_and_two_bytes(L):
    for s in ms.SHORT_SLIDES:
        assert _run(ms.short_set(L, s), ("short", L, s)) == 8


def test_md_front_seams_prefixes():
    """the last workgroup with one, two and three records, the last record without a right neighbour, a pair cut by the end"""
    for n in ms.PREFIX_NS:
        assert _run(ms.prefix_set(n), ("prefix", n)) == (8 if n >= 3 else 4)
