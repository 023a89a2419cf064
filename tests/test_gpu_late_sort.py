"""A coordinate sort that comes AFTER elp_bqsr_apply (-m gpu; serial, one thread): the apply spoils the scores, not the keys, so the sort
does not enter the adapt stage - which is what lets a host run it on a thread of its own beside gather -> finalize -> apply
(include/elprep_hip.h).  The scores are recomputed on demand, from the rewritten qualities."""
import dataclasses

import numpy as np
import pytest

import oracle as orc
from elprep_amd.engine import BqsrTables, Engine
from tests.common import dataset

pytestmark = pytest.mark.gpu

ADAPT_LAUNCHES = ("adapt_fixed", "adapt_score", "adapt_score_flat")


def test_sort_behind_apply_does_not_rerun_the_adapt_stage():
    cfg, b, h, refs, sites = dataset("tiny", 4000, 1, 0.05)
    oflags = orc.mark_duplicates(b, h)
    operm = orc.sort_coordinate(b, oflags)
    oq, oc, ox = orc.bqsr_gather(b, h, orc.BqsrRef(refs, sites), oflags, 500)
    oqual = orc.BqsrFinal(oq, oc, ox, 500).apply(b, h, 0)
    e = Engine(h)
    try:
        e.stage(b)
        for r in range(h.n_ref):
            e.set_reference(r, refs[r])
            e.set_known_sites(r, sites[r])
        e.profile_enable(True)
        flags = e.mark_duplicates(True)
        qt, ct, xt = e.recalibrate(500)
        lut, present = BqsrTables(qt, ct, xt, 500).finalize().build_lut(0)
        qual = e.apply_bqsr(lut, present, 500)
        assert np.array_equal(flags, oflags) and np.array_equal(qual, oqual)
        assert (qual != b.qual).mean() > 0.5
        e.profile_reset()
        perm = e.sort_coordinate()
        e.sync()
        ran = {k: v[0] for k, v in e.profile().items() if v[0]}
        e.profile_enable(False)
        print("launches booked during the sort: %s" % sorted(ran.items()))
        assert np.array_equal(perm, operm)
        assert ran, "the profile booked nothing during the sort"
        assert not [k for k in ADAPT_LAUNCHES if k in ran], "the sort re-ran the adapt stage: %s" % sorted(ran)
        # the scores were spoiled by the apply and are recomputed on demand: the oracle's for the REWRITTEN qualities
        _, oupos, oscore = orc.mark_duplicates(dataclasses.replace(b, qual=oqual), h, with_adapted=True)
        up, sc = e.adapted()
        assert np.array_equal(up, oupos) and np.array_equal(sc, oscore)
        assert not np.array_equal(oscore, orc.mark_duplicates(b, h, with_adapted=True)[2])
    finally:
        e.close()
