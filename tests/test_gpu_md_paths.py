"""Every host path of mark duplicates (markdup_impl; csrc/markdup_plan.hpp decides) on the smallest read set that takes it
(tests/md_paths.py): the duplicate flags bit for bit against the oracle - compared as the seam tests compare them - and, from the
profile's launch counts, the kernels that must and must not have run, which proves that the path was the one meant.

The mate table's overflow retry (more Bloom-filter hits than the first table was sized for) needs an input derived from the key hash:
tests/test_gpu_md_bloom.py."""
import numpy as np
import pytest

from elprep_amd.engine import Engine
from tests import md_paths as mp

pytestmark = pytest.mark.gpu

RADIX = "md_pair_radix_"  # the pair list's radix passes (booked under the phase's prefix)

# read set, tuning, kernels that must not run, kernels that must ("md_pair_radix_": any kernel of a radix pass)
PATHS = {
    "fast": ("fast", {}, ("md_mate_pairs", "md_bloom_coarse", "md_pair_list"), ()),
    "below_the_cut": ("below_the_cut", {}, (), ("md_mate_pairs",)),
    "listed": ("listed", {}, (), ("md_mate_table", "md_bloom_coarse")),
    "full_table": ("listed", {"mate_path": 2}, ("md_mate_table",), ()),
    "big_group": ("big_group", {}, (), ("md_big_collect",)),
    "ndig_0": ("one_bucket", {"mate_path": 2}, (RADIX,), ("md_pair_bounds",)),
    "ndig_1": ("two_buckets", {"mate_path": 2}, ("md_pair_bounds",), (RADIX,)),
}


def _launched(e):
    e.sync()
    return {k: v[0] for k, v in e.profile().items() if v[0]}


def _count(ran, name):
    return sum(v for k, v in ran.items() if k.startswith(name)) if name.endswith("_") else ran.get(name, 0)


@pytest.mark.parametrize("path", list(PATHS))
def test_md_path(path):
    which, tuning, absent, present = PATHS[path]
    rs = mp.read_set(which)
    oflags, octr = rs.expected[0], rs.expected[5]
    e = Engine(mp.header(), tuning=dict(tuning))
    try:
        e.stage(rs.b)
        e.profile_enable(True)
        e.profile_reset()
        flags = e.mark_duplicates(True)
        ran = _launched(e)
        e.profile_enable(False)
        print(path, sorted(ran.items()))
        assert np.array_equal(flags, oflags), (path, np.nonzero(flags != oflags)[0][:16].tolist())
        assert np.array_equal(e.dup_metrics(100), octr), path
        assert ran.get("md_front", 0) == 1 and ran.get("md_pair_bucket", 0) == 1, (path, ran)
        for name in absent:
            assert _count(ran, name) == 0, (path, name, ran)
        for name in present:
            assert _count(ran, name) >= 1, (path, name, ran)
    finally:
        e.close()
