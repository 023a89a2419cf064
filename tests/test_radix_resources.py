"""The radix scatter kernel's forms (radix.hip) compiled for gfx950 (hipcc cross-compiles without a GPU): the 1024-thread form is one
workgroup of 16 waves per CU - four waves per SIMD, which 128 vector registers allow and 129 do not (the launch would fail) -, the
512-thread form is built for the same four waves per SIMD (two workgroups per CU).  Neither may spill or use scratch: a spill in the
ranking loop is a memory round trip per key.  Only the kernels' resource records are read."""
import os

import pytest

from tests.test_kernel_resources import HIPCC, _resources


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_radix_scatter_forms_keep_four_waves_per_simd(tmp_path):
    rec = _resources(tmp_path, "radix.hip")
    for threads, lds in ((1024, 16 * 1024 + 1024 + 64 + 16), (512, 8 * 1024 + 1024 + 64 + 16)):  # static LDS: counters, bases, scan words
        for pairs in (0, 1):
            r = rec("k_radix_scatter_tILi%dELb%dEE" % (threads, pairs))
            assert r["vgpr"] <= 128 and r["spill"] == 0 and r["scratch"] == 0 and r["lds"] <= lds, (threads, pairs, r)
