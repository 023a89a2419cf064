"""The queryname sort's kernels (qsort.hip) compiled for gfx950 (hipcc cross-compiles without a GPU): no scratch, no spills, and the
registers that keep eight waves per SIMD for the three per-record kernels."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_queryname_sort_kernels_use_no_scratch(tmp_path):
    out = tmp_path / "qsort.s"
    subprocess.check_call([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "--cuda-device-only", "-S", "-w",
                           "-I", os.path.join(ROOT, "elprep_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           "-o", str(out), os.path.join(ROOT, "elprep_amd", "csrc", "qsort.hip")])
    recs = {}
    for m in re.finditer(r"\.name:\s*(\S+).*?\.private_segment_fixed_size:\s*(\d+).*?\.vgpr_count:\s*(\d+).*?\.vgpr_spill_count:\s*(\d+)",
                         out.read_text(), re.S):
        recs[m.group(1)] = dict(scratch=int(m.group(2)), vgpr=int(m.group(3)), spill=int(m.group(4)))
    for part in ("k_qn_values", "k_qn_keys", "k_qn_ties"):
        names = [k for k in recs if part in k]
        assert len(names) == 1, (part, sorted(recs))
        r = recs[names[0]]
        assert r["scratch"] == 0 and r["spill"] == 0 and r["vgpr"] <= 64, (part, r)
