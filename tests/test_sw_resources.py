"""The registers, the LDS and the private segment of the Smith-Waterman kernels (elprep_amd/csrc/sw.hip), read from the assembly hipcc
writes for gfx950 without a GPU, the way tests/test_kernel_resources.py does for the BGZF kernels.

The DP kernel runs one wave per problem and every step of its sweep waits for the step before it, so what hides that latency is other
waves on the same SIMD: the design asks for all eight.  Eight waves per SIMD need at most 512 / 8 = 64 vector registers per lane
(AGPRs included); the reference bytes take 4 KB of LDS per wave, 32 waves x 4 KB = 128 KB of a CU's 160.  A lane's strip lives in
registers (SwLane): an index into it that the compiler cannot resolve puts the whole struct into the private segment - the kernel then
showed 76 registers and 60 bytes of scratch - so "no private segment" is part of the bound."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def _resources(tmp_path, source):
    out = tmp_path / (source + ".s")
    subprocess.check_call([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "--cuda-device-only", "-S", "-w",
                           "-I", os.path.join(ROOT, "elprep_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           "-o", str(out), os.path.join(ROOT, "elprep_amd", "csrc", source)])
    text = out.read_text()
    recs = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s*(\d+).*?\.name:\s*(\S+).*?\.private_segment_fixed_size:\s*(\d+).*?\.vgpr_count:\s*(\d+).*?\.vgpr_spill_count:\s*(\d+)",
                         text, re.S):
        recs[m.group(2)] = dict(lds=int(m.group(1)), scratch=int(m.group(3)), vgpr=int(m.group(4)), spill=int(m.group(5)))

    def rec(part):
        names = [k for k in recs if part in k]
        assert len(names) == 1, (part, names)
        return recs[names[0]]
    return rec


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_sw_kernels_keep_their_occupancy(tmp_path):
    rec = _resources(tmp_path, "sw.hip")
    dp = rec("k_sw_dp")  # eight waves per SIMD: <= 64 registers, no spills, no private segment; the reference's 4096 bytes of LDS
    assert dp["vgpr"] <= 64 and dp["spill"] == 0 and dp["scratch"] == 0 and dp["lds"] == 4096, dp
    for name in ("k_sw_shortcut", "k_sw_write", "k_sw_decode"):
        k = rec(name)
        assert k["vgpr"] <= 64 and k["spill"] == 0 and k["scratch"] == 0 and k["lds"] == 0, (name, k)
