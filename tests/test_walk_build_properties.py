"""walk_speculate (stenos_amd/csrc/walk_kernels.hip), checked with the cross compiler (no GPU): a lane holds the bytes of several
steps of the window scan in registers at once (walk.h, SCAN_STEPS), and still the kernel uses no scratch memory, spills nothing and
runs eight waves per SIMD -- the 2 048 workgroups of four waves that a long frame needs are then resident in one round on 256 CUs."""
import os
import re
import shutil
import subprocess

import pytest

from _libs import ROOT


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_walk_speculate_keeps_eight_waves_without_scratch():
    # (csrc/Makefile: walk_kernels.hip is built with the encoders' flags)
    cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-c", os.path.join(ROOT, "stenos_amd", "csrc", "walk_kernels.hip"),
           "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage", "-DWV_PREDICATE_BRANCHES"]
    err = subprocess.run(cmd, capture_output=True, text=True, timeout=900).stderr
    res, cur = {}, None
    for line in err.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = res.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[bytes/lane\]| \[waves/SIMD\]| \[bytes/block\])?: (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    hits = [v for k, v in res.items() if "walk_speculate" in k]
    assert len(hits) == 1, list(res)
    k = hits[0]
    assert k["ScratchSize"] == 0 and k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0, k
    assert k["Occupancy"] == 8 and k["VGPRs"] <= 64, k
    # eight workgroups per CU must fit the LDS as well (160 KiB per CU)
    assert k["LDS Size"] * 8 <= 160 * 1024, k
