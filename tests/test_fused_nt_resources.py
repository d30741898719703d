"""The non-temporal fused encoder of bytesoftype 4 (kernels.hip, encode_superblocks_nt), checked with the cross compiler (no GPU):
it is compiled for the workgroups per CU it is launched with, it keeps out of scratch memory but for a register or two -- its input and frame accesses
are global ones, not flat accesses the compiler must assume may alias the stack --, and it exists for bytesoftype 4 only."""
import os
import re
import shutil
import subprocess

import pytest

from _libs import ROOT

NT_OCCUPANCY = 7  # kernels.hip, FUSED_NT_OCCUPANCY


def _usage(source, flags):
    cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-c", os.path.join(ROOT, "stenos_amd", "csrc", source),
           "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"] + flags
    err = subprocess.run(cmd, capture_output=True, text=True, timeout=900).stderr
    res, cur = {}, None
    for line in err.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = res.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[bytes/lane\]| \[waves/SIMD\])?: (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return res


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_nt_encoder_resources_stay_inside_their_budget():
    enc = _usage("kernels.hip", ["-DWV_PREDICATE_BRANCHES"])
    nt = {k: v for k, v in enc.items() if "encode_superblocks_nt" in k}
    assert list(nt) and all("encode_superblocks_ntILj4E" in k for k in nt), sorted(nt)
    e = next(iter(nt.values()))
    assert e["Occupancy"] == NT_OCCUPANCY, e
    assert e["ScratchSize"] <= 8 and e["VGPRs Spill"] <= 2, e  # (a register or two parked, as in the int16 kernel; the plain int32 one has 24 bytes)
    assert e["TotalSGPRs"] <= 96, e  # (above 96 a SIMD holds fewer than eight waves' scalar registers; seven are asked for)
    src = open(os.path.join(ROOT, "stenos_amd", "csrc", "kernels.hip")).read()
    assert re.search(r"constexpr uint32_t FUSED_NT_OCCUPANCY = (\d+);", src).group(1) == str(NT_OCCUPANCY)
