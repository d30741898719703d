"""The two fused encoders of bytesoftype 4 after the cut of scalar instructions on the path of a group of four blocks
(slot_codec.h: scan_expected_group4, write_slots_group4; block_codec.h: lz_precheck_passes_lanes), checked with the cross
compiler (no GPU).

The cut may cost neither vector registers, scratch memory nor a resident wave: both kernels keep what their parent (353ca73) had,
72 / 64 registers, 8 / 24 bytes of scratch, 7 / 8 waves.

And it adds no divergent branch to the group's path.  The new decisions are taken on wave-uniform scalars -- the planes the wave
expects and the plane numbers derived from them --, and a branch on a value the compiler takes for divergent is laid out around
lane masks.  LLVM's uniformity analysis (tools/divergent_branches.sh) lists the divergent branches under the group's
lambda; by the function they stand in, there are no more of them than at the parent, and none in the new functions."""
import collections
import os
import re
import shutil
import subprocess

import pytest

from _libs import ROOT
from test_fused_nt_resources import _usage

# kernel -> (VGPRs, ScratchSize [bytes/lane], VGPRs Spill, Occupancy [waves/SIMD]) at the parent
FIGURES = {
    "encode_superblocks_ntILj4E": (72, 8, 1, 7),
    "encode_superblocksILj4E": (64, 24, 5, 8),
}
# kernel -> function the branch stands in -> divergent branches under group4 (the lambda encode_blocks_to calls) at the parent:
# the predicated stores and the regions of lanes_below; in the plain kernel also the two tests of a sink that only measures
PARENT_DIVERGENT = {
    "encode_superblocks_ntILj4E": {"gst128": 2, "lanes_below": 2, "lds_st128": 1, "lds_st32": 4, "slot_rows_analyse": 4, "slot_rows_reload": 1, "stream_append": 2},
    "encode_superblocksILj4E": {"append": 1, "gst128": 2, "lanes_below": 1, "lds_st128": 1, "lds_st32": 4, "operator()": 2, "slot_rows_analyse": 2,
                                "slot_rows_reload": 1, "stream_append": 2},
}
NEW_FUNCTIONS = ("scan_expected_group4", "write_slots_group4", "lz_precheck_passes_lanes", "plane_bytes")


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_the_int32_encoders_keep_their_registers_scratch_and_waves():
    enc = _usage("kernels.hip", ["-DWV_PREDICATE_BRANCHES"])
    for key, (vgprs, scratch, spill, occupancy) in FIGURES.items():
        hits = [v for k, v in enc.items() if key in k]
        assert len(hits) == 1, (key, [k for k in enc if key in k])
        e = hits[0]
        assert e["VGPRs"] <= vgprs, (key, e)
        assert e["ScratchSize"] <= scratch and e["VGPRs Spill"] <= spill, (key, e)
        assert e["Occupancy"] == occupancy, (key, e)


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_the_group_path_has_no_divergent_branch_its_parent_had_not():
    keys = list(PARENT_DIVERGENT)
    p = subprocess.run([os.path.join(ROOT, "tools", "divergent_branches.sh"), "kernels.hip"] + keys + ["--", "-DWV_PREDICATE_BRANCHES"],
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-1500:]
    found = {k: collections.Counter() for k in keys}
    key = None
    for line in p.stdout.splitlines():
        if line.startswith("== "):
            key = line.split()[1]
            continue
        m = re.match(r"\s*(\d+) (.*)", line)
        if not m:
            continue
        frames = m.group(2).split(" <- ")
        assert not any(f.startswith(NEW_FUNCTIONS) for f in frames), line
        # (group4 is the lambda without template arguments that encode_blocks_to calls; the passes' lambda has a type argument)
        if any(re.fullmatch(r"operator\(\):\d+", f) and frames[i + 1].startswith("encode_blocks_to") for i, f in enumerate(frames[:-1])):
            found[key][re.match(r"[\w~]+(\(\))?", frames[0]).group(0)] += int(m.group(1))
    for k in keys:
        assert sum(found[k].values()) > 0, (k, "the tool listed nothing under group4: its output has changed")
        for leaf, n in found[k].items():
            assert n <= PARENT_DIVERGENT[k].get(leaf, 0), (k, leaf, n, dict(found[k]))
