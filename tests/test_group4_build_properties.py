"""The two fused encoders of bytesoftype 4 after the instruction cuts on the path of a group of four blocks (slot_codec.h:
lz_distinct_keys_group4, slot_rows_emit_rows_packed), checked with the cross compiler (no GPU): a cut that costs vector registers,
scratch memory or a resident wave takes back more than it gives, so neither kernel may use more of them than its parent did.

The parent's figures: commit b2ad1cb, its sources compiled with the product's flags (stenos_amd/csrc/Makefile, as
tools/build_variant.sh builds a variant of them) and -Rpass-analysis=kernel-resource-usage.  "No scratch" means for these two
kernels what it meant there: the eight bytes of one parked register in the non-temporal kernel, the 24 bytes the cold mini-LZ
branches of the plain one spill (tests/test_build_properties.py, tests/test_fused_nt_resources.py) -- and not a byte more."""
import shutil

import pytest

from test_fused_nt_resources import _usage

PARENT = "b2ad1cb"
# kernel -> (VGPRs, ScratchSize [bytes/lane], VGPRs Spill, Occupancy [waves/SIMD]) at PARENT
PARENT_FIGURES = {
    "encode_superblocks_ntILj4E": (72, 8, 1, 7),
    "encode_superblocksILj4E": (64, 24, 5, 8),
}


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_the_int32_encoders_use_no_more_registers_or_scratch_than_their_parent():
    enc = _usage("kernels.hip", ["-DWV_PREDICATE_BRANCHES"])
    for key, (vgprs, scratch, spill, occupancy) in PARENT_FIGURES.items():
        hits = [v for k, v in enc.items() if key in k]
        assert len(hits) == 1, (key, [k for k in enc if key in k])
        e = hits[0]
        assert e["VGPRs"] <= vgprs, (key, e)
        assert e["ScratchSize"] <= scratch and e["VGPRs Spill"] <= spill, (key, e)
        assert e["Occupancy"] == occupancy, (key, e)
