"""The inputs of tests/test_group4_scalar_cpu.py (tests/group4_scalar_inputs.py: the scan of a group's blocks against the planes
the wave expects, every pair of planes, the mini-LZ gate on either side of its inequalities) through the library on the GPU: the
product library as it picks its kernel, and the test build with the non-temporal and the plain fused encoder forced.  Frames equal
the oracle's byte for byte and decode back.  A run of 32 blocks is what one wave takes of a superblock, so the runs are laid four
to a superblock: arrays of one to three superblocks, and one with a ragged tail."""
import numpy as np
import pytest
import torch

import group4_inputs as g4in
import group4_scalar_inputs as gsi
from _libs import oracle_compress
from stenos_amd.api import Stenos

pytestmark = pytest.mark.gpu

T = 4
PLAIN, NT = 1, 2


@pytest.fixture(scope="module")
def cases(oracle):
    """(name, bytes, the oracle's frame), computed once"""
    runs = [gsi.rand12_run(), gsi.plane_pairs(1), gsi.plane_pairs(2), gsi.first_varies()]
    for g, pos in gsi.PLACES:
        runs += [gsi.const_plane(0, g, pos), gsi.const_plane(1, g, pos)] + [gsi.third_plane(lane, g, pos) for lane in gsi.LANES]
    for t, (f, d) in enumerate(gsi.GATE_TARGETS):
        runs += [gsi.gate_run(oracle, gsi.RUN, 4 * g + (t + n) % 4, f, d) for n, g in enumerate(gsi.GROUPS)]
        runs.append(np.concatenate([gsi.gate_run(oracle, 4, pos, f, d) for pos in range(4)] * 2))  # (eight groups of their own)
    for kind in ("dict", "low_two"):
        v = g4in.rand12(gsi.RUN, 11)
        for pos in range(4):
            g4in.change_block(v, 8 * pos + pos, kind, 11)
        runs.append(v)
    assert all(r.size == gsi.RUN * gsi.BLOCK for r in runs)
    out = []
    for at in range(0, len(runs), 12):  # up to three superblocks an array
        part = runs[at:at + 12]
        part += [gsi.rand12_run(23)] * (-len(part) % 4)
        data = np.concatenate(part).view(np.uint8)
        out.append((f"runs{at}", data, oracle_compress(oracle, data, T, 1)[1]))
    data = np.concatenate(runs[4:8] + [g4in.rand12(5, 29), np.arange(77, dtype="<u4") & np.uint32(0xFFF)]).view(np.uint8)
    out.append(("ragged", data, oracle_compress(oracle, data, T, 1)[1]))
    return out


def _check(st, name, data, ref):
    src = torch.from_numpy(data.view(np.uint8).ravel()).cuda()
    cap = st.bound(src.numel())
    dst = torch.full((cap + 256,), 0xC3, dtype=torch.uint8, device="cuda")
    c = st.compress(src, T, dst[:cap])
    assert c == ref.size, name
    got = dst[:c].cpu().numpy()
    assert np.array_equal(got, ref), (name, np.nonzero(got != ref)[0][:8])
    assert bool((dst[cap:] == 0xC3).all()), (name, "wrote past dst_size")
    back = torch.zeros_like(src)
    assert st.decompress(dst, T, c, back) == src.numel() and torch.equal(back, src), name


def test_the_product_library_writes_the_oracles_frames(cases):
    st = Stenos(1)
    for name, data, ref in cases:
        _check(st, name, data, ref)
    st.close()


@pytest.mark.parametrize("variant", [NT, PLAIN], ids=["nt", "plain"])
def test_either_fused_kernel_writes_the_oracles_frames(cases, hooks_lib, variant):
    st = Stenos(1, lib=hooks_lib)
    st.lib.stenos_hip_test_fused_timeouts(st.ctx, -1 - variant)
    for name, data, ref in cases:
        _check(st, name, data, ref)
    st.close()
