"""The inputs of tests/test_group4_paths_cpu.py (tests/group4_inputs.py: a kind for every precondition the group of four int32
blocks and its straight-line emission test, and one that breaks it in the second, third or fourth block of a group) through the
library on the GPU: the product library as it picks its kernel, and the test build with the non-temporal and the plain fused
encoder forced.  Frames equal the oracle's byte for byte and decode back.  Shapes: one group, a group and a remainder, groups on
both sides of a changed block, a superblock and three blocks; and three superblocks and a tail of `u & 0xFFF`, so that a
workgroup's tickets, the parity of its staging buffers and its deferred store all turn over once."""
import numpy as np
import pytest
import torch

import group4_inputs as g4in
from _libs import oracle_compress
from stenos_amd.api import Stenos
from stenos_amd.datagen import generate

pytestmark = pytest.mark.gpu

T = 4
PLAIN, NT = 1, 2
# (blocks, the changed block of every group); the fused encoders take whole superblocks of 128 blocks -- there the groups run --,
# the shorter inputs and the three blocks behind a superblock go through the encoder of single blocks
SHAPES = ((4, 1), (5, 2), (9, 3), (128 + 3, 1), (128 + 3, 2), (128 + 3, 3))


@pytest.fixture(scope="module")
def cases(oracle):
    """(name, bytes, the oracle's frame), computed once"""
    out = []
    for kind in g4in.KINDS:
        for n, pos in SHAPES:
            data = g4in.make(kind, n, pos)
            out.append((f"{kind}-{n}-{pos}", data, oracle_compress(oracle, data, T, 1)[1]))
    for d in (g4in.THRESHOLD_COUNTS[0], 24, 25, g4in.THRESHOLD_COUNTS[-1]):
        data = g4in.make("low_count", 128 + 3, 1, distinct=d)
        out.append((f"low_count{d}-131", data, oracle_compress(oracle, data, T, 1)[1]))
    data = generate("rand12", T, 3 * 32768 + 5 * 256 + 77, 23)
    out.append(("rand12-3sb-tail", data, oracle_compress(oracle, data, T, 1)[1]))
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
