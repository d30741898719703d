"""The two fused encoders of bytesoftype 4 (kernels.hip): encode_superblocks, ordinary accesses and eight workgroups per CU, and
encode_superblocks_nt, non-temporal input and frame and fewer workgroups.  The library picks one per call (encode_host.cpp: the nt
kernel unless the context's last fused call stored more than half its superblocks as copies); the test build can force either
(stenos_hip_test_fused_timeouts(ctx, -1 - v)).  Both must write the oracle's frame byte for byte whatever the data: 12-bit
values, full entropy, copies and coded superblocks in every alternation, more superblocks than resident workgroups, and a
context whose data changes character from call to call."""
import numpy as np
import pytest
import torch

from _libs import oracle_compress
from stenos_amd.api import Stenos
from stenos_amd.datagen import generate

pytestmark = pytest.mark.gpu

T = 4
AUTO, PLAIN, NT = 0, 1, 2


def _context(hooks_lib, variant):
    st = Stenos(1, lib=hooks_lib)
    st.lib.stenos_hip_test_fused_timeouts(st.ctx, -1 - variant)
    return st


def _check(st, data, ref):
    src = torch.from_numpy(data.view(np.uint8).ravel()).cuda()
    cap = st.bound(src.numel())
    dst = torch.full((cap + 256,), 0xC3, dtype=torch.uint8, device="cuda")
    c = st.compress(src, T, dst[:cap])
    assert c == ref.size
    got = dst[:c].cpu().numpy()
    assert np.array_equal(got, ref), np.nonzero(got != ref)[0][:8]
    assert bool((dst[cap:] == 0xC3).all()), "wrote past dst_size"
    back = torch.zeros_like(src)
    assert st.decompress(dst, T, c, back) == src.numel() and torch.equal(back, src)


def _codes(frame):
    codes, p = [], 12 if frame[0] == 255 else 8
    while p + 4 <= frame.size:
        codes.append(int(frame[p]))
        p += 4 + (int(frame[p + 1]) | (int(frame[p + 2]) << 8) | (int(frame[p + 3]) << 16))
    return codes


def _mixed(mib, seed):
    """stretches of 1..40 superblocks of noise, 12-bit values, sorted values and constants in random order, and a partial
    superblock at the end (as in test_gpu_speculative_copy.py)"""
    rng = np.random.default_rng(seed)
    sb = 131072
    left, parts = (mib << 20) // sb, []
    kinds = ["rand", "rand12", "sorted", "same", "rand"]
    while left:
        n = int(min(left, rng.integers(1, 41)))
        parts.append(generate(kinds[int(rng.integers(0, len(kinds)))], T, n * sb // T, int(rng.integers(0, 1 << 30))).view(np.uint8).ravel())
        left -= n
    parts.append(generate("rand", T, 1000, 5).view(np.uint8).ravel())
    return np.ascontiguousarray(np.concatenate(parts))


@pytest.mark.parametrize("kind,elements", [("rand12", (640 << 20) // 4), ("rand12", 3_000_003), ("rand", (384 << 20) // 4 + 77), ("mixed", 400)])
def test_both_kernels_write_the_oracles_frame(oracle, hooks_lib, kind, elements):
    """640 MiB of 12-bit values are 5 120 superblocks: more than the workgroups of either kernel, so every workgroup goes on past
    its first superblock and its first staging buffer."""
    data = _mixed(elements, 11) if kind == "mixed" else generate(kind, T, elements, 42)
    _, ref = oracle_compress(oracle, data, T, 1)
    codes = set(_codes(ref))
    assert {"rand12": {1}, "rand": {6}, "mixed": {1, 6}}[kind] <= codes  # (the case is what it says)
    for variant in (PLAIN, NT):
        st = _context(hooks_lib, variant)
        _check(st, data, ref)
        _check(st, data, ref)  # (a second call on the same context: warm buffers, the other staging parity)
        st.close()


def test_the_choice_between_calls_follows_the_data(oracle, hooks_lib):
    """One context, the library's own rule: compressible, incompressible, incompressible, compressible, mixed, compressible --
    the kernel changes after the first incompressible call and after the first compressible one behind it."""
    mib = 256
    seq = [generate("rand12", T, (mib << 20) // T, 1), generate("rand", T, (mib << 20) // T + 5, 2), generate("rand", T, (mib << 20) // T, 3),
           generate("sorted", T, (mib << 20) // T + 1, 4), _mixed(mib, 5), generate("rand12", T, (mib << 20) // T, 6)]
    refs = [oracle_compress(oracle, d, T, 1)[1] for d in seq]
    st = _context(hooks_lib, AUTO)
    for d, ref in zip(seq, refs):
        _check(st, d, ref)
    st.close()
    st = Stenos(1)  # (the product library: the same rule, nothing forced)
    for d, ref in zip(seq, refs):
        _check(st, d, ref)
    st.close()
