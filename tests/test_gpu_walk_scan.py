"""The window scan of the parallel header walk (walk_kernels.hip, walk_speculate: several steps' loads in flight, a filter on two
bytes, the candidates' exact test put off to a list; the serial walk inside walk_write) on the device, at the smallest shapes
that still have at least four segments: the parallel index against the serial walk's (the test switch stenos_hip_test_walk, as in
tests/test_gpu_walk.py) and against the encoder's, and whether the serial walk had to run."""
import ctypes

import pytest
import torch

from stenos_amd.api import Stenos, StenosError
from stenos_amd.datagen import generate_torch

pytestmark = pytest.mark.gpu

MIB = 1 << 20


def _index(st, frame, T, csize, serial):
    st.lib.stenos_hip_test_walk(st.ctx, 1 if serial else 0)
    try:
        return st.frame_index(frame, T, csize)
    except StenosError:
        return None
    finally:
        st.lib.stenos_hip_test_walk(st.ctx, 0)


def _both(st, frame, T, csize):
    """-> (index by the parallel walk, whether the serial walk ran after all, index by the serial walk)"""
    par = _index(st, frame, T, csize, serial=False)
    fell_back = st.lib.stenos_hip_test_walk(st.ctx, 0)
    return par, fell_back, _index(st, frame, T, csize, serial=True)


def _encoder_index(st):
    p, nsb = st.last_index()
    enc = torch.empty(nsb + 1, dtype=torch.int64)
    hip = ctypes.CDLL("libamdhip64.so")
    assert hip.hipMemcpy(ctypes.c_void_p(enc.data_ptr()), ctypes.c_void_p(p), ctypes.c_size_t((nsb + 1) * 8), 2) == 0
    return enc.tolist()


def _segments(csize, first, sb):
    """walk.h, make_plan: segments of four windows"""
    return -(-(csize - first) // ((4 * (sb + 4) + 15) & ~15))


def _compress(st, src, T):
    dst = torch.empty(st.bound(src.numel()), dtype=torch.uint8, device="cuda")
    return dst, st.compress(src, T, dst)


def _mixed12(n_bytes):
    """12-byte elements: a superblock of 129 024 bytes, no power of two; compressible superblocks, then stored ones, then compressible ones"""
    q = n_bytes // 4 // 12
    return torch.cat([generate_torch("dict16", 12, q, 3), generate_torch("rand", 12, 2 * q, 4), generate_torch("dict16", 12, q, 5)])


CASES = [("rand12", 4, 16, 131072), ("rand", 4, 4, 131072), ("walk", 2, 8, 131072), ("sine", 8, 8, 131072), ("mixed12", 12, 6, 129024)]


@pytest.mark.parametrize("kind,T,mib,sb", CASES, ids=[f"{c[0]}-T{c[1]}" for c in CASES])
def test_the_codecs_own_frames(kind, T, mib, sb, hooks_lib):
    """rand at level 1: every superblock is stored, so each hop is exactly a window long (a root's hop equal to the window)"""
    src = _mixed12(mib * MIB) if kind == "mixed12" else generate_torch(kind, T, mib * MIB // T, 17)
    st = Stenos(1, lib=hooks_lib)
    dst, c = _compress(st, src, T)
    enc = _encoder_index(st)
    assert _segments(c, 8, sb) >= 4, (c, "too few segments: the parallel walk is not what runs")
    if kind == "rand":
        assert all(b - a == sb + 4 for a, b in zip(enc[:-2], enc[1:-1]))
    par, fell_back, ser = _both(st, dst, T, c)
    assert par is not None and par == ser and par == enc
    assert fell_back == 0, "a well-formed frame needed the serial walk"
    back = torch.zeros_like(src)
    assert st.decompress(dst, T, c, back) == src.numel() and torch.equal(back, src)
    st.close()


def test_a_payload_of_look_alikes_takes_the_serial_walk(hooks_lib):
    """Level 0 stores the input: 01 01 00 00 over and over makes every position of a payload a plausible header that points at
    another one -- thousands of candidates per window (more than the list holds), more than 64 roots: the segments are given up."""
    T = 4
    src = torch.tensor([1, 1, 0, 0], dtype=torch.uint8, device="cuda").repeat(4 * MIB // 4)
    st = Stenos(0, lib=hooks_lib)
    dst, c = _compress(st, src, T)
    enc = _encoder_index(st)
    assert _segments(c, 8, 131072) >= 4
    par, fell_back, ser = _both(st, dst, T, c)
    assert par is not None and par == ser and par == enc
    assert fell_back == 1, "the speculation cannot have held"
    back = torch.zeros_like(src)
    assert st.decompress(dst, T, c, back) == src.numel() and torch.equal(back, src)
    st.close()


def test_a_frame_stored_inside_a_frame(hooks_lib):
    """Level 0 of an input that is a level-1 frame itself: the payloads hold a second chain of true headers, so every window has
    the roots of two chains.  The stored chain is cut by the outer frame's headers every 131 072 bytes -- the hop over one lands
    four bytes short -- so it dies before its segment ends (the host replay of walk.h says the same of this input: no segment is
    given up), and the index is the outer chain's either way."""
    T = 4
    inner_src = generate_torch("rand12", T, 10 * MIB // T, 5)
    st1 = Stenos(1, lib=hooks_lib)
    inner, c1 = _compress(st1, inner_src, T)
    st1.close()
    assert 3 * MIB < c1 <= 4 * MIB
    src = torch.zeros(4 * MIB, dtype=torch.uint8, device="cuda")
    src[:c1] = inner[:c1]
    st = Stenos(0, lib=hooks_lib)
    dst, c = _compress(st, src, T)
    enc = _encoder_index(st)
    assert _segments(c, 8, 131072) >= 4
    par, fell_back, ser = _both(st, dst, T, c)
    assert par is not None and par == ser and par == enc
    assert fell_back == 0
    back = torch.zeros_like(src)
    assert st.decompress(dst, T, c, back) == src.numel() and torch.equal(back, src)
    st.close()


def test_cut_frames_as_the_serial_walk_sees_them(hooks_lib):
    """the rand12 frame with its size cut by 1 byte, by 5 bytes, and to the middle of a header (the last one's and one half way)"""
    T = 4
    src = generate_torch("rand12", T, 16 * MIB // T, 17)
    st = Stenos(1, lib=hooks_lib)
    dst, c = _compress(st, src, T)
    enc = _encoder_index(st)
    for size in (c - 1, c - 5, enc[-2] + 2, enc[len(enc) // 2] + 2):
        assert _segments(size, 8, 131072) >= 4
        par, _, ser = _both(st, dst, T, size)
        assert par == ser, size  # (None: the frame is refused, by both)
    # ... and whole again
    par, fell_back, ser = _both(st, dst, T, c)
    assert par == ser == enc and fell_back == 0
    st.close()
