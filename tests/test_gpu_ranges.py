"""Byte ranges of a frame on the device (include/stenos_hip.h: stenos_hip_decompress_ranges): every range of a call equals the
slice of stenos_hip_decompress's output, whatever the superblock codes, the index form, the alignment of the destinations;
nothing is written outside a destination, on success or on any error; the caller's index survives any number of calls; the
refusals happen before anything is written; damage is seen where a range looks and nowhere else."""
import base64
import ctypes
import json
import os

import numpy as np
import pytest

import streamgen as sg
from stenos_amd.api import Stenos, StenosError
from stenos_amd.datagen import generate

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
E = lambda k: (1 << 64) - k  # noqa: E731
INVALID_PARAMETER, SRC_OVERFLOW, INVALID_INPUT = E(9), E(2), E(4)
GUARD, GUARD_BYTE = 64, 0xA5
TS = [2, 4, 8, 3, 12, 64]


def _cuda():
    import torch

    assert torch.cuda.is_available()
    return torch


def _data(kind, T, nbytes, seed):
    if (kind == "rand12" and T != 4) or (kind == "sine" and T not in (4, 8)):  # (int32 data / float data)
        kind = "rand8" if kind == "rand12" else "slopes"
    return np.ascontiguousarray(generate(kind, T, nbytes // T + 1, seed).view(np.uint8)[:nbytes])


def _mixed_data(T, nbytes, sb, seed):
    """one kind per superblock: compressible ones, noise (stored as copies) and dictionary data (mini-LZ blocks)"""
    kinds = ("walk", "rand12", "rand", "lzmix" if T == 4 else "dict16", "sine", "runs")
    parts = [_data(kinds[(s + seed) % len(kinds)], T, min(sb, nbytes - at), seed + s) for s, at in enumerate(range(0, nbytes, sb))]
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)


def _sb(T, shift=None):
    bs = 256 * T
    return bs << shift if shift is not None else sg.base_superblock(T)


def _sizes(T, sb):
    """1 superblock; 2 + 300 bytes; 2 + 100 bytes (a last superblock under 128 bytes: zstd-coded); 3 + a partial block; an exact multiple"""
    bs = 256 * T
    return [sb, 2 * sb + 300, 2 * sb + 100, 3 * sb + (bs if sb > bs else 0) + 37 * T + 5, 2 * sb]


def range_set(total, sb, bs, rng, nrandom=200):
    r = [(0, 0), (0, 1), (total - 1, 1), (0, total), (total, 0), (total // 2, 0)]
    for b in range(sb, total + 1, sb):  # superblock boundaries: one byte on both sides
        r.append((b - 1, 1))
        if b < total:
            r += [(b - 1, 2), (b, 1)]
    nsb = (total + sb - 1) // sb
    if nsb >= 2:
        r.append((sb * ((nsb - 1) // 2), min(sb, total - sb * ((nsb - 1) // 2))))  # a whole superblock (an interior one where there is one), exactly
    for b in sorted({bs, 2 * bs, ((total // bs) // 2) * bs, (total // bs) * bs}):  # block boundaries
        if 0 < b < total:
            r += [(b - 1, 1), (b, 1), (b - 1, 2)]
            if b + 3 <= total and b >= 2:
                r.append((b - 2, 5))
    tail = total % bs
    if tail:  # into the last superblock's partial block, its rows and the raw bytes behind them
        r += [(total - tail, tail), (max(0, total - tail - 3), min(total, 3 + tail)), (total - (tail % (16 * bs // 256) or 1), tail % (16 * bs // 256) or 1)]
    r += [(1, min(777, total - 1)), (min(total - 1, 12345), min(total - min(total - 1, 12345), 4321)), (total // 3 | 1, min(total - (total // 3 | 1), 33333))]
    for _ in range(nrandom):
        lo = int(rng.integers(0, total))
        cap = int(rng.choice([7, 300, 300, 300, 5000, 5000, 70000]))
        r.append((lo, int(rng.integers(1, min(cap, total - lo) + 1))))
    r += [r[-1], r[len(r) // 2]]  # the same range twice
    assert all(0 <= lo and n >= 0 and lo + n <= total for lo, n in r)
    return r


class Carved:
    """destinations out of one buffer: misalignments 0..15 in turn, 64 guard bytes of 0xA5 between them and at both ends"""

    def __init__(self, torch, ranges):
        self.at = []
        pos = GUARD
        for i, (_, n) in enumerate(ranges):
            pos = (pos + 15) // 16 * 16 + i % 16
            self.at.append(pos)
            pos += n + GUARD
        self.buf = torch.full((pos + 16,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
        self.ranges = ranges
        self.ptrs = [self.buf.data_ptr() + a for a in self.at]

    def expected(self, full):
        want = np.full(self.buf.numel(), GUARD_BYTE, dtype=np.uint8)
        for (lo, n), a in zip(self.ranges, self.at):
            want[a:a + n] = full[lo:lo + n]
        return want

    def check(self, full):
        got = self.buf.cpu().numpy()
        want = self.expected(full)
        if not np.array_equal(got, want):
            bad = int(np.flatnonzero(got != want)[0])
            i = max(k for k, a in enumerate(self.at) if a - GUARD <= bad) if bad >= self.at[0] - GUARD else 0
            raise AssertionError(f"byte {bad} of the buffer differs (got {got[bad]}, want {want[bad]}): around range {i} = {self.ranges[i]} placed at {self.at[i]}")

    def guards_intact(self):
        got = self.buf.cpu().numpy()
        mask = np.ones(got.size, dtype=bool)
        for (_, n), a in zip(self.ranges, self.at):
            mask[a:a + n] = False
        return bool((got[mask] == GUARD_BYTE).all())

    def untouched(self):
        return bool((self.buf == GUARD_BYTE).all().item())


def _full_decode(st, torch, frame, T, csize, total):
    out = torch.zeros(total, dtype=torch.uint8, device="cuda")
    assert st.decompress(frame, T, csize, out) == total
    return out.cpu().numpy()


def _check_all_index_forms(st, torch, frame, T, csize, full, ranges, last_index=None):
    """no index, the index of the compression (where there was one), the index of stenos_hip_frame_index"""
    want = sum(n for _, n in ranges)
    c = Carved(torch, ranges)
    assert st.decompress_ranges(frame, T, csize, ranges, c.ptrs) == want
    c.check(full)
    if last_index:
        c = Carved(torch, ranges)
        assert st.decompress_ranges(frame, T, csize, ranges, c.ptrs, last_index) == want
        c.check(full)
    n = ctypes.c_size_t(0)
    p = st.lib.stenos_hip_frame_index(st.ctx, frame.data_ptr(), T, csize, ctypes.byref(n), st._stream_ptr())
    assert p
    c = Carved(torch, ranges)
    assert st.decompress_ranges(frame, T, csize, ranges, c.ptrs, p) == want
    c.check(full)
    return p


@pytest.mark.parametrize("shift", [None, 0, 2])
@pytest.mark.parametrize("T", TS)
def test_level1_frames(T, shift):
    torch = _cuda()
    st = Stenos(level=1)
    try:
        if shift is not None:
            assert st.lib.stenos_set_block_size(st.ctx, shift) == 0
        sb, bs = _sb(T, shift), 256 * T
        rng = np.random.default_rng([21, T, shift or 9])
        for k, total in enumerate(_sizes(T, sb)):
            data = _mixed_data(T, total, sb, 3 * T + k)
            src = torch.from_numpy(data).cuda()
            frame = torch.zeros(st.bound(total) + 8 * (total // sb + 2), dtype=torch.uint8, device="cuda")  # (stenos_bound counts default superblocks)
            csize = st.compress(src, T, frame)
            last, nsb = st.last_index()
            assert last and nsb == (total + sb - 1) // sb
            ranges = range_set(total, sb, bs, rng, 200 if k == 3 else 60)
            # (the index of the compression first: the calls that follow overwrite the context's index)
            c = Carved(torch, ranges)
            assert st.decompress_ranges(frame, T, csize, ranges, c.ptrs, last) == sum(n for _, n in ranges)
            c.check(data)
            full = _full_decode(st, torch, frame, T, csize, total)
            assert np.array_equal(full, data)
            _check_all_index_forms(st, torch, frame, T, csize, full, ranges)
    finally:
        st.close()


@pytest.mark.parametrize("T", TS)
def test_level0_frames_are_copies(T):
    torch = _cuda()
    st = Stenos(level=0)
    try:
        sb, bs = _sb(T), 256 * T
        rng = np.random.default_rng([22, T])
        for total in (sb, 2 * sb + 300, 3 * sb + 37 * T + 5):
            data = _data("rand", T, total, T)
            frame = torch.zeros(st.bound(total), dtype=torch.uint8, device="cuda")
            csize = st.compress(torch.from_numpy(data).cuda(), T, frame)
            full = _full_decode(st, torch, frame, T, csize, total)
            _check_all_index_forms(st, torch, frame, T, csize, full, range_set(total, sb, bs, rng, 100))
    finally:
        st.close()


@pytest.mark.parametrize("default_size", [False, True])
@pytest.mark.parametrize("T", TS)
def test_frames_no_encoder_writes(T, default_size):
    """tests/streamgen.py: copied superblocks among block-coded ones, every block form, oversize blocks"""
    torch = _cuda()
    st = Stenos(level=1)
    try:
        rng = np.random.default_rng([23, T, int(default_size)])
        bps = 3
        sb = sg.base_superblock(T) if default_size else bps * 256 * T
        frame_np, offs, data = sg.make_mixed_frame(rng, T, 2 if default_size else 9, bps, min(sb - 1, 256 * T + 21 * T + 3), default_size=default_size)
        frame = torch.from_numpy(frame_np).cuda()
        full = _full_decode(st, torch, frame, T, frame_np.size, data.size)
        assert np.array_equal(full, data)
        _check_all_index_forms(st, torch, frame, T, frame_np.size, full, range_set(data.size, sb, 256 * T, rng, 200))
    finally:
        st.close()


with open(os.path.join(HERE, "golden", "level_frames.json")) as f:
    LEVEL_CASES = json.load(f)["cases"]


def _case_input(e):
    if "input_b64" in e:
        return np.frombuffer(base64.b64decode(e["input_b64"]), dtype=np.uint8).copy()
    return generate(e["kind"], e["T"], e["n"], 42)


@pytest.mark.parametrize("e", LEVEL_CASES, ids=lambda e: f"{e['kind']}-T{e['T']}-l{e['level']}-codes{''.join(map(str, e['codes']))}")
def test_reference_frames_of_higher_levels(e):
    """zstd-based codes 2-5 (and bytesoftype 1): finished on the host unit by unit"""
    torch = _cuda()
    st = Stenos(level=1)
    try:
        T = e["T"]
        frame_np = np.frombuffer(base64.b64decode(e["frame_b64"]), dtype=np.uint8).copy()
        data = _case_input(e)
        frame = torch.from_numpy(frame_np).cuda()
        full = _full_decode(st, torch, frame, T, frame_np.size, data.nbytes)
        assert np.array_equal(full, data.view(np.uint8).ravel())
        rng = np.random.default_rng([24, T, e["level"]])
        sb = sg.base_superblock(T)
        _check_all_index_forms(st, torch, frame, T, frame_np.size, full, range_set(full.size, sb, 256 * T, rng, 40))
    finally:
        st.close()


@pytest.mark.parametrize("level", [2, 3, 9])
@pytest.mark.parametrize("T", [1, 2, 4, 8])
def test_own_frames_of_higher_levels(T, level):
    torch = _cuda()
    st = Stenos(level=level)
    try:
        sb = sg.base_superblock(T)
        total = 2 * sb + 4000 + 3
        data = _mixed_data(max(T, 2), total, sb, level)  # (bytes are bytes: bytesoftype 1 takes the int16 kinds)
        frame = torch.zeros(st.bound(total), dtype=torch.uint8, device="cuda")
        csize = st.compress(torch.from_numpy(data).cuda(), T, frame)
        full = _full_decode(st, torch, frame, T, csize, total)
        assert np.array_equal(full, data)
        rng = np.random.default_rng([25, T, level])
        _check_all_index_forms(st, torch, frame, T, csize, full, range_set(total, sb, 256 * T, rng, 40))
    finally:
        st.close()


def _walk_frame(st, torch, T, nsb_bytes):
    data = _data("walk", T, nsb_bytes, 5)
    frame = torch.zeros(st.bound(data.nbytes), dtype=torch.uint8, device="cuda")
    csize = st.compress(torch.from_numpy(data).cuda(), T, frame)
    return data, frame, csize


def test_the_callers_index_survives():
    """the pointer of stenos_hip_frame_index: three calls in a row give the same, and a full decode given that pointer still round-trips"""
    torch = _cuda()
    st = Stenos(level=1)
    try:
        T, sb = 4, _sb(4)
        data, frame, csize = _walk_frame(st, torch, T, 5 * sb + 999)
        offs = st.frame_index(frame, T, csize)
        n = ctypes.c_size_t(0)
        p = st.lib.stenos_hip_frame_index(st.ctx, frame.data_ptr(), T, csize, ctypes.byref(n), st._stream_ptr())
        assert p and n.value == 6
        rng = np.random.default_rng(26)
        ranges = range_set(data.nbytes, sb, 256 * T, rng, 200)
        outs = []
        for _ in range(3):
            c = Carved(torch, ranges)
            assert st.decompress_ranges(frame, T, csize, ranges, c.ptrs, p) == sum(k for _, k in ranges)
            c.check(data)
            outs.append(c.buf.cpu().numpy())
        assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])
        index = torch.empty(7, dtype=torch.int64)
        hip = ctypes.CDLL("libamdhip64.so")
        assert hip.hipMemcpy(ctypes.c_void_p(index.data_ptr()), ctypes.c_void_p(p), ctypes.c_size_t(56), 2) == 0
        assert index.tolist() == offs
        back = torch.zeros(data.nbytes, dtype=torch.uint8, device="cuda")
        assert st.decompress(frame, T, csize, back, p) == data.nbytes
        assert np.array_equal(back.cpu().numpy(), data)
        out = torch.zeros(100, dtype=torch.uint8, device="cuda")
        assert st.decompress_range(frame, T, csize, sb - 50, 100, out, p) == 100
        assert np.array_equal(out.cpu().numpy(), data[sb - 50:sb + 50])
    finally:
        st.close()


def _code(call):
    try:
        return call()
    except StenosError as err:
        return err.code


def test_refusals_write_nothing():
    torch = _cuda()
    st = Stenos(level=1)
    try:
        T, sb = 4, _sb(4)
        data, frame, csize = _walk_frame(st, torch, T, 2 * sb + 77)
        total = data.nbytes
        ok = [(0, 10), (sb - 3, 6)]
        for bad in ((total - 4, 5), (total, 1), (total + 1, 0), (2**64 - 1, 2), (2**64 - 1, 0), (5, 2**64 - 3), (1, total)):
            ranges = ok + [bad] + ok
            c = Carved(torch, [(lo, min(n, 64)) for lo, n in ranges])
            assert _code(lambda: st.decompress_ranges(frame, T, csize, ranges, c.ptrs)) == INVALID_PARAMETER, bad
            assert c.untouched(), bad
        for badT in (0, 65):
            c = Carved(torch, ok)
            assert _code(lambda: st.decompress_ranges(frame, badT, csize, ok, c.ptrs)) == INVALID_PARAMETER, badT
            assert c.untouched()
        assert st.decompress_ranges(frame, T, csize, [], []) == 0
        # a pending _async job: refused, and the job is left alone
        src = torch.from_numpy(data).cuda()
        other = torch.zeros(st.bound(total), dtype=torch.uint8, device="cuda")
        st.compress(src, T, other, wait=False)
        c = Carved(torch, ok)
        assert _code(lambda: st.decompress_ranges(frame, T, csize, ok, c.ptrs)) == INVALID_PARAMETER
        assert c.untouched()
        assert st.finish() == csize
        assert torch.equal(other[:csize], frame[:csize])
        c = Carved(torch, ok)
        assert st.decompress_ranges(frame, T, csize, ok, c.ptrs) == 16
        c.check(data)
    finally:
        st.close()


def test_damage_is_seen_where_a_range_looks():
    torch = _cuda()
    st = Stenos(level=1)
    try:
        T, sb = 4, _sb(4)
        data, frame, csize = _walk_frame(st, torch, T, 3 * sb + 500)
        offs = st.frame_index(frame, T, csize)
        def index_ptr(f, size):
            n = ctypes.c_size_t(0)
            return st.lib.stenos_hip_frame_index(st.ctx, f.data_ptr(), T, size, ctypes.byref(n), st._stream_ptr())

        touching = [(10, 100), (sb + 5, 1000), (2 * sb - 2, 2)]  # superblocks 0 and 1
        # a byte flipped in superblock 2, which no range touches: not seen, with or without an index
        flipped = frame.clone()
        flipped[offs[2] + 4 + 40] = flipped[offs[2] + 4 + 40] ^ 0xFF
        for p in (None, index_ptr(flipped, csize)):
            c = Carved(torch, touching)
            assert st.decompress_ranges(flipped, T, csize, touching, c.ptrs, p) == 1102
            c.check(data)
        # the frame cut short inside superblock 1: its csize runs past the end
        p = index_ptr(frame, csize)
        cut = offs[1] + 4 + 10
        for idx in (p, None):
            c = Carved(torch, touching)
            assert _code(lambda: st.decompress_ranges(frame, T, cut, touching, c.ptrs, idx)) in (SRC_OVERFLOW, INVALID_INPUT), idx
            assert c.guards_intact()
        c = Carved(torch, touching[:1])  # ... which a call that stays in superblock 0 does not see, given the index
        assert st.decompress_ranges(frame, T, cut, touching[:1], c.ptrs, p) == 100
        c.check(data)
        p = index_ptr(frame, csize)  # (the call without an index walked the cut frame into the context's index)
        # an unknown code and a block stream that ends too early in a touched superblock
        for at, value in ((offs[1], 9), (offs[1] + 1, 7)):
            bad = frame.clone()
            if at == offs[1] + 1:  # csize := 7: the payload ends inside the first block (the index is given, so the chain is not walked)
                bad[at:at + 3] = torch.tensor([7, 0, 0], dtype=torch.uint8, device="cuda")
            else:
                bad[at] = value
            c = Carved(torch, touching)
            assert _code(lambda: st.decompress_ranges(bad, T, csize, touching, c.ptrs, p)) == INVALID_INPUT, (at, value)
            assert c.guards_intact()
    finally:
        st.close()


def test_non_default_stream():
    """The frame is written on a side stream behind a few milliseconds of other work there; only work ordered on that stream sees it."""
    torch = _cuda()
    st = Stenos(level=1)
    try:
        T, sb = 8, _sb(8)
        s = torch.cuda.Stream()
        data = _data("sine", T, 3 * sb + 4321, 9)
        ready = torch.from_numpy(data).cuda()
        src = torch.zeros_like(ready)
        dst = torch.zeros(st.bound(data.nbytes), dtype=torch.uint8, device="cuda")
        frame = torch.zeros_like(dst)
        busy = torch.zeros(64 << 20, dtype=torch.float32, device="cuda")
        rng = np.random.default_rng(27)
        ranges = range_set(data.nbytes, sb, 256 * T, rng, 100)
        c = Carved(torch, ranges)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            for _ in range(200):
                busy.add_(1.0)
            src.copy_(ready)
            csize = st.compress(src, T, dst)
            for _ in range(200):
                busy.add_(1.0)
            frame.copy_(dst)
            got = st.decompress_ranges(frame, T, csize, ranges, c.ptrs)
        torch.cuda.synchronize()
        assert got == sum(n for _, n in ranges)
        c.check(data)
    finally:
        st.close()
