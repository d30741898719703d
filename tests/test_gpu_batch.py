"""Batches on the device (include/stenos_hip.h: stenos_hip_compress_batch / stenos_hip_decompress_batch): every frame equals
the oracle's and the single call's byte for byte, tight destinations overflow exactly where the single call does and nothing is
written past them, round trips are exact, frames the library did not make (reference frames with zstd-coded superblocks,
truncated or malformed ones) get the single call's result item by item, and the refusals write nothing."""
import base64
import ctypes
import json
import os

import numpy as np
import pytest

from _libs import oracle_compress
from stenos_amd.api import ERR_BASE, Stenos, StenosError
from stenos_amd.datagen import generate

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
E = lambda k: (1 << 64) - k  # noqa: E731
DST_OVERFLOW, INVALID_PARAMETER, SRC_OVERFLOW, INVALID_INPUT = E(6), E(9), E(2), E(4)
KINDS = ("rand12", "walk", "sine", "dict16", "steps", "rand")


def _cuda():
    import torch

    assert torch.cuda.is_available()
    return torch


def _data(kind, T, nbytes, seed):
    if (kind == "rand12" and T != 4) or (kind == "sine" and T not in (4, 8)):  # (int32 data / float data)
        kind = "rand8" if kind == "rand12" else "slopes"
    return np.ascontiguousarray(generate(kind, T, nbytes // T + 1, seed).view(np.uint8)[:nbytes])


def _sb(T, shift=None):
    bs = 256 * T
    return bs << shift if shift is not None else (131072 // bs) * bs if bs <= 131072 else bs


def _sizes(T, sb):
    return [0, 1, T - 1, 255 * T, 256 * T, sb - 1, sb, sb + 1, sb + 100, 2 * sb + 300, 3 * (1 << 20) + 7]


def _single(st, torch, data, T, dst_size):
    src = torch.from_numpy(data).cuda() if data.nbytes else torch.empty(0, dtype=torch.uint8, device="cuda")
    dst = torch.zeros(dst_size, dtype=torch.uint8, device="cuda")
    r = st.lib.stenos_hip_compress(st.ctx, src.data_ptr(), T, data.nbytes, dst.data_ptr(), dst_size, st._stream_ptr())
    return r, (dst[:r].cpu().numpy() if r < ERR_BASE else None)


@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("T", [2, 3, 4, 8, 12, 64])
def test_frames_equal_oracle_and_single_call(oracle, level, T):
    torch = _cuda()
    st = Stenos(level=level)
    try:
        sizes = [s for s in _sizes(T, _sb(T)) if s >= 0]
        datas = [_data(KINDS[k % len(KINDS)], T, s, 100 + k) for k, s in enumerate(sizes)]
        srcs = [torch.from_numpy(d).cuda() if d.nbytes else torch.empty(0, dtype=torch.uint8, device="cuda") for d in datas]
        dsts = [torch.zeros(max(st.bound(d.nbytes), 16), dtype=torch.uint8, device="cuda") for d in datas]
        res = st.compress_batch(srcs, T, dsts)
        for k, d in enumerate(datas):
            r, ref = oracle_compress(oracle, d, T, level)
            assert res[k] == r, (T, level, sizes[k], hex(res[k]), r)
            got = dsts[k][: res[k]].cpu().numpy()
            assert np.array_equal(got, ref), (T, level, sizes[k])
            r1, f1 = _single(st, torch, d, T, dsts[k].numel())
            assert r1 == res[k] and np.array_equal(f1, got), (T, level, sizes[k])
    finally:
        st.close()


@pytest.mark.parametrize("T", [2, 4, 8])
def test_custom_block_shift_equals_single_call(T):
    torch = _cuda()
    st = Stenos(level=1)
    try:
        assert st.lib.stenos_set_block_size(st.ctx, 2) == 0
        sb = _sb(T, 2)
        sizes = _sizes(T, sb)
        datas = [_data(KINDS[k % len(KINDS)], T, s, 7 + k) for k, s in enumerate(sizes)]
        srcs = [torch.from_numpy(d).cuda() if d.nbytes else torch.empty(0, dtype=torch.uint8, device="cuda") for d in datas]
        # (small custom superblocks: a frame of copies outgrows stenos_bound, 4 header bytes per superblock)
        dsts = [torch.zeros(st.bound(d.nbytes) + 4 * (d.nbytes // sb + 2) + 16, dtype=torch.uint8, device="cuda") for d in datas]
        res = st.compress_batch(srcs, T, dsts)
        for k, d in enumerate(datas):
            r1, f1 = _single(st, torch, d, T, dsts[k].numel())
            assert r1 < ERR_BASE, (T, sizes[k], hex(r1))
            assert res[k] == r1, (T, sizes[k], hex(res[k]), hex(r1))
            assert np.array_equal(dsts[k][: res[k]].cpu().numpy(), f1), (T, sizes[k])
            if d.nbytes:
                assert f1[0] == 255
    finally:
        st.close()


@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("T,kind", [(4, "rand12"), (2, "walk"), (8, "sine"), (4, "rand")])
def test_tight_destinations(oracle, level, T, kind):
    """dst_size from the bound down to below the frame size, every item in one shared buffer with sentinel bytes between items."""
    torch = _cuda()
    st = Stenos(level=level)
    try:
        sb = _sb(T)
        items = []
        for k, n in enumerate([sb + 100, 2 * sb + 300, 3 * sb + 5, 5000 * T]):
            d = _data(kind, T, n, 31 + k)
            r, _ = oracle_compress(oracle, d, T, level)
            bound = st.bound(n)
            for cap in sorted({bound, r + 3, r + 1, r, r - 1, r - 5, max(r - 200, 9), (r + 8) // 2, 8, 7}):
                items.append((d, cap))
        GAP = 64
        offs, pos = [], 0
        for d, cap in items:
            offs.append(pos)
            pos += cap + GAP
        buf = torch.full((pos,), 0xA5, dtype=torch.uint8, device="cuda")
        srcs = [torch.from_numpy(d).cuda() for d, _ in items]
        dsts = [buf[o : o + cap] for o, (_, cap) in zip(offs, items)]
        res = st.compress_batch(srcs, T, dsts)
        host = buf.cpu().numpy()
        for k, (d, cap) in enumerate(items):
            r, ref = oracle_compress(oracle, d, T, level, cap)
            assert res[k] == r, (k, cap, hex(res[k]), hex(r))
            if r < ERR_BASE:
                assert np.array_equal(host[offs[k] : offs[k] + r], ref), (k, cap)
            assert (host[offs[k] + cap : offs[k] + cap + GAP] == 0xA5).all(), (k, cap)
    finally:
        st.close()


def test_round_trip_4096_items():
    torch = _cuda()
    st = Stenos(level=1)
    try:
        rng = np.random.default_rng(4096)
        T = 4
        sizes = [int(x) for x in rng.integers(1, 256 << 10, size=4096)]
        kinds = [KINDS[int(x)] for x in rng.integers(0, len(KINDS), size=4096)]
        total = sum(sizes)
        flat = torch.empty(total, dtype=torch.uint8, device="cuda")
        offs = np.concatenate([[0], np.cumsum(sizes)])
        for k in range(0, 4096, 512):  # (a few distinct payloads, tiled)
            d = _data(kinds[k], T, 256 << 10, k)
            for i in range(k, min(k + 512, 4096)):
                flat[offs[i] : offs[i + 1]] = torch.from_numpy(d[: sizes[i]]).cuda()
        srcs = [flat[offs[i] : offs[i + 1]] for i in range(4096)]
        frames = [torch.empty(st.bound(s), dtype=torch.uint8, device="cuda") for s in sizes]
        res = st.compress_batch(srcs, T, frames)
        assert all(r < ERR_BASE for r in res)
        back = torch.zeros(total, dtype=torch.uint8, device="cuda")
        outs = [back[offs[i] : offs[i + 1]] for i in range(4096)]
        got = st.decompress_batch(frames, T, res, outs)
        assert got == sizes
        assert torch.equal(back, flat)
        for i in (0, 1, 17, 1000, 4095):
            r1, f1 = _single(st, torch, srcs[i].cpu().numpy(), T, frames[i].numel())
            assert r1 == res[i] and np.array_equal(frames[i][:r1].cpu().numpy(), f1), i
            one = torch.zeros(sizes[i], dtype=torch.uint8, device="cuda")
            assert st.decompress(frames[i], T, res[i], one) == sizes[i]
    finally:
        st.close()


def _level_cases():
    with open(os.path.join(HERE, "golden", "level_frames.json")) as f:
        cases = json.load(f)["cases"]
    by_t = {}
    for e in cases:
        by_t.setdefault(e["T"], []).append(e)
    return by_t


def _input(e):
    if "input_b64" in e:
        return np.frombuffer(base64.b64decode(e["input_b64"]), dtype=np.uint8).copy()
    return generate(e["kind"], e["T"], e["n"], 42)


@pytest.mark.parametrize("T", [1, 2, 3, 4, 8])
def test_decode_mixed_batches(T):
    """reference frames with host codes, level-0 frames (one long enough for the parallel chain walk), a truncated frame, a bad
    shift byte, a destination too small"""
    torch = _cuda()
    cases = _level_cases().get(T, [])
    st = Stenos(level=0)
    try:
        frames, csizes, dsts, want = [], [], [], []
        for e in cases:
            fr = np.frombuffer(base64.b64decode(e["frame_b64"]), dtype=np.uint8).copy()
            frames.append(torch.from_numpy(fr).cuda())
            csizes.append(fr.nbytes)
            dsts.append(torch.zeros(_input(e).nbytes, dtype=torch.uint8, device="cuda"))
            want.append(_input(e))
        for k, n in enumerate([300 * _sb(T) + 5, 1000 * T + 3, 3 * _sb(T) + 11]):  # (300 superblocks: the parallel walk, batch_host.cpp)
            d = _data("walk", T, n, 5 + k)
            f = torch.empty(st.bound(n), dtype=torch.uint8, device="cuda")
            r = st.compress(torch.from_numpy(d).cuda(), T, f)
            frames.append(f)
            csizes.append(r)
            dsts.append(torch.zeros(n, dtype=torch.uint8, device="cuda"))
            want.append(d)
        good = len(frames)
        base = frames[-1]
        bad = [base[: csizes[-1] - 7].clone(), base[: csizes[-1]].clone(), base[: csizes[-1]].clone()]
        bad[1][0] = 9  # shift byte
        frames += bad
        csizes += [csizes[-1] - 7, csizes[-1], csizes[-1]]
        dsts += [torch.zeros(want[-1].nbytes, dtype=torch.uint8, device="cuda"), torch.zeros(want[-1].nbytes, dtype=torch.uint8, device="cuda"),
                 torch.zeros(want[-1].nbytes - 1, dtype=torch.uint8, device="cuda")]
        res = st.decompress_batch(frames, T, csizes, dsts)
        for k in range(good):
            assert res[k] == want[k].nbytes, (k, hex(res[k]))
            assert np.array_equal(dsts[k].cpu().numpy(), want[k]), k
        for k in range(good, len(frames)):
            single = st.lib.stenos_hip_decompress(st.ctx, frames[k].data_ptr(), T, csizes[k], dsts[k].data_ptr(), dsts[k].numel(), None, st._stream_ptr())
            assert res[k] == single and res[k] >= ERR_BASE, (k, hex(res[k]), hex(single))
        assert res[good:] == [SRC_OVERFLOW, INVALID_INPUT, DST_OVERFLOW]
    finally:
        st.close()


def test_refusals_write_nothing():
    torch = _cuda()
    src = torch.from_numpy(_data("rand12", 4, 100_000, 3)).cuda()
    for level, T, setup in ((2, 4, None), (1, 1, None), (1, 65, None), (1, 4, "time"), (1, 4, "async"), (0, 0, None)):
        st = Stenos(level=level)
        try:
            pending = None
            if setup == "time":
                st.lib.stenos_set_max_nanoseconds(st.ctx, 10**9)
            if setup == "async":
                pending = torch.zeros(st.bound(src.numel()), dtype=torch.uint8, device="cuda")
                st.compress(src, 4, pending, wait=False)
            dst = torch.full((st.bound(src.numel()),), 0x3C, dtype=torch.uint8, device="cuda")
            with pytest.raises(StenosError) as ei:
                st.compress_batch([src], T, [dst])
            assert ei.value.code == INVALID_PARAMETER, (level, T, setup)
            with pytest.raises(StenosError) as ei:  # (decompression: any level, bytesoftype 1 included -- refused for 65 or a pending job)
                st.decompress_batch([dst], 4 if setup == "async" else 65, [100], [dst])
            assert ei.value.code == INVALID_PARAMETER, (level, T, setup)
            assert (dst.cpu().numpy() == 0x3C).all(), (level, T, setup)
            if pending is not None:  # the pending job is left alone
                r = st.finish()
                back = torch.zeros_like(src)
                assert st.decompress(pending, 4, r, back) == src.numel() and torch.equal(back, src)
        finally:
            st.close()


def test_batch_of_one_and_of_none():
    torch = _cuda()
    st = Stenos(level=1)
    try:
        d = _data("walk", 2, 300_001, 8)
        src = torch.from_numpy(d).cuda()
        dst = torch.zeros(st.bound(d.nbytes), dtype=torch.uint8, device="cuda")
        (r,) = st.compress_batch([src], 2, [dst])
        r1, f1 = _single(st, torch, d, 2, dst.numel())
        assert r == r1 and np.array_equal(dst[:r].cpu().numpy(), f1)
        assert st.compress_batch([], 2, []) == [] and st.decompress_batch([], 2, [], []) == []
    finally:
        st.close()


def test_context_reuse_and_last_index():
    torch = _cuda()
    st = Stenos(level=1)
    try:
        d = _data("rand12", 4, 1 << 20, 4)
        src = torch.from_numpy(d).cuda()
        a = torch.zeros(st.bound(d.nbytes), dtype=torch.uint8, device="cuda")
        ra = st.compress(src, 4, a)
        p, nsb = st.last_index()
        assert p and nsb == 8
        b = torch.zeros_like(a)
        (rb,) = st.compress_batch([src], 4, [b])
        assert rb == ra and torch.equal(a[:ra], b[:rb])
        assert st.last_index() == (None, 0)
        c = torch.zeros_like(a)
        assert st.compress(src, 4, c) == ra and torch.equal(a[:ra], c[:ra])
        p, nsb = st.last_index()
        assert p and nsb == 8
        back = torch.zeros_like(src)
        assert st.decompress(c, 4, ra, back, index_ptr=p) == d.nbytes and torch.equal(back, src)
        # a decompression batch overwrites the index workspace too
        back.zero_()
        assert st.decompress_batch([c], 4, [ra], [back]) == [d.nbytes] and torch.equal(back, src)
        assert st.last_index() == (None, 0)
        # ... and a host-pointer compression after a batch leaves its index again
        host = np.zeros(st.bound(d.nbytes), dtype=np.uint8)
        assert st.lib.stenos_compress_generic(st.ctx, d.ctypes.data, 4, d.nbytes, host.ctypes.data, host.nbytes) == ra
        p, nsb = st.last_index()
        assert p and nsb == 8
    finally:
        st.close()


def test_non_default_stream():
    """The sources (then the frames) are written on a side stream behind a few milliseconds of other work there; only work
    ordered on that stream sees them."""
    torch = _cuda()
    st = Stenos(level=1)
    try:
        s = torch.cuda.Stream()
        datas = [_data("sine", 8, n, 12 + n % 7) for n in (70_000, 300_008, 5)]
        ready = [torch.from_numpy(d).cuda() for d in datas]
        srcs = [torch.zeros_like(r) for r in ready]
        dsts = [torch.zeros(st.bound(d.nbytes), dtype=torch.uint8, device="cuda") for d in datas]
        frames = [torch.zeros_like(t) for t in dsts]
        outs = [torch.zeros(d.nbytes, dtype=torch.uint8, device="cuda") for d in datas]
        busy = torch.zeros(64 << 20, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            for _ in range(200):
                busy.add_(1.0)
            for a, b in zip(srcs, ready):
                a.copy_(b)
            res = st.compress_batch(srcs, 8, dsts)
            for _ in range(200):
                busy.add_(1.0)
            for a, b in zip(frames, dsts):
                a.copy_(b)
            got = st.decompress_batch(frames, 8, res, outs)
        torch.cuda.synchronize()
        assert got == [d.nbytes for d in datas]
        for d, o in zip(datas, outs):
            assert np.array_equal(o.cpu().numpy(), d)
    finally:
        st.close()


def test_pending_async_job_is_tracked_by_the_calls_that_set_it():
    """A synchronous call that fails before it starts a job leaves the pending asynchronous one pending (a batch still refuses);
    an asynchronous call that fails before it starts one leaves none (a batch runs)."""
    torch = _cuda()
    st = Stenos(level=1)
    try:
        d = _data("walk", 2, 200_001, 6)
        src = torch.from_numpy(d).cuda()
        pending = torch.zeros(st.bound(d.nbytes), dtype=torch.uint8, device="cuda")
        other = torch.zeros_like(pending)
        st.compress(src, 2, pending, wait=False)
        r = st.lib.stenos_hip_compress(st.ctx, src.data_ptr(), 0, d.nbytes, other.data_ptr(), other.numel(), st._stream_ptr())
        assert r >= ERR_BASE  # (bytesoftype 0)
        with pytest.raises(StenosError) as ei:
            st.compress_batch([src], 2, [other])
        assert ei.value.code == INVALID_PARAMETER
        csize = st.finish()
        r1, f1 = _single(st, torch, d, 2, pending.numel())
        assert csize == r1 and np.array_equal(pending[:csize].cpu().numpy(), f1)
        r = st.lib.stenos_hip_compress_async(st.ctx, src.data_ptr(), 0, d.nbytes, other.data_ptr(), other.numel(), st._stream_ptr())
        assert r >= ERR_BASE
        assert st.compress_batch([src], 2, [other]) == [csize]
    finally:
        st.close()
