"""Rows of many frames on the device by device-resident (frame number, row number) pairs (include/stenos_hip.h:
stenos_hip_gather_rows_batch, stenos_hip_frames_index): every slot equals the row of its frame's array and what
stenos_hip_gather_rows delivers for that frame, whatever the frames' sizes and superblock sizes, the index form, the alignment and
the stride of the slots; nothing is written outside the slots; an invalid pair leaves its slot alone and fails the call; the
index of stenos_hip_frames_index survives any number of calls and is the single frames' indices one after the other; refusals
write nothing; damage is seen where a row looks and nowhere else; pairs computed on the stream of the call need no synchronisation.

The slot buffer is pre-filled with 0xA5 and compared whole against a numpy image, so the gaps and both ends are checked."""
import ctypes

import numpy as np
import pytest

from stenos_amd.api import Stenos, StenosError
from test_gpu_gather import GUARD_BYTE, INVALID_INPUT, INVALID_PARAMETER, SRC_OVERFLOW, TS, Slots, _code, _row_sizes, _rows_tensor
from test_gpu_ranges import _data, _mixed_data, _sb, _sizes

pytestmark = pytest.mark.gpu

SHIFT = 2  # the small custom superblock: four blocks


def _cuda():
    import torch

    assert torch.cuda.is_available()
    return torch


def _device_words(ptr, count):
    torch = _cuda()
    host = torch.empty(count, dtype=torch.int64)
    hip = ctypes.CDLL("libamdhip64.so")
    assert hip.hipMemcpy(ctypes.c_void_p(host.data_ptr()), ctypes.c_void_p(ptr), ctypes.c_size_t(count * 8), 2) == 0
    return host.tolist()


class Batch:
    """m frames on the device with their arrays on the host: .frames, .csizes, .datas, .sbs"""

    def __init__(self):
        self.frames, self.csizes, self.datas, self.sbs = [], [], [], []

    def add(self, frame, csize, data, sb):
        self.frames.append(frame)
        self.csizes.append(int(csize))
        self.datas.append(np.ascontiguousarray(data).view(np.uint8).ravel())
        self.sbs.append(sb)

    def add_single(self, st, torch, T, data, sb):
        frame = torch.zeros(st.bound(data.nbytes) + 8 * (data.nbytes // sb + 2), dtype=torch.uint8, device="cuda")
        self.add(frame, st.compress(torch.from_numpy(data).cuda(), T, frame), data, sb)

    def add_batch(self, st, torch, T, datas, sb):
        srcs = [torch.from_numpy(d).cuda() for d in datas]
        dsts = [torch.zeros(st.bound(d.nbytes) + 8 * (d.nbytes // sb + 2), dtype=torch.uint8, device="cuda") for d in datas]
        res = st.compress_batch(srcs, T, dsts)
        for d, dst, r in zip(datas, dsts, res):
            assert r < (1 << 63), r
            self.add(dst, r, d, sb)

    def add_empty(self, torch):
        self.add(torch.zeros(8, dtype=torch.uint8, device="cuda"), 8, np.zeros(0, dtype=np.uint8), 1)  # [shift 0][0 bytes]

    @property
    def m(self):
        return len(self.frames)

    def image(self, sl, fids, rows, skip=()):
        """the numpy image of the slot buffer after a call with these pairs"""
        want = np.full(sl.buf.numel(), GUARD_BYTE, dtype=np.uint8)
        keep = np.array([i for i in range(len(rows)) if i not in skip], dtype=np.int64) if skip else np.arange(len(rows), dtype=np.int64)
        if keep.size:
            cat = np.concatenate(self.datas)
            base = np.cumsum([0] + [d.size for d in self.datas])[:-1]
            f = np.asarray(fids, dtype=np.int64)[keep]
            r = np.asarray(rows, dtype=np.int64)[keep]
            col = np.arange(sl.row_bytes, dtype=np.int64)
            want[(sl.at + keep * sl.stride)[:, None] + col] = cat[(base[f] + r * sl.row_bytes)[:, None] + col]
        return want

    def check(self, sl, fids, rows, skip=()):
        got, want = sl.buf.cpu().numpy(), self.image(sl, fids, rows, skip)
        if not np.array_equal(got, want):
            bad = int(np.flatnonzero(got != want)[0])
            i = (bad - sl.at) // sl.stride
            raise AssertionError(f"byte {bad} of the buffer differs (got {got[bad]}, want {want[bad]}): slot {i}, pair "
                                 f"{(fids[i], rows[i]) if 0 <= i < len(rows) else None}, row_bytes {sl.row_bytes}, stride {sl.stride}")

    def gather(self, st, torch, T, row_bytes, fids, rows, index_ptr=None, stride=None, mis=0, unsigned=False):
        sl = Slots(torch, len(rows), row_bytes, stride, mis)
        got = st.gather_rows_batch(self.frames, T, self.csizes, row_bytes, _rows_tensor(torch, fids, unsigned), _rows_tensor(torch, rows, unsigned), sl.ptr, index_ptr, stride)
        assert got == len(rows) * row_bytes
        self.check(sl, fids, rows)
        return sl


def make_batch(torch, T, seed=0):
    """eight frames, both superblock sizes, made partly by compress_batch and partly by single calls: copies and mini-LZ blocks
    (_mixed_data), a last superblock under 128 bytes (zstd-coded: the host path), one-superblock frames, an empty array"""
    a, b = _sb(T), _sb(T, SHIFT)
    st, st2 = Stenos(level=1), Stenos(level=1)
    try:
        assert st2.lib.stenos_set_block_size(st2.ctx, SHIFT) == 0
        sa, sbb = _sizes(T, a), _sizes(T, b)
        bt = Batch()
        bt.add_single(st, torch, T, _mixed_data(T, sa[1], a, seed + 1), a)                                               # 0: 2 sb + 300
        bt.add_batch(st2, torch, T, [_mixed_data(T, sbb[3], b, seed + 2), _mixed_data(T, sbb[0], b, seed + 3)], b)      # 1: 3 sb + ..., 2: one superblock
        bt.add_empty(torch)                                                                                             # 3
        bt.add_batch(st, torch, T, [_mixed_data(T, sa[2], a, seed + 4), _mixed_data(T, sa[3], a, seed + 5), _mixed_data(T, sa[0], a, seed + 6)], a)  # 4: tiny last, 5: 4 sb, 6: one
        bt.add_single(st2, torch, T, _mixed_data(T, sbb[4], b, seed + 7), b)                                            # 7: 2 sb exactly
        return bt
    finally:
        st.close()
        st2.close()


def pair_set(bt, row_bytes, rng):
    """every valid (frame, row) pair in one random permutation across the frames, duplicates, and exactly 64 and 65 rows of one
    interior superblock of a middle frame (frame 5, superblock 1)"""
    fids = np.concatenate([np.full(d.size // row_bytes, f, dtype=np.int64) for f, d in enumerate(bt.datas)])
    rows = np.concatenate([np.arange(d.size // row_bytes, dtype=np.int64) for d in bt.datas])
    order = rng.permutation(rows.size)
    fids, rows = fids[order], rows[order]
    sb = bt.sbs[5]
    if sb // row_bytes >= 66:
        first = -(-sb // row_bytes)
        assert (first + 65) * row_bytes <= 2 * sb < bt.datas[5].size
        fids = np.concatenate([fids, np.full(129, 5, dtype=np.int64)])
        rows = np.concatenate([rows, np.arange(first, first + 64), np.arange(first + 64, first - 1, -1)])
    dup = np.array([0, rows.size // 2, 0])
    return np.concatenate([fids, fids[dup]]), np.concatenate([rows, rows[dup]])


@pytest.mark.parametrize("T", TS)
def test_parity(T):
    torch = _cuda()
    bt = make_batch(torch, T)
    st = Stenos(level=1)
    try:
        rng = np.random.default_rng([71, T])
        for row_bytes in _row_sizes(T, _sb(T), max(d.size for d in bt.datas)):
            fids, rows = pair_set(bt, row_bytes, rng)
            assert np.unique(fids).size >= 2
            sl = bt.gather(st, torch, T, row_bytes, fids, rows)
            bt.gather(st, torch, T, row_bytes, fids, rows, None, row_bytes + 67, 5, unsigned=True)
            # ... and what stenos_hip_gather_rows gives, frame by frame
            got = sl.buf[sl.at:sl.at + len(rows) * row_bytes].cpu().numpy().reshape(len(rows), row_bytes)
            fa, ra = np.asarray(fids), np.asarray(rows)
            for f in range(bt.m):
                mine = np.flatnonzero(fa == f)
                if mine.size == 0:
                    continue
                out = torch.zeros(mine.size * row_bytes, dtype=torch.uint8, device="cuda")
                assert st.gather_rows(bt.frames[f], T, bt.csizes[f], row_bytes, _rows_tensor(torch, ra[mine]), out) == mine.size * row_bytes
                assert np.array_equal(out.cpu().numpy().reshape(mine.size, row_bytes), got[mine]), (row_bytes, f)
    finally:
        st.close()


def test_one_frame_is_the_single_call():
    torch = _cuda()
    st = Stenos(level=1)
    try:
        T, sb = 4, _sb(4)
        bt = Batch()
        bt.add_single(st, torch, T, _mixed_data(T, 3 * sb + 777, sb, 3), sb)
        rng = np.random.default_rng(72)
        for row_bytes, stride, mis in ((300, None, 0), (7, 7 + 67, 5), (sb + 5, None, 0)):
            nrows = bt.datas[0].size // row_bytes
            rows = [int(r) for r in rng.integers(0, nrows, 500)] + [0, nrows - 1]
            sl = bt.gather(st, torch, T, row_bytes, [0] * len(rows), rows, None, stride, mis)
            single = Slots(torch, len(rows), row_bytes, stride, mis)
            assert st.gather_rows(bt.frames[0], T, bt.csizes[0], row_bytes, _rows_tensor(torch, rows), single.ptr, None, stride) == len(rows) * row_bytes
            assert torch.equal(sl.buf, single.buf)
    finally:
        st.close()


def test_the_same_frame_listed_twice():
    torch = _cuda()
    st = Stenos(level=1)
    try:
        T, sb = 8, _sb(8)
        bt = Batch()
        bt.add_single(st, torch, T, _mixed_data(T, 2 * sb + 300, sb, 5), sb)
        bt.add_single(st, torch, T, _data("walk", T, sb + 99, 6), sb)
        bt.add(bt.frames[0], bt.csizes[0], bt.datas[0], sb)
        rng = np.random.default_rng(73)
        nrows = [d.size // 300 for d in bt.datas]
        fids = [int(f) for f in rng.integers(0, 3, 900)]
        rows = [int(rng.integers(0, nrows[f])) for f in fids]
        assert {0, 2} <= set(fids)
        bt.gather(st, torch, T, 300, fids, rows, None, 300 + 67, 5)
        p, entries = st.frames_index(bt.frames, T, bt.csizes)
        bt.gather(st, torch, T, 300, fids, rows, p)
    finally:
        st.close()


def test_index_forms():
    """no index; the index of stenos_hip_frames_index for three calls, its bytes unchanged afterwards and equal to the frames' own
    indices one after the other; a level-2 frame in the batch goes the host path"""
    torch = _cuda()
    bt = make_batch(torch, 4, seed=10)
    st, hi = Stenos(level=1), Stenos(level=2)
    try:
        T, sb = 4, _sb(4)
        data = _mixed_data(T, 2 * sb + 4000 + 3, sb, 2)
        bt.add_single(hi, torch, T, data, sb)
        assert bt.m == 9
        # (a second context makes the single frames' indices: the first one's index buffer is what is under test)
        singles = [hi.frame_index(f, T, c) if d.size else [8] for f, c, d in zip(bt.frames, bt.csizes, bt.datas)]
        rng = np.random.default_rng(74)
        fids, rows = pair_set(bt, 300, rng)
        assert 8 in fids
        bt.gather(st, torch, T, 300, fids, rows)
        p, entries = st.frames_index(bt.frames, T, bt.csizes)
        assert entries == sum(len(s) for s in singles)
        before = _device_words(p, entries)
        assert before == [x for s in singles for x in s]
        outs = [bt.gather(st, torch, T, 300, fids, rows, p, 300 + 67, 5).buf.cpu().numpy() for _ in range(3)]
        assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])
        bt.gather(st, torch, T, sb + 5, *pair_set(bt, sb + 5, rng), p)
        assert _device_words(p, entries) == before
        # only the level-2 frame and the last superblock under 128 bytes: everything is finished on the host
        few = [(8, 0), (4, bt.datas[4].size // 50 - 1), (8, bt.datas[8].size // 50 - 1), (8, sb // 50)]
        bt.gather(st, torch, T, 50, [f for f, _ in few], [r for _, r in few], p, 64, 3)
    finally:
        st.close()
        hi.close()


def test_long_chains_through_the_shared_front_end(hooks_lib):
    """Frames of exactly 256 and 257 superblocks -- the two sides of kBatchSerialWalkMax (csrc/frame_access.h): the first is walked
    by the serial batched walk, the second by a parallel walk of its own --, one of 3 superblocks and a few bytes, and an empty
    array, through the three calls that share the front end of csrc/frame_batch.h: the index of stenos_hip_frames_index is the
    frames' own indices one after the other, stenos_hip_gather_rows_batch delivers the rows with and without it, and
    stenos_hip_decompress_batch returns the arrays.  Then all of it again with every chain walked by one lane (the test build's
    stenos_hip_test_walk): the same index words.  Level 0 and the small superblock: every superblock is a copy."""
    torch = _cuda()
    T, rb = 4, 100  # (rows of 100 bytes straddle the superblocks' boundaries)
    sb = _sb(T, SHIFT)
    make, st, other = Stenos(0, lib=hooks_lib), Stenos(1, lib=hooks_lib), Stenos(1, lib=hooks_lib)
    try:
        assert make.lib.stenos_set_block_size(make.ctx, SHIFT) == 0
        rng = np.random.default_rng(77)
        bt = Batch()
        for nbytes in (256 * sb, 257 * sb, 3 * sb + 20):
            bt.add_single(make, torch, T, rng.integers(0, 256, nbytes, dtype=np.uint8), sb)
        bt.add_empty(torch)
        # (a second context makes the single frames' indices: the first one's index buffer is what is under test)
        singles = [other.frame_index(f, T, c) if d.size else [8] for f, c, d in zip(bt.frames, bt.csizes, bt.datas)]
        assert [len(s) - 1 for s in singles] == [256, 257, 4, 0]
        nrows = [d.size // rb for d in bt.datas]
        # the first and last row of every frame that has rows; in the long frame the rows of superblocks 255 and 256 and the one
        # that straddles their boundary; random ones
        pairs = [(f, r) for f in range(3) for r in (0, nrows[f] - 1)]
        pairs += [(1, r) for r in (255 * sb // rb + 1, 256 * sb // rb, 256 * sb // rb + 1, 257 * sb // rb - 1)]
        assert (256 * sb) % rb and (256 * sb // rb + 1) * rb <= 257 * sb
        pairs += [(int(f), int(rng.integers(0, nrows[f]))) for f in rng.integers(0, 3, 300)]
        fids, rows = [f for f, _ in pairs], [r for _, r in pairs]
        words = []
        for serial in (False, True):
            assert st.lib.stenos_hip_test_walk(st.ctx, 1 if serial else 0) in (-1, 0)
            p, entries = st.frames_index(bt.frames, T, bt.csizes)
            assert entries == sum(len(s) for s in singles)
            words.append(_device_words(p, entries))
            assert words[-1] == [x for s in singles for x in s], serial
            bt.gather(st, torch, T, rb, fids, rows)  # (walks the chains itself)
            p, entries = st.frames_index(bt.frames, T, bt.csizes)
            bt.gather(st, torch, T, rb, fids, rows, p, rb + 67, 5)
            assert _device_words(p, entries) == words[-1]
            dsts = [torch.full((max(d.size, 8),), GUARD_BYTE, dtype=torch.uint8, device="cuda") for d in bt.datas]
            assert st.decompress_batch(bt.frames, T, bt.csizes, dsts) == [d.size for d in bt.datas]
            for d, dst in zip(bt.datas, dsts):
                assert np.array_equal(dst[:d.size].cpu().numpy(), d) and (dst[d.size:] == GUARD_BYTE).all().item()
            if not serial:  # (the flag the last parallel walk left: it did not fall back to one lane)
                assert st.lib.stenos_hip_test_walk(st.ctx, 0) == 0
        assert words[0] == words[1]
    finally:
        st.lib.stenos_hip_test_walk(st.ctx, 0)
        for s in (make, st, other):
            s.close()


def test_invalid_pairs():
    """a frame number equal to m, one of 2^63, and the row the small frame refuses though a larger frame of the batch accepts it:
    INVALID_PARAMETER, that slot untouched, every gap intact; without the pair the call is correct"""
    torch = _cuda()
    bt = make_batch(torch, 4, seed=20)
    st = Stenos(level=1)
    try:
        T, row_bytes = 4, 300
        small = bt.datas[2].size // row_bytes
        assert small < bt.datas[5].size // row_bytes
        rng = np.random.default_rng(75)
        gf, gr = pair_set(bt, row_bytes, rng)
        gf, gr = gf[:400].tolist(), gr[:400].tolist()
        for index in (None, "given"):
            p = st.frames_index(bt.frames, T, bt.csizes)[0] if index else None
            for bad in ((bt.m, 0), (1 << 63, 0), (2, small), (3, 0)):
                fids, rows = gf[:57] + [bad[0]] + gf[57:], gr[:57] + [bad[1]] + gr[57:]
                for unsigned in (False, True):
                    sl = Slots(torch, len(rows), row_bytes, row_bytes + 67, 5)
                    call = lambda: st.gather_rows_batch(bt.frames, T, bt.csizes, row_bytes, _rows_tensor(torch, fids, unsigned), _rows_tensor(torch, rows, unsigned),  # noqa: E731
                                                        sl.ptr, p, row_bytes + 67)
                    assert _code(call) == INVALID_PARAMETER, bad
                    assert sl.gaps_intact()
                    at = sl.at + 57 * sl.stride
                    assert (sl.buf[at:at + row_bytes] == GUARD_BYTE).all().item(), bad
            bt.gather(st, torch, T, row_bytes, gf, gr, p, row_bytes + 67, 5)
        # a batch of empty arrays only: every pair is invalid
        only = Batch()
        only.add_empty(torch)
        only.add_empty(torch)
        sl = Slots(torch, 2, 16)
        assert _code(lambda: st.gather_rows_batch(only.frames, T, only.csizes, 16, _rows_tensor(torch, [0, 1]), _rows_tensor(torch, [0, 0]), sl.ptr)) == INVALID_PARAMETER
        assert sl.untouched()
    finally:
        st.close()


def test_refusals_write_nothing():
    torch = _cuda()
    bt = make_batch(torch, 4, seed=30)
    st = Stenos(level=1)
    try:
        T = 4
        fids, rows = [0, 1, 5, 7], [0, 3, 9, 1]
        ft, rt = _rows_tensor(torch, fids), _rows_tensor(torch, rows)
        sl = Slots(torch, 4, 16, 32)
        P, Z = ctypes.c_void_p * bt.m, ctypes.c_size_t * bt.m
        ptrs, sizes = P(*[f.data_ptr() for f in bt.frames]), Z(*bt.csizes)
        call = lambda **kw: st.lib.stenos_hip_gather_rows_batch(st.ctx, kw.get("m", bt.m), kw.get("T", T), ptrs, sizes, kw.get("row_bytes", 16), kw.get("n", 4),  # noqa: E731
                                                                ft.data_ptr(), rt.data_ptr(), sl.ptr, kw.get("stride", 32), None, st._stream_ptr())
        for kw in (dict(m=0), dict(row_bytes=0), dict(stride=15), dict(T=0), dict(T=65), dict(row_bytes=1 << 62, stride=1 << 62), dict(n=1 << 60),
                   dict(n=1 << 40, stride=1 << 30), dict(n=1 << 31), dict(n=1 << 30, row_bytes=17, stride=17)):
            assert call(**kw) == INVALID_PARAMETER, kw
            assert sl.untouched(), kw
        assert st.gather_rows_batch(bt.frames, T, bt.csizes, 16, ft[:0], rt[:0], sl.ptr) == 0 and sl.untouched()
        # frame headers stenos_hip_decompress refuses: the code of the first such frame in order
        bad = bt.frames[1].clone()
        bad[0] = 77
        frames = list(bt.frames)
        frames[1] = bad
        csizes = list(bt.csizes)
        csizes[5] = 5
        gather = lambda fr, cs, index=None: _code(lambda: st.gather_rows_batch(fr, T, cs, 16, ft, rt, sl.ptr, index, 32))  # noqa: E731
        p = st.frames_index(bt.frames, T, bt.csizes)[0]
        for index in (p, None):
            assert gather(frames, csizes, index) == INVALID_INPUT and sl.untouched()
            assert gather(bt.frames, csizes, index) == SRC_OVERFLOW and sl.untouched()
            assert gather(frames, bt.csizes, index) == INVALID_INPUT and sl.untouched()
        with pytest.raises(StenosError):
            st.frames_index(frames, T, bt.csizes)
        # a pending _async job: refused, and the job is left alone
        src = torch.from_numpy(bt.datas[0]).cuda()
        other = torch.zeros(st.bound(src.numel()), dtype=torch.uint8, device="cuda")
        st.compress(src, T, other, wait=False)
        assert gather(bt.frames, bt.csizes) == INVALID_PARAMETER and sl.untouched()
        assert st.finish() > 0
        assert gather(bt.frames, bt.csizes) == 64
        bt.check(sl, fids, rows)
    finally:
        st.close()


def test_damage_is_seen_where_a_row_looks():
    """with a given index only (a walk would see the damage): a frame size cut inside a superblock gives SRC_OVERFLOW, an unknown
    superblock code INVALID_INPUT, both only when a row touches that superblock; rows elsewhere in the batch succeed"""
    torch = _cuda()
    bt = make_batch(torch, 4, seed=40)
    st, other = Stenos(level=1), Stenos(level=1)
    try:
        T, rb, sb = 4, 100, bt.sbs[5]
        offs = other.frame_index(bt.frames[5], T, bt.csizes[5])
        p = st.frames_index(bt.frames, T, bt.csizes)[0]
        rng = np.random.default_rng(76)
        fids, rows = pair_set(bt, rb, rng)
        elsewhere = [(f, r) for f, r in zip(fids, rows) if f != 5 or (r + 1) * rb <= sb or r * rb >= 2 * sb][:600]
        assert sum(f == 5 for f, _ in elsewhere) > 5
        touching = elsewhere[:50] + [(5, sb // rb + 3)] + elsewhere[50:]
        split = lambda pairs: ([f for f, _ in pairs], [r for _, r in pairs])  # noqa: E731

        def gather(frames, csizes, pairs):
            f, r = split(pairs)
            sl = Slots(torch, len(pairs), rb, rb + 9, 3)
            code = _code(lambda: st.gather_rows_batch(frames, T, csizes, rb, _rows_tensor(torch, f), _rows_tensor(torch, r), sl.ptr, p, rb + 9))
            return code, sl

        cut = list(bt.csizes)
        cut[5] = offs[1] + 4 + 10
        unknown = list(bt.frames)
        unknown[5] = bt.frames[5].clone()
        unknown[5][offs[1]] = 9
        for frames, csizes, want in ((bt.frames, cut, SRC_OVERFLOW), (unknown, bt.csizes, INVALID_INPUT)):
            code, sl = gather(frames, csizes, touching)
            assert code == want and sl.gaps_intact()
            if want == INVALID_INPUT:  # (the cut frame has lost the superblocks behind the cut as well)
                code, sl = gather(frames, csizes, elsewhere)
                assert code == len(elsewhere) * rb
                bt.check(sl, *split(elsewhere))
        before = [(f, r) for f, r in elsewhere if f != 5 or (r + 1) * rb <= sb]
        code, sl = gather(bt.frames, cut, before)
        assert code == len(before) * rb
        bt.check(sl, *split(before))
    finally:
        st.close()
        other.close()


def test_pairs_computed_on_a_side_stream():
    """the frame numbers and row numbers are computed by torch ops on a side stream behind a few milliseconds of other work there,
    directly before the call; nothing is synchronised"""
    torch = _cuda()
    bt = make_batch(torch, 8, seed=50)
    st = Stenos(level=1)
    try:
        T, rb = 8, 256
        nrows = torch.tensor([d.size // rb for d in bt.datas], dtype=torch.int64, device="cuda")
        live = torch.tensor([f for f, d in enumerate(bt.datas) if d.size >= rb], dtype=torch.int64, device="cuda")
        n = 5000
        sl = Slots(torch, n, rb, rb + 67, 5)
        busy = torch.zeros(64 << 20, dtype=torch.float32, device="cuda")
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            for _ in range(200):
                busy.add_(1.0)
            k = torch.randperm(n, device="cuda")
            fids = live[(k * 7 + 3) % live.numel()]
            rows = (k * 13 + 5) % nrows[fids]
            got = st.gather_rows_batch(bt.frames, T, bt.csizes, rb, fids, rows, sl.ptr, None, rb + 67)
        torch.cuda.synchronize()
        assert got == n * rb
        bt.check(sl, fids.cpu().tolist(), rows.cpu().tolist())
    finally:
        st.close()
