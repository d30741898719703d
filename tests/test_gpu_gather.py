"""Rows of a frame on the device by device-resident row numbers (include/stenos_hip.h: stenos_hip_gather_rows): every slot equals
the row of stenos_hip_decompress's output and the bytes stenos_hip_decompress_ranges delivers for the same ranges, whatever the
superblock codes, the index form, the alignment and the stride of the slots; nothing is written outside the slots -- not between
them either --, on success or on any error; an invalid row number leaves its slot alone and fails the call; the caller's index
survives any number of calls; the refusals happen before anything is written; damage is seen where a row looks and nowhere else;
row numbers computed on the stream of the call need no synchronisation.

The slot buffer is pre-filled with 0xA5 and compared whole against a numpy image, so the gaps and both ends are checked."""
import base64
import ctypes
import json
import os

import numpy as np
import pytest

import streamgen as sg
from stenos_amd.api import Stenos, StenosError
from stenos_amd.datagen import generate
from test_gpu_ranges import _data, _mixed_data, _sb, _sizes, _walk_frame

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


class Slots:
    """n slots of row_bytes every `stride` bytes, the first one `mis` bytes behind a 256-byte boundary, 64 guard bytes in front
    and behind; the whole buffer is 0xA5 before the call"""

    def __init__(self, torch, n, row_bytes, stride=None, mis=0):
        self.n, self.row_bytes, self.stride = n, row_bytes, stride or row_bytes
        self.at = 256 + mis
        span = (n - 1) * self.stride + row_bytes if n else 0
        self.buf = torch.full((self.at + span + GUARD + 16,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 256 == 0
        self.ptr = self.buf.data_ptr() + self.at

    def expected(self, full, rows, skip=()):
        want = np.full(self.buf.numel(), GUARD_BYTE, dtype=np.uint8)
        keep = np.array([i for i in range(len(rows)) if i not in skip], dtype=np.int64)
        if keep.size:
            r = np.asarray(rows, dtype=np.uint64).astype(np.int64)[keep]
            col = np.arange(self.row_bytes, dtype=np.int64)
            want[(self.at + keep * self.stride)[:, None] + col] = full[(r * self.row_bytes)[:, None] + col]
        return want

    def check(self, full, rows, skip=()):
        got = self.buf.cpu().numpy()
        want = self.expected(full, rows, skip)
        if not np.array_equal(got, want):
            bad = int(np.flatnonzero(got != want)[0])
            i = (bad - self.at) // self.stride
            raise AssertionError(f"byte {bad} of the buffer differs (got {got[bad]}, want {want[bad]}): slot {i} at {self.at + i * self.stride}, "
                                 f"row {rows[i] if 0 <= i < len(rows) else None}, row_bytes {self.row_bytes}, stride {self.stride}")

    def gaps_intact(self):
        got = self.buf.cpu().numpy()
        mask = np.ones(got.size, dtype=bool)
        for i in range(self.n):
            mask[self.at + i * self.stride:self.at + i * self.stride + self.row_bytes] = False
        return bool((got[mask] == GUARD_BYTE).all())

    def untouched(self):
        return bool((self.buf == GUARD_BYTE).all().item())


def _rows_tensor(torch, rows, unsigned=False):
    a = np.asarray(rows, dtype=np.uint64)
    t = torch.from_numpy(a.view(np.int64)).cuda()
    return t.view(torch.uint64) if unsigned and hasattr(torch, "uint64") else t


def row_set(total, sb, row_bytes, rng):
    """every valid row in a random permutation (with short rows: more than 64 pieces per superblock, several chunks), exactly 64
    and 65 rows of one superblock, duplicates, the first and the last row"""
    nrows = total // row_bytes
    if nrows == 0:
        return []
    rows = [int(r) for r in rng.permutation(nrows)]
    per_sb = sb // row_bytes
    if per_sb >= 65:  # rows wholly inside the last whole superblock (or the first)
        s = max(0, total // sb - 1)
        first = -(-s * sb // row_bytes)
        if first + 65 <= nrows:
            rows += list(range(first, first + 64)) + list(range(first + 64, first - 1, -1))
    rows += [rows[0], rows[0], rows[len(rows) // 2], 0, nrows - 1, nrows - 1, 0]
    return rows


def _ranges_image(st, torch, frame, T, csize, rows, row_bytes, index_ptr=None):
    """the same rows through stenos_hip_decompress_ranges, one range per row, back to back"""
    out = torch.zeros(max(1, len(rows) * row_bytes), dtype=torch.uint8, device="cuda")
    ranges = [(r * row_bytes, row_bytes) for r in rows]
    assert st.decompress_ranges(frame, T, csize, ranges, [out.data_ptr() + i * row_bytes for i in range(len(rows))], index_ptr) == len(rows) * row_bytes
    return out.cpu().numpy()


def _gather_checked(st, torch, frame, T, csize, full, row_bytes, rows, index_ptr=None, stride=None, mis=0, unsigned=False):
    sl = Slots(torch, len(rows), row_bytes, stride, mis)
    assert st.gather_rows(frame, T, csize, row_bytes, _rows_tensor(torch, rows, unsigned), sl.ptr, index_ptr, stride) == len(rows) * row_bytes
    sl.check(full, rows)
    return sl


def _check_all_index_forms(st, torch, frame, T, csize, full, row_bytes, rows, last_index=None, against_ranges=True):
    """no index, the index of the compression (where there was one), the index of stenos_hip_frame_index; the aligned base with
    stride row_bytes and a base misaligned by 5 with stride row_bytes + 64 + 3 take turns, each form sees both"""
    wide = dict(stride=row_bytes + 64 + 3, mis=5)
    if last_index:  # (first: the calls that follow overwrite the context's index)
        _gather_checked(st, torch, frame, T, csize, full, row_bytes, rows, last_index)
        _gather_checked(st, torch, frame, T, csize, full, row_bytes, rows, last_index, **wide)
    sl = _gather_checked(st, torch, frame, T, csize, full, row_bytes, rows)
    _gather_checked(st, torch, frame, T, csize, full, row_bytes, rows, unsigned=True, **wide)
    n = ctypes.c_size_t(0)
    p = st.lib.stenos_hip_frame_index(st.ctx, frame.data_ptr(), T, csize, ctypes.byref(n), st._stream_ptr())
    assert p
    _gather_checked(st, torch, frame, T, csize, full, row_bytes, rows, p)
    _gather_checked(st, torch, frame, T, csize, full, row_bytes, rows, p, **wide)
    if against_ranges and rows:
        got = sl.buf[sl.at:sl.at + len(rows) * row_bytes].cpu().numpy()
        assert np.array_equal(got, _ranges_image(st, torch, frame, T, csize, rows, row_bytes, p)), "gather and ranges differ"
    return p


def _row_sizes(T, sb, total):
    return [rb for rb in (1, 7, 300, 256 * T, 4096, sb, sb + 5) if rb <= total]


def _full_decode(st, torch, frame, T, csize, total):
    out = torch.zeros(total, dtype=torch.uint8, device="cuda")
    assert st.decompress(frame, T, csize, out) == total
    return out.cpu().numpy()


@pytest.mark.parametrize("shift", [None, 0, 2])
@pytest.mark.parametrize("T", TS)
def test_level1_frames(T, shift):
    torch = _cuda()
    st = Stenos(level=1)
    try:
        if shift is not None:
            assert st.lib.stenos_set_block_size(st.ctx, shift) == 0
        sb = _sb(T, shift)
        rng = np.random.default_rng([41, T, shift or 9])
        for k, total in enumerate(_sizes(T, sb)):
            data = _mixed_data(T, total, sb, 3 * T + k)
            src = torch.from_numpy(data).cuda()
            frame = torch.zeros(st.bound(total) + 8 * (total // sb + 2), dtype=torch.uint8, device="cuda")  # (stenos_bound counts default superblocks)
            csize = st.compress(src, T, frame)
            last, nsb = st.last_index()
            assert last and nsb == (total + sb - 1) // sb
            cases = [(rb, row_set(total, sb, rb, rng)) for rb in _row_sizes(T, sb, total)]
            wide = lambda rb: dict(stride=rb + 64 + 3, mis=5)  # noqa: E731
            # the index of the compression first: the calls without one overwrite the context's index
            for rb, rows in cases:
                _gather_checked(st, torch, frame, T, csize, data, rb, rows, last)
                _gather_checked(st, torch, frame, T, csize, data, rb, rows, last, unsigned=True, **wide(rb))
            for rb, rows in cases:
                _gather_checked(st, torch, frame, T, csize, data, rb, rows)
                _gather_checked(st, torch, frame, T, csize, data, rb, rows, **wide(rb))
            n = ctypes.c_size_t(0)
            p = st.lib.stenos_hip_frame_index(st.ctx, frame.data_ptr(), T, csize, ctypes.byref(n), st._stream_ptr())
            assert p and n.value == nsb
            for rb, rows in cases:
                sl = _gather_checked(st, torch, frame, T, csize, data, rb, rows, p)
                _gather_checked(st, torch, frame, T, csize, data, rb, rows, p, **wide(rb))
                if len(rows) <= 3000:  # (one Python object per range: the short lists)
                    got = sl.buf[sl.at:sl.at + len(rows) * rb].cpu().numpy()
                    assert np.array_equal(got, _ranges_image(st, torch, frame, T, csize, rows, rb, p)), (rb, "gather and ranges differ")
    finally:
        st.close()


@pytest.mark.parametrize("row_bytes", [7, 300, 4096])
def test_chunk_boundaries(row_bytes):
    """exactly 63, 64, 65, 128 and 129 rows of one superblock and nothing else: one chunk that is not full, one that is, a full one and
    one piece, two full ones, two and one piece -- alone, and with one row of another superblock in front and behind"""
    torch = _cuda()
    st = Stenos(level=1)
    try:
        T, sb = 4, _sb(4)
        data, frame, csize = _walk_frame(st, torch, T, 3 * sb + 500)
        rng = np.random.default_rng([48, row_bytes])
        first, per_sb = -(-sb // row_bytes), sb // row_bytes - 1  # the rows wholly inside superblock 1
        for count in (63, 64, 65, 128, 129):
            inside = [first + int(r) for r in rng.integers(0, per_sb, count)] if count > per_sb else [first + int(r) for r in rng.permutation(per_sb)[:count]]
            for rows in (inside, [0] + inside + [data.nbytes // row_bytes - 1]):
                _gather_checked(st, torch, frame, T, csize, data, row_bytes, rows)
                _gather_checked(st, torch, frame, T, csize, data, row_bytes, rows, None, row_bytes + 64 + 3, 5)
    finally:
        st.close()


@pytest.mark.parametrize("T", TS)
def test_level0_frames_are_copies(T):
    torch = _cuda()
    st = Stenos(level=0)
    try:
        sb = _sb(T)
        rng = np.random.default_rng([42, T])
        for total in (sb, 2 * sb + 300, 3 * sb + 37 * T + 5):
            data = _data("rand", T, total, T)
            frame = torch.zeros(st.bound(total), dtype=torch.uint8, device="cuda")
            csize = st.compress(torch.from_numpy(data).cuda(), T, frame)
            full = _full_decode(st, torch, frame, T, csize, total)
            for row_bytes in (7, 300, 4096, sb + 5):
                if row_bytes <= total:
                    _check_all_index_forms(st, torch, frame, T, csize, full, row_bytes, row_set(total, sb, row_bytes, rng), against_ranges=row_bytes == 300)
    finally:
        st.close()


@pytest.mark.parametrize("default_size", [False, True])
@pytest.mark.parametrize("T", TS)
def test_frames_no_encoder_writes(T, default_size):
    """tests/streamgen.py: copied superblocks among block-coded ones, every block form, oversize blocks"""
    torch = _cuda()
    st = Stenos(level=1)
    try:
        rng = np.random.default_rng([43, T, int(default_size)])
        bps = 3
        sb = sg.base_superblock(T) if default_size else bps * 256 * T
        frame_np, offs, data = sg.make_mixed_frame(rng, T, 2 if default_size else 9, bps, min(sb - 1, 256 * T + 21 * T + 3), default_size=default_size)
        frame = torch.from_numpy(frame_np).cuda()
        full = _full_decode(st, torch, frame, T, frame_np.size, data.size)
        assert np.array_equal(full, data)
        for row_bytes in (7, 300, 256 * T, sb + 5):
            _check_all_index_forms(st, torch, frame, T, frame_np.size, full, row_bytes, row_set(data.size, sb, row_bytes, rng), against_ranges=row_bytes == 300)
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
    """zstd-based codes 2-5 (and bytesoftype 1): the rows come down and the pieces are finished on the host"""
    torch = _cuda()
    st = Stenos(level=1)
    try:
        T = e["T"]
        frame_np = np.frombuffer(base64.b64decode(e["frame_b64"]), dtype=np.uint8).copy()
        data = _case_input(e)
        frame = torch.from_numpy(frame_np).cuda()
        full = _full_decode(st, torch, frame, T, frame_np.size, data.nbytes)
        assert np.array_equal(full, data.view(np.uint8).ravel())
        rng = np.random.default_rng([44, T, e["level"]])
        sb = sg.base_superblock(T)
        for row_bytes in (4096, sb + 5):
            if row_bytes <= full.size:
                rows = row_set(full.size, sb, row_bytes, rng)[:40]
                _check_all_index_forms(st, torch, frame, T, frame_np.size, full, row_bytes, rows)
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
        rng = np.random.default_rng([45, T, level])
        for row_bytes in (4096, sb + 5):
            rows = row_set(total, sb, row_bytes, rng)[:40] + [total // row_bytes - 1]
            _check_all_index_forms(st, torch, frame, T, csize, full, row_bytes, rows)
    finally:
        st.close()


def _code(call):
    try:
        return call()
    except StenosError as err:
        return err.code


@pytest.mark.parametrize("row_bytes, wide", [(300, False), (4096, True), (7, True)])
def test_invalid_rows(row_bytes, wide):
    """nrows, 2^63 and 2^64 - 1 among valid ones: INVALID_PARAMETER, those slots untouched, every gap intact; the same call without
    them is then correct; an int64 tensor with -1 is the same as 2^64 - 1"""
    torch = _cuda()
    st = Stenos(level=1)
    try:
        T, sb = 4, _sb(4)
        data, frame, csize = _walk_frame(st, torch, T, 2 * sb + 777)
        nrows = data.nbytes // row_bytes
        rng = np.random.default_rng([46, row_bytes])
        good = [int(r) for r in rng.integers(0, nrows, 200)] + [0, nrows - 1]
        stride, mis = (row_bytes + 64 + 3, 5) if wide else (None, 0)
        for bad_values in ([nrows], [1 << 63], [(1 << 64) - 1], [nrows, 1 << 63, (1 << 64) - 1, nrows + 1]):
            rows = list(good)
            for k, v in enumerate(bad_values):
                rows.insert((k * 53 + 7) % len(rows), v)
            bad_at = [i for i, v in enumerate(rows) if v >= nrows]
            assert len(bad_at) == len(bad_values)
            for unsigned in (False, True):
                sl = Slots(torch, len(rows), row_bytes, stride, mis)
                assert _code(lambda: st.gather_rows(frame, T, csize, row_bytes, _rows_tensor(torch, rows, unsigned), sl.ptr, None, stride)) == INVALID_PARAMETER
                assert sl.gaps_intact()
                got = sl.buf.cpu().numpy()
                for b in bad_at:
                    assert (got[sl.at + b * sl.stride:sl.at + b * sl.stride + row_bytes] == GUARD_BYTE).all(), (bad_values, b)
            _gather_checked(st, torch, frame, T, csize, data, row_bytes, [r for i, r in enumerate(rows) if i not in bad_at], None, stride, mis)
        minus = torch.tensor([0, -1, 1], dtype=torch.int64, device="cuda")
        sl = Slots(torch, 3, row_bytes, stride, mis)
        assert _code(lambda: st.gather_rows(frame, T, csize, row_bytes, minus, sl.ptr, None, stride)) == INVALID_PARAMETER
        assert sl.gaps_intact() and (sl.buf[sl.at + sl.stride:sl.at + sl.stride + row_bytes] == GUARD_BYTE).all().item()
        # row_bytes > total: every index is invalid
        big = data.nbytes + 1
        sl = Slots(torch, 2, big)
        assert _code(lambda: st.gather_rows(frame, T, csize, big, _rows_tensor(torch, [0, 0]), sl.ptr)) == INVALID_PARAMETER
        assert sl.untouched()
    finally:
        st.close()


def test_refusals_write_nothing():
    torch = _cuda()
    st = Stenos(level=1)
    try:
        T, sb = 4, _sb(4)
        data, frame, csize = _walk_frame(st, torch, T, 2 * sb + 77)
        total = data.nbytes
        rows = [0, 3, sb // 16, total // 16 - 1]
        r = _rows_tensor(torch, rows)
        sl = Slots(torch, len(rows), 16, 32)
        call = lambda **kw: _code(lambda: st.lib.stenos_hip_gather_rows(st.ctx, frame.data_ptr(), kw.get("T", T), csize, kw.get("row_bytes", 16), kw.get("n", len(rows)),  # noqa: E731
                                                                        r.data_ptr(), sl.ptr, kw.get("stride", 32), None, st._stream_ptr()))
        for kw in (dict(row_bytes=0), dict(stride=15), dict(T=0), dict(T=65), dict(row_bytes=1 << 62, stride=1 << 62), dict(n=1 << 60),
                   dict(n=1 << 40, stride=1 << 30), dict(n=1 << 31), dict(n=1 << 30, row_bytes=17, stride=17)):
            assert call(**kw) == INVALID_PARAMETER, kw
            assert sl.untouched(), kw
        assert st.gather_rows(frame, T, csize, 16, r[:0], sl.ptr) == 0 and sl.untouched()
        # a frame header stenos_hip_decompress refuses: its code
        bad = frame.clone()
        bad[0] = 77
        assert _code(lambda: st.gather_rows(bad, T, csize, 16, r, sl.ptr, None, 32)) == INVALID_INPUT and sl.untouched()
        assert _code(lambda: st.gather_rows(frame, T, 5, 16, r, sl.ptr, None, 32)) == SRC_OVERFLOW and sl.untouched()
        # a pending _async job: refused, and the job is left alone
        src = torch.from_numpy(data).cuda()
        other = torch.zeros(st.bound(total), dtype=torch.uint8, device="cuda")
        st.compress(src, T, other, wait=False)
        assert _code(lambda: st.gather_rows(frame, T, csize, 16, r, sl.ptr, None, 32)) == INVALID_PARAMETER
        assert sl.untouched()
        assert st.finish() == csize
        assert torch.equal(other[:csize], frame[:csize])
        assert st.gather_rows(frame, T, csize, 16, r, sl.ptr, None, 32) == 64
        sl.check(data, rows)
    finally:
        st.close()


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
        rng = np.random.default_rng(47)
        rows = row_set(data.nbytes, sb, 300, rng)
        outs = [_gather_checked(st, torch, frame, T, csize, data, 300, rows, p, 300 + 67, 5).buf.cpu().numpy() for _ in range(3)]
        assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])
        index = torch.empty(7, dtype=torch.int64)
        hip = ctypes.CDLL("libamdhip64.so")
        assert hip.hipMemcpy(ctypes.c_void_p(index.data_ptr()), ctypes.c_void_p(p), ctypes.c_size_t(56), 2) == 0
        assert index.tolist() == offs
        back = torch.zeros(data.nbytes, dtype=torch.uint8, device="cuda")
        assert st.decompress(frame, T, csize, back, p) == data.nbytes
        assert np.array_equal(back.cpu().numpy(), data)
        _gather_checked(st, torch, frame, T, csize, data, sb + 5, [1, 0, 2], p)
    finally:
        st.close()


def test_damage_is_seen_where_a_row_looks():
    torch = _cuda()
    st = Stenos(level=1)
    try:
        T, sb = 4, _sb(4)
        data, frame, csize = _walk_frame(st, torch, T, 3 * sb + 500)
        offs = st.frame_index(frame, T, csize)
        def index_ptr(f, size):
            n = ctypes.c_size_t(0)
            return st.lib.stenos_hip_frame_index(st.ctx, f.data_ptr(), T, size, ctypes.byref(n), st._stream_ptr())

        rb = 100
        touching = [0, 1, sb // rb + 3, 2 * sb // rb - 1, 2 * sb // rb - 1]  # superblocks 0 and 1
        assert all((r + 1) * rb <= 2 * sb for r in touching)
        gather = lambda f, size, rows, p, sl: _code(lambda: st.gather_rows(f, T, size, rb, _rows_tensor(torch, rows), sl.ptr, p, rb + 9))  # noqa: E731
        # a byte flipped in superblock 2, which no row touches: not seen, with or without an index
        flipped = frame.clone()
        flipped[offs[2] + 4 + 40] = flipped[offs[2] + 4 + 40] ^ 0xFF
        for p in (None, index_ptr(flipped, csize)):
            sl = Slots(torch, len(touching), rb, rb + 9, 3)
            assert gather(flipped, csize, touching, p, sl) == rb * len(touching)
            sl.check(data, touching)
        # the frame cut short inside superblock 1: its csize runs past the end
        p = index_ptr(frame, csize)
        cut = offs[1] + 4 + 10
        for idx in (p, None):
            sl = Slots(torch, len(touching), rb, rb + 9, 3)
            assert gather(frame, cut, touching, idx, sl) in (SRC_OVERFLOW, INVALID_INPUT), idx
            assert sl.gaps_intact()
        sl = Slots(torch, 2, rb, rb + 9, 3)  # ... which a call that stays in superblock 0 does not see, given the index
        assert gather(frame, cut, touching[:2], p, sl) == 2 * rb
        sl.check(data, touching[:2])
        p = index_ptr(frame, csize)  # (the call without an index walked the cut frame into the context's index)
        # an unknown code and a block stream that ends too early in a touched superblock
        for at, value in ((offs[1], 9), (offs[1] + 1, 7)):
            bad = frame.clone()
            if at == offs[1] + 1:  # csize := 7: the payload ends inside the first block (the index is given, so the chain is not walked)
                bad[at:at + 3] = torch.tensor([7, 0, 0], dtype=torch.uint8, device="cuda")
            else:
                bad[at] = value
            sl = Slots(torch, len(touching), rb, rb + 9, 3)
            assert gather(bad, csize, touching, p, sl) == INVALID_INPUT, (at, value)
            assert sl.gaps_intact()
    finally:
        st.close()


def test_row_numbers_computed_on_a_side_stream():
    """The frame is written on a side stream behind a few milliseconds of other work there, and the row numbers are computed there
    by torch ops; nothing is synchronised before the call."""
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
        rb = 256
        nrows = data.nbytes // rb
        sl = Slots(torch, nrows, rb, rb + 67, 5)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            for _ in range(200):
                busy.add_(1.0)
            src.copy_(ready)
            csize = st.compress(src, T, dst)
            for _ in range(200):
                busy.add_(1.0)
            frame.copy_(dst)
            rows = (torch.randperm(nrows, device="cuda") * 7 + 3) % nrows  # (7 and nrows need not be coprime: rows may repeat)
            got = st.gather_rows(frame, T, csize, rb, rows, sl.ptr, None, rb + 67)
        torch.cuda.synchronize()
        assert got == nrows * rb
        sl.check(data, rows.cpu().tolist())
    finally:
        st.close()
