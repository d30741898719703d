"""Rows of a frame on the device replaced by device-resident row numbers (include/stenos_hip.h: stenos_hip_update_rows).  The oracle
is exact: the output frame is, byte for byte and in size, the frame stenos_hip_compress makes of the numpy-updated array (for input
frames that stenos_hip_compress made at the same level into a destination of the bound's size); for frames of other origin the
untouched superblocks are the input's bytes and the decode is the updated array.  d_out is written only inside the frame, and not
at all when the call fails; the new index is the context's afterwards; sources and row numbers written on the call's stream need
no synchronisation; repeated rows hold one of their sources.

The output buffer is pre-filled with 0xA5, misaligned by 5, and compared whole, so both ends are checked."""
import base64
import ctypes
import json
import os

import numpy as np
import pytest

import streamgen as sg
from stenos_amd.api import Stenos, StenosError
from stenos_amd.datagen import generate
from test_gpu_ranges import _data, _mixed_data, _sb, _sizes

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
E = lambda k: (1 << 64) - k  # noqa: E731
INVALID_PARAMETER, SRC_OVERFLOW, INVALID_INPUT, DST_OVERFLOW = E(9), E(2), E(4), E(6)
GUARD, GUARD_BYTE = 64, 0xA5
TS = [2, 4, 8, 3, 12, 64]


def _cuda():
    import torch

    assert torch.cuda.is_available()
    return torch


def _code(call):
    try:
        return call()
    except StenosError as err:
        return err.code


class Out:
    """`cap` bytes 5 bytes behind a 256-byte boundary, 64 guard bytes behind them; the whole buffer is 0xA5 before the call"""

    def __init__(self, torch, cap):
        self.at, self.cap = 256 + 5, cap
        self.buf = torch.full((self.at + cap + GUARD + 16,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 256 == 0
        self.view = self.buf[self.at:self.at + cap]

    def frame(self, size):
        """the frame's bytes; everything else in the buffer must still be 0xA5"""
        got = self.buf.cpu().numpy()
        assert (got[:self.at] == GUARD_BYTE).all() and (got[self.at + size:] == GUARD_BYTE).all(), "a byte outside [d_out, d_out + returned size) changed"
        return got[self.at:self.at + size]

    def untouched(self):
        return bool((self.buf == GUARD_BYTE).all().item())


def _rows_tensor(torch, rows):
    return torch.from_numpy(np.asarray(rows, dtype=np.uint64).view(np.int64)).cuda()


def _sources(rng, n, row_bytes, stride, mis=0, marker=None):
    """n source rows `stride` apart, `mis` bytes into the buffer; marker: the byte of the gaps (the rows then hold none of it)"""
    span = (n - 1) * stride + row_bytes if n else 0
    buf = np.full(mis + span + 3, 0 if marker is None else marker, dtype=np.uint8)
    rows = rng.integers(0, 256, (n, row_bytes), dtype=np.uint8)
    if marker is not None:
        rows[rows == marker] = marker ^ 1
    col = np.arange(row_bytes, dtype=np.int64)
    if n:
        buf[(mis + np.arange(n, dtype=np.int64) * stride)[:, None] + col] = rows
    return buf, rows


def _updated(data, rows, row_bytes, src_rows):
    out = data.copy()
    if len(rows):
        col = np.arange(row_bytes, dtype=np.int64)
        out[(np.asarray(rows, dtype=np.int64) * row_bytes)[:, None] + col] = src_rows
    return out


def _compress(st, torch, data, T, extra=0):
    src = torch.from_numpy(data).cuda()
    frame = torch.zeros(st.bound(data.nbytes) + extra, dtype=torch.uint8, device="cuda")
    csize = st.compress(src, T, frame)
    return frame, csize


def _decode(st, torch, frame, T, csize, total):
    out = torch.zeros(total, dtype=torch.uint8, device="cuda")
    assert st.decompress(frame, T, csize, out) == total
    return out.cpu().numpy()


def _download(torch, p, n):
    host = torch.empty(n, dtype=torch.int64)
    hip = ctypes.CDLL("libamdhip64.so")
    assert hip.hipMemcpy(ctypes.c_void_p(host.data_ptr()), ctypes.c_void_p(p), ctypes.c_size_t(n * 8), 2) == 0
    return host.tolist()


def _row_sizes(T, sb, total):
    return [rb for rb in (1, 7, 300, 256 * T, 4096, sb, sb + 5) if rb <= total]


def row_sets(total, sb, row_bytes, rng):
    """unique rows: one; the first and the last valid one; exactly 64 and 65 inside one superblock (the chunk boundary); a random
    quarter; every row"""
    nrows = total // row_bytes
    sets = [[int(rng.integers(0, nrows))], sorted({0, nrows - 1})]
    if sb // row_bytes >= 66:  # rows wholly inside the last whole superblock
        first = -(-max(0, total // sb - 1) * sb // row_bytes)
        if first + 65 <= nrows:
            sets += [[first + int(r) for r in rng.permutation(64)], [first + int(r) for r in rng.permutation(65)]]
    sets.append([int(r) for r in rng.permutation(nrows)[:max(1, nrows // 4)]])
    sets.append([int(r) for r in rng.permutation(nrows)])
    return sets


def _parity(T, level, shift):
    torch = _cuda()
    st, ref = Stenos(level=level), Stenos(level=level)
    try:
        if shift is not None:
            for s in (st, ref):
                assert s.lib.stenos_set_block_size(s.ctx, shift) == 0
        sb = _sb(T, shift)
        rng = np.random.default_rng([61, T, level, shift or 9])
        cases = 0
        for k, total in enumerate(_sizes(T, sb)):
            data = _mixed_data(T, total, sb, 3 * T + k)
            extra = 8 * (total // sb + 2) if shift is not None else 0  # (stenos_bound counts default superblocks)
            frame, csize = _compress(st, torch, data, T, extra)
            cap = frame.numel()
            nsb = -(-total // sb)
            n = ctypes.c_size_t(0)
            p = st.lib.stenos_hip_frame_index(st.ctx, frame.data_ptr(), T, csize, ctypes.byref(n), st._stream_ptr())
            assert p and n.value == nsb
            old_index = _download(torch, p, nsb + 1)
            old = frame[:csize].cpu().numpy()
            for rb in _row_sizes(T, sb, total):
                for rows in row_sets(total, sb, rb, rng):
                    src_np, src_rows = _sources(rng, len(rows), rb, rb)
                    want_data = _updated(data, rows, rb, src_rows)
                    want_frame, want_size = _compress(ref, torch, want_data, T, extra)
                    out = Out(torch, cap)
                    # the index of the last call on the context (the frame_index above, then every update's own) or none, in turn
                    index_ptr = None
                    if cases % 3 == 1:
                        index_ptr = st.lib.stenos_hip_frame_index(st.ctx, frame.data_ptr(), T, csize, ctypes.byref(n), st._stream_ptr())
                    r = st.update_rows(frame, T, csize, rb, _rows_tensor(torch, rows), torch.from_numpy(src_np).cuda(), out.view, index_ptr)
                    got = out.frame(r)
                    assert r == want_size, (total, rb, len(rows), r, want_size)
                    want = want_frame[:want_size].cpu().numpy()
                    if not np.array_equal(got, want):
                        bad = int(np.flatnonzero(got != want)[0])
                        raise AssertionError(f"T {T} total {total} row_bytes {rb} {len(rows)} rows: byte {bad} of the frame differs")
                    # untouched superblocks are the input's bytes; the context's index is the new frame's
                    lp, ln = st.last_index()
                    assert lp and ln == nsb
                    new_index = _download(torch, lp, nsb + 1)
                    assert new_index[0] == old_index[0] and new_index[-1] == r
                    touched = set()
                    for row in rows:
                        touched.update(range(row * rb // sb, ((row + 1) * rb - 1) // sb + 1))
                    for s in range(nsb):
                        if s not in touched:
                            assert np.array_equal(got[new_index[s]:new_index[s + 1]], old[old_index[s]:old_index[s + 1]]), s
                    cases += 1
            assert torch.equal(frame[:csize].cpu(), torch.from_numpy(old)), "the input frame was modified"
        assert cases >= 60
    finally:
        st.close()
        ref.close()


@pytest.mark.parametrize("level", [1, 0])
@pytest.mark.parametrize("T", TS)
def test_parity_with_compressing_the_updated_array(T, level):
    _parity(T, level, None)


@pytest.mark.parametrize("T", [4, 3])
def test_parity_custom_block_size(T):
    """stenos_set_block_size: a 12-byte frame header; the geometry is the header's"""
    _parity(T, 1, 2)


def test_sizes_move_both_ways():
    """a compressible superblock overwritten with noise becomes a copy, a noise superblock overwritten with constants shrinks"""
    torch = _cuda()
    st, ref = Stenos(level=1), Stenos(level=1)
    try:
        T, sb = 4, _sb(4)
        total = 6 * sb + 300
        data = _mixed_data(T, total, sb, 0)  # superblock s: walk, rand12, rand, lzmix, sine, runs, walk
        frame, csize = _compress(st, torch, data, T)
        index = st.frame_index(frame, T, csize)
        sizes = np.diff(index)
        assert sizes[2] == sb + 4 and sizes[0] < sb, sizes  # noise is stored as it is, the walk is compressed
        rng = np.random.default_rng(62)
        rb = 4096
        per = sb // rb
        rows = list(range(0, per)) + list(range(2 * per, 3 * per))  # superblocks 0 and 2, whole
        src_rows = np.concatenate([rng.integers(0, 256, (per, rb), dtype=np.uint8), np.full((per, rb), 7, dtype=np.uint8)])
        want_data = _updated(data, rows, rb, src_rows)
        want_frame, want_size = _compress(ref, torch, want_data, T)
        out = Out(torch, frame.numel())
        r = st.update_rows(frame, T, csize, rb, _rows_tensor(torch, rows), torch.from_numpy(src_rows.reshape(-1)).cuda(), out.view)
        got = out.frame(r)
        assert r == want_size and np.array_equal(got, want_frame[:r].cpu().numpy())
        lp, ln = st.last_index()
        new_sizes = np.diff(_download(torch, lp, ln + 1))
        assert new_sizes[0] == sb + 4 and new_sizes[2] < sb // 8, new_sizes
        assert (new_sizes[[1, 3, 4, 5, 6]] == sizes[[1, 3, 4, 5, 6]]).all()
        assert np.array_equal(_decode(ref, torch, out.view, T, r, total), want_data)
    finally:
        st.close()
        ref.close()


def test_out_size_exact_and_one_less():
    torch = _cuda()
    st = Stenos(level=1)
    try:
        T, sb = 8, _sb(8)
        total = 2 * sb + 300
        data = _mixed_data(T, total, sb, 2)
        frame, csize = _compress(st, torch, data, T)
        rng = np.random.default_rng(63)
        rows = [3, total // 512 - 1]
        src_np, src_rows = _sources(rng, 2, 512, 512)
        src = torch.from_numpy(src_np).cuda()
        rt = _rows_tensor(torch, rows)
        roomy = Out(torch, frame.numel())
        size = st.update_rows(frame, T, csize, 512, rt, src, roomy.view)
        want = roomy.frame(size)
        exact = Out(torch, size)
        assert st.update_rows(frame, T, csize, 512, rt, src, exact.view) == size
        assert np.array_equal(exact.frame(size), want)
        tight = Out(torch, size - 1)
        assert _code(lambda: st.update_rows(frame, T, csize, 512, rt, src, tight.view)) == DST_OVERFLOW
        assert tight.untouched()
        # no rows: a byte copy, with the same rule
        copy = Out(torch, csize)
        assert st.update_rows(frame, T, csize, 512, None, None, copy.view) == csize
        assert np.array_equal(copy.frame(csize), frame[:csize].cpu().numpy())
        tight = Out(torch, csize - 1)
        assert _code(lambda: st.update_rows(frame, T, csize, 512, None, None, tight.view)) == DST_OVERFLOW
        assert tight.untouched()
    finally:
        st.close()


@pytest.mark.parametrize("T", [4, 3])
def test_strided_misaligned_sources(T):
    """src_stride = row_bytes + 67, d_src misaligned: the gap bytes never reach the result"""
    torch = _cuda()
    st, ref = Stenos(level=1), Stenos(level=1)
    try:
        sb = _sb(T)
        total = 3 * sb + 256 * T + 37 * T + 5
        data = _data("walk", T, total, 4)
        data[data == 0xC3] = 0xC2
        frame, csize = _compress(st, torch, data, T)
        rng = np.random.default_rng([64, T])
        for rb in (1, 7, 300, sb + 5):
            nrows = total // rb
            rows = [int(r) for r in rng.permutation(nrows)[:min(nrows, 700)]]
            src_np, src_rows = _sources(rng, len(rows), rb, rb + 67, mis=3, marker=0xC3)
            src = torch.from_numpy(src_np).cuda()
            out = Out(torch, frame.numel())
            r = st.update_rows(frame, T, csize, rb, _rows_tensor(torch, rows), src.data_ptr() + 3, out.view, None, rb + 67)
            got = out.frame(r)
            want_data = _updated(data, rows, rb, src_rows)
            want_frame, want_size = _compress(ref, torch, want_data, T)
            assert r == want_size and np.array_equal(got, want_frame[:r].cpu().numpy()), rb
            back = _decode(ref, torch, out.view, T, r, total)
            assert not (back == 0xC3).any() and np.array_equal(back, want_data)
    finally:
        st.close()
        ref.close()


def test_index_forms_and_the_new_index():
    """no index, the index of the compression, the index of stenos_hip_frame_index (the last two are the context's own buffer, which
    the call replaces); afterwards the context's index is the new frame's: a gather on d_out with it returns the sources, and two
    updates in a row go from buffer to buffer without a walk"""
    torch = _cuda()
    st, ref = Stenos(level=1), Stenos(level=1)
    try:
        T, sb = 4, _sb(4)
        total = 3 * sb + 1024 + 37 * 4 + 5
        data = _mixed_data(T, total, sb, 5)
        rng = np.random.default_rng(65)
        rb = 300
        rows = [int(r) for r in rng.permutation(total // rb)[:500]]
        src_np, src_rows = _sources(rng, len(rows), rb, rb)
        src, rt = torch.from_numpy(src_np).cuda(), _rows_tensor(torch, rows)
        want_data = _updated(data, rows, rb, src_rows)
        want_frame, want_size = _compress(ref, torch, want_data, T)
        want = want_frame[:want_size].cpu().numpy()
        nsb = -(-total // sb)
        for form in ("none", "last", "frame_index"):
            frame, csize = _compress(st, torch, data, T)
            p = None
            if form == "last":
                p, n = st.last_index()
                assert p and n == nsb
            elif form == "frame_index":
                n = ctypes.c_size_t(0)
                p = st.lib.stenos_hip_frame_index(st.ctx, frame.data_ptr(), T, csize, ctypes.byref(n), st._stream_ptr())
                assert p and n.value == nsb
            a, b = Out(torch, frame.numel()), Out(torch, frame.numel())
            r = st.update_rows(frame, T, csize, rb, rt, src, a.view, p)
            assert r == want_size and np.array_equal(a.frame(r), want), form
            lp, ln = st.last_index()
            assert lp and ln == nsb
            assert _download(torch, lp, nsb + 1) == ref.frame_index(a.view, T, r), form
            # the gather call with that index returns the sources
            got = torch.zeros(len(rows) * rb, dtype=torch.uint8, device="cuda")
            assert st.gather_rows(a.view, T, r, rb, rt, got, lp) == len(rows) * rb
            assert np.array_equal(got.cpu().numpy().reshape(-1, rb), src_rows)
            # a second update, from a to b, with the index the first one left: the first rows back to what they were
            lp, ln = st.last_index()
            undo = rows[:100]
            undo_rows = np.stack([data[x * rb:(x + 1) * rb] for x in undo])
            r2 = st.update_rows(a.view, T, r, rb, _rows_tensor(torch, undo), torch.from_numpy(undo_rows.reshape(-1)).cuda(), b.view, lp)
            want2_data = _updated(want_data, undo, rb, undo_rows)
            want2_frame, want2_size = _compress(ref, torch, want2_data, T)
            assert r2 == want2_size and np.array_equal(b.frame(r2), want2_frame[:r2].cpu().numpy()), form
            assert np.array_equal(a.frame(r), want), "the input frame of the second update was modified"
            lp, ln = st.last_index()
            assert _download(torch, lp, nsb + 1) == ref.frame_index(b.view, T, r2)
    finally:
        st.close()
        ref.close()


def _check_foreign(st, ref, torch, frame_np, T, data, sb, rb, rows, rng):
    """a frame no encoder of ours wrote: untouched superblocks byte-identical, the decode is the updated array"""
    frame = torch.from_numpy(frame_np).cuda()
    total = data.size
    nsb = -(-total // sb)
    old_index = ref.frame_index(frame, T, frame_np.size)
    src_np, src_rows = _sources(rng, len(rows), rb, rb)
    out = Out(torch, st.bound(total) + frame_np.size)
    r = st.update_rows(frame, T, frame_np.size, rb, _rows_tensor(torch, rows), torch.from_numpy(src_np).cuda(), out.view)
    got = out.frame(r)
    lp, ln = st.last_index()
    assert ln == nsb
    new_index = _download(torch, lp, nsb + 1)
    assert new_index == ref.frame_index(out.view, T, r)
    touched = set()
    for row in rows:
        touched.update(range(row * rb // sb, ((row + 1) * rb - 1) // sb + 1))
    for s in range(nsb):
        if s not in touched:
            assert np.array_equal(got[new_index[s]:new_index[s + 1]], frame_np[old_index[s]:old_index[s + 1]]), s
    assert np.array_equal(got[:old_index[0]], frame_np[:old_index[0]])
    assert np.array_equal(_decode(ref, torch, out.view, T, r, total), _updated(data, rows, rb, src_rows))
    return touched


@pytest.mark.parametrize("T", [2, 4, 3])
def test_free_choice_streams(T):
    """tests/streamgen.py: legal streams no encoder writes, copied superblocks among them, a custom superblock size"""
    torch = _cuda()
    st, ref = Stenos(level=1), Stenos(level=1)
    try:
        rng = np.random.default_rng([66, T])
        bps = 3
        sb = bps * 256 * T
        frame_np, offs, data = sg.make_mixed_frame(rng, T, 9, bps, 256 * T + 21 * T + 3)
        for rb, rows in ((7, [0, 5, sb // 7, data.size // 7 - 1]), (300, [int(r) for r in rng.permutation(data.size // 300)[:9]]), (sb + 5, [1, 4])):
            touched = _check_foreign(st, ref, torch, frame_np, T, data, sb, rb, rows, rng)
            assert 0 < len(touched) < 10
    finally:
        st.close()
        ref.close()


with open(os.path.join(HERE, "golden", "level_frames.json")) as f:
    _ALL = json.load(f)["cases"]
LEVEL_CASES = [next(e for e in _ALL if e["T"] > 1 and e["level"] >= 2 and e["codes"] == [c]) for c in (2, 3, 4, 5)]


@pytest.mark.parametrize("e", LEVEL_CASES, ids=lambda e: f"{e['kind']}-T{e['T']}-l{e['level']}-codes{''.join(map(str, e['codes']))}")
def test_reference_frames_of_higher_levels(e):
    """zstd-based codes: touched superblocks are decoded on the host and encoded again at the context's level"""
    torch = _cuda()
    st, ref = Stenos(level=1), Stenos(level=1)
    try:
        T = e["T"]
        frame_np = np.frombuffer(base64.b64decode(e["frame_b64"]), dtype=np.uint8).copy()
        data = np.frombuffer(base64.b64decode(e["input_b64"]), dtype=np.uint8).copy() if "input_b64" in e else generate(e["kind"], T, e["n"], 42).view(np.uint8).ravel()
        rng = np.random.default_rng([67, T, e["level"]])
        rows = [int(r) for r in rng.permutation(data.size // 100)[:20]]
        _check_foreign(st, ref, torch, frame_np, T, data, sg.base_superblock(T), 100, rows, rng)
    finally:
        st.close()
        ref.close()


def test_errors_write_nothing():
    torch = _cuda()
    st = Stenos(level=1)
    try:
        T, sb = 4, _sb(4)
        total = 3 * sb + 500
        data = _data("walk", T, total, 5)
        frame, csize = _compress(st, torch, data, T)
        offs = st.frame_index(frame, T, csize)
        rng = np.random.default_rng(68)
        rb = 64
        nrows = total // rb
        ok = [1, sb // rb + 2, 7]  # superblocks 0 and 1
        src_np, src_rows = _sources(rng, 8, rb, rb)
        src = torch.from_numpy(src_np).cuda()
        cap = frame.numel()

        def call(rows, f=frame, size=csize, T_=T, row_bytes=rb, stride=None, index_ptr=None, cap_=cap):
            out = Out(torch, cap_)
            r = _code(lambda: st.update_rows(f, T_, size, row_bytes, _rows_tensor(torch, rows), src, out.view, index_ptr, stride))
            return r, out

        def index_ptr(f, size):
            n = ctypes.c_size_t(0)
            return st.lib.stenos_hip_frame_index(st.ctx, f.data_ptr(), T, size, ctypes.byref(n), st._stream_ptr())

        # invalid row numbers among valid ones
        for bad in (nrows, nrows + 1, 2**63, 2**64 - 1):
            r, out = call(ok + [bad] + ok[:1])
            assert r == INVALID_PARAMETER and out.untouched(), bad
        # host-side refusals
        for kw in (dict(row_bytes=0), dict(stride=rb - 1), dict(T_=0), dict(T_=65), dict(size=7), dict(row_bytes=1 << 62)):
            r, out = call(ok, **kw)
            assert r in (INVALID_PARAMETER, SRC_OVERFLOW) and (r == SRC_OVERFLOW) == ("size" in kw) and out.untouched(), kw
        r, out = call(ok, T_=1)  # bytesoftype 1 at level 1: the context could not compress the touched superblocks
        assert r == INVALID_PARAMETER and out.untouched()
        # more than 2^31 - 1 pieces (refused behind the header fetch, in front of any launch: the row numbers are never read)
        for n_, rb_ in ((1 << 31, 1), (1 << 30, 5), (3, 1 << 50)):  # one piece per row; two; 2^33 pieces per row
            out = Out(torch, cap)
            r = st.lib.stenos_hip_update_rows(st.ctx, frame.data_ptr(), T, csize, rb_, n_, _rows_tensor(torch, ok).data_ptr(), src.data_ptr(), rb_, out.view.data_ptr(),
                                              cap, None, st._stream_ptr())
            assert r == INVALID_PARAMETER and out.untouched(), (n_, rb_)
        badshift = frame.clone()
        badshift[0] = 9
        r, out = call(ok, f=badshift)
        assert r == INVALID_INPUT and out.untouched()
        for level in (2, 9):
            st.lib.stenos_set_level(st.ctx, level)
            r, out = call(ok)
            assert r == INVALID_PARAMETER and out.untouched(), level
        st.lib.stenos_set_level(st.ctx, 1)
        st.lib.stenos_set_max_nanoseconds(st.ctx, 10**9)
        r, out = call(ok)
        assert r == INVALID_PARAMETER and out.untouched()
        st.lib.stenos_set_max_nanoseconds(st.ctx, 0)
        # a pending _async job: refused, and the job is left alone
        other = torch.zeros(st.bound(total), dtype=torch.uint8, device="cuda")
        st.compress(torch.from_numpy(data).cuda(), T, other, wait=False)
        r, out = call(ok)
        assert r == INVALID_PARAMETER and out.untouched()
        assert st.finish() == csize
        # damage in a touched superblock (tests/test_gpu_ranges.py: an unknown code, a block stream that ends too early): the
        # decoder's code, nothing written; the index is given, so the chain is not walked
        for what in ("code", "csize"):
            bad = frame.clone()
            if what == "code":
                bad[offs[1]] = bad[offs[1]] ^ 0xFF
            else:
                bad[offs[1] + 1:offs[1] + 4] = torch.tensor([7, 0, 0], dtype=torch.uint8, device="cuda")
            r, out = call(ok, f=bad, index_ptr=index_ptr(frame, csize))
            assert r == INVALID_INPUT and out.untouched(), what
        # the same damage in an untouched superblock: not seen, and copied
        bad = frame.clone()
        bad[offs[2]] = bad[offs[2]] ^ 0xFF
        r, out = call(ok, f=bad, index_ptr=index_ptr(frame, csize))
        assert r < E(100)
        got = out.frame(r)
        lp, ln = st.last_index()
        new_index = _download(torch, lp, ln + 1)
        assert np.array_equal(got[new_index[2]:new_index[3]], bad[offs[2]:offs[3]].cpu().numpy())
        # the frame cut short inside superblock 1, with and without an index
        for p in (index_ptr(frame, csize), None):
            r, out = call(ok, size=offs[1] + 14, index_ptr=p)
            assert r in (SRC_OVERFLOW, INVALID_INPUT) and out.untouched(), p
        # an index that decreases, one with a superblock under four bytes, one that ends beyond the frame
        for k, (at, value, code) in enumerate(((2, offs[1] - 1, INVALID_INPUT), (3, offs[2] + 3, INVALID_INPUT), (4, csize + 1, SRC_OVERFLOW))):
            idx = list(offs)
            idx[at] = value
            d_idx = torch.tensor(idx, dtype=torch.int64, device="cuda")
            r, out = call([1, 7], index_ptr=d_idx.data_ptr())  # (superblock 0 only: the damage is the index's alone)
            assert r == code and out.untouched(), (k, hex(r))
        # and the context still works
        r, out = call(ok)
        assert r < E(100) and out.frame(r).size == r
    finally:
        st.close()


def test_rows_and_sources_made_on_the_stream_need_no_synchronisation():
    """The contract, not the mechanism: row numbers and source rows produced by torch ops on the call's stream right in front of the
    call, behind a few milliseconds of other work there, are what the call uses, with no synchronisation by the caller.  (The call
    itself begins with a header fetch that waits for the stream, so today nothing here could run ahead of them; the test pins the
    result a caller relies on.)"""
    torch = _cuda()
    st, ref = Stenos(level=1), Stenos(level=1)
    try:
        T, sb = 8, _sb(8)
        total = 3 * sb + 4321
        data = _data("sine", T, total, 9)
        frame, csize = _compress(st, torch, data, T)
        rb, n = 512, 150
        nrows = total // rb
        assert 2 * n < nrows
        s = torch.cuda.Stream()
        busy = torch.zeros(32 << 20, dtype=torch.float32, device="cuda")
        seed = torch.arange(n * rb, dtype=torch.int64, device="cuda")
        base = torch.arange(n, dtype=torch.int64, device="cuda")
        out = Out(torch, frame.numel())
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            for _ in range(100):
                busy.add_(1.0)
            rows_t = torch.flip(base, [0]) * 2 + 1  # (unique, below 2 n < nrows)
            src_t = ((seed * 2654435761) >> 7).to(torch.uint8)
            r = st.update_rows(frame, T, csize, rb, rows_t, src_t, out.view)
        torch.cuda.synchronize()
        rows = rows_t.cpu().numpy().tolist()
        assert len(set(rows)) == n
        want_data = _updated(data, rows, rb, src_t.cpu().numpy().reshape(n, rb))
        want_frame, want_size = _compress(ref, torch, want_data, T)
        assert r == want_size and np.array_equal(out.frame(r), want_frame[:r].cpu().numpy())
    finally:
        st.close()
        ref.close()


@pytest.mark.parametrize("row_bytes", [1, 300, 4096 + 5])
def test_repeated_rows(row_bytes):
    """identical sources: parity; different sources: every piece (a row cut at superblock boundaries) is one of its candidates, whole"""
    torch = _cuda()
    st, ref = Stenos(level=1), Stenos(level=1)
    try:
        T, sb = 4, _sb(4)
        total = 2 * sb + 300
        data = _data("walk", T, total, 6)
        frame, csize = _compress(st, torch, data, T)
        rng = np.random.default_rng([69, row_bytes])
        rb = row_bytes
        nrows = total // rb
        straddler = sb // rb if sb % rb else 5
        uniq = [straddler, 0, nrows - 1] + [int(r) for r in rng.integers(0, nrows, 40)]
        rows = [uniq[int(i)] for i in rng.integers(0, len(uniq), 400)]  # (more than 64 pieces in a superblock: several chunks)
        # identical sources
        per_row = {r: rng.integers(0, 256, rb, dtype=np.uint8) for r in set(rows)}
        src_rows = np.stack([per_row[r] for r in rows])
        want_data = _updated(data, rows, rb, src_rows)
        want_frame, want_size = _compress(ref, torch, want_data, T)
        out = Out(torch, frame.numel())
        r = st.update_rows(frame, T, csize, rb, _rows_tensor(torch, rows), torch.from_numpy(src_rows.reshape(-1)).cuda(), out.view)
        assert r == want_size and np.array_equal(out.frame(r), want_frame[:r].cpu().numpy())
        # different sources
        src_rows = rng.integers(0, 256, (len(rows), rb), dtype=np.uint8)
        out = Out(torch, frame.numel())
        r = st.update_rows(frame, T, csize, rb, _rows_tensor(torch, rows), torch.from_numpy(src_rows.reshape(-1)).cuda(), out.view)
        back = _decode(ref, torch, out.view, T, out.frame(r).size, total)
        covered = np.zeros(total, dtype=bool)
        for row in set(rows):
            cands = [src_rows[i] for i, x in enumerate(rows) if x == row]
            lo, hi = row * rb, (row + 1) * rb
            covered[lo:hi] = True
            cuts = [lo] + [b for b in range(sb, total, sb) if lo < b < hi] + [hi]
            for a, b in zip(cuts, cuts[1:]):
                assert any(np.array_equal(back[a:b], c[a - lo:b - lo]) for c in cands), (row, a, b)
        assert np.array_equal(back[~covered], data[~covered])
    finally:
        st.close()
        ref.close()


@pytest.mark.parametrize("own_index", [True, False], ids=["context_index", "no_index"])
def test_every_call_in_turn_on_one_context(own_index):
    """ranges, gather, update, then gather, ranges and a whole decode of the updated frame, all on one context: with the context's
    own index (stenos_hip_last_index: the buffer every walk, the update's encoder and the update's new index are written into)
    passed to each call, and with no index at all.  Every result is the numpy slice of the original or the updated array; the
    update leaves the old frame as it was."""
    torch = _cuda()
    st = Stenos(level=1)
    try:
        T, sb = 4, _sb(4)
        total = 3 * sb + 256 * T + 37 * T + 5  # three superblocks and a partial one
        nsb = 4
        data = _mixed_data(T, total, sb, 7)
        frame, csize = _compress(st, torch, data, T)
        old = frame[:csize].cpu().numpy()
        rng = np.random.default_rng(70)

        def index(n_expected=nsb):
            if not own_index:
                return None
            p, n = st.last_index()
            assert p and n == n_expected
            return p

        def check_ranges(f, size, full, p):
            ranges = [(sb - 3, 7), (2 * sb - 100, sb + 200), (5, 300), (3 * sb - 1, total - 3 * sb + 1), (sb // 2, 2 * sb)]
            dsts = [torch.full((n + 2 * GUARD,), GUARD_BYTE, dtype=torch.uint8, device="cuda") for _, n in ranges]
            assert st.decompress_ranges(f, T, size, ranges, [d.data_ptr() + GUARD for d in dsts], p) == sum(n for _, n in ranges)
            for (lo, n), d in zip(ranges, dsts):
                got = d.cpu().numpy()
                assert np.array_equal(got[GUARD:GUARD + n], full[lo:lo + n]), (lo, n)
                assert (got[:GUARD] == GUARD_BYTE).all() and (got[GUARD + n:] == GUARD_BYTE).all(), (lo, n)

        def check_gather(f, size, full, p):
            rb = 300
            assert sb % rb and (2 * sb) % rb
            rows = [0, sb // rb, 7, 2 * sb // rb, total // rb - 1, sb // rb + 1, 7]  # rows sb // rb and 2 sb // rb straddle two superblocks
            out = torch.full((len(rows) * rb + GUARD,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
            assert st.gather_rows(f, T, size, rb, _rows_tensor(torch, rows), out, p) == len(rows) * rb
            got = out.cpu().numpy()
            assert np.array_equal(got[:len(rows) * rb].reshape(-1, rb), np.stack([full[r * rb:(r + 1) * rb] for r in rows]))
            assert (got[len(rows) * rb:] == GUARD_BYTE).all()

        p = index()
        check_ranges(frame, csize, data, p)
        check_gather(frame, csize, data, p)
        # update: rows in superblocks 0 and 2 (the last row of superblock 0 among them), none in superblock 1 or 3
        rb = 512
        rows = [1, 2 * sb // rb + 3, sb // rb - 1, 3 * sb // rb - 2, 40]
        assert {r * rb // sb for r in rows} == {0, 2} and {((r + 1) * rb - 1) // sb for r in rows} <= {0, 2}
        src_np, src_rows = _sources(rng, len(rows), rb, rb)
        updated = _updated(data, rows, rb, src_rows)
        out = Out(torch, frame.numel())
        r = st.update_rows(frame, T, csize, rb, _rows_tensor(torch, rows), torch.from_numpy(src_np).cuda(), out.view, p)
        new = out.frame(r).copy()
        assert np.array_equal(frame[:csize].cpu().numpy(), old), "the update modified its input frame"
        lp, ln = st.last_index()
        assert lp and ln == nsb
        new_index = _download(torch, lp, nsb + 1)
        assert new_index[-1] == r and new_index[0] == 8
        p = index()
        check_gather(out.view, r, updated, p)
        check_ranges(out.view, r, updated, p)
        assert np.array_equal(_decode(st, torch, out.view, T, r, total), updated)
        assert np.array_equal(out.frame(r), new) and np.array_equal(frame[:csize].cpu().numpy(), old)
        # and the old frame still decodes to the original array on the same context
        assert np.array_equal(_decode(st, torch, frame, T, csize, total), data)
    finally:
        st.close()
