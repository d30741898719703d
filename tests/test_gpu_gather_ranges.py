"""Variable-length ranges of a frame on the device by device-resident offsets and lengths (include/stenos_hip.h:
stenos_hip_gather_ranges): the packed output equals the slices of the original array back to back and the offsets their cumulative
sum, whatever the superblock codes, the index form and the alignment of the output; the scan that forms the offsets works across
workgroups; an invalid range or lengths beyond dst_size fail the call on the device with the output untouched; offsets computed on
the stream of the call need no synchronisation; damage is seen where a range looks and nowhere else; the refusals happen before
anything is written; the bytes are those of stenos_hip_decompress_ranges and stenos_hip_gather_rows.

The output buffer is pre-filled with 0xA5 and compared whole against a numpy image, so both ends are checked."""
import ctypes

import numpy as np
import pytest

import test_decoder_streams_cpu as td
import test_gather_ranges_cpu as tc
from stenos_amd.api import Stenos, StenosError
from test_gpu_ranges import Carved, _data, _mixed_data, _sb, _sizes, _walk_frame, range_set

pytestmark = pytest.mark.gpu

E = lambda k: (1 << 64) - k  # noqa: E731
INVALID_PARAMETER, SRC_OVERFLOW, INVALID_INPUT, DST_OVERFLOW = E(9), E(2), E(4), E(6)
GUARD, GUARD_BYTE = 64, 0xA5
M64 = (1 << 64) - 1
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


def _u64(torch, values, unsigned=False):
    t = torch.from_numpy(np.asarray(values, dtype=np.uint64).view(np.int64)).cuda()
    return t.view(torch.uint64) if unsigned and hasattr(torch, "uint64") else t


class Packed:
    """room for `nbytes` of packed output, `mis` bytes behind a 256-byte boundary, at least 64 guard bytes in front and behind; the
    whole buffer is 0xA5 before the call"""

    def __init__(self, torch, nbytes, mis=0):
        self.at, self.nbytes = 256 + mis, nbytes
        self.buf = torch.full((self.at + nbytes + GUARD + 16,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 256 == 0
        self.ptr = self.buf.data_ptr() + self.at

    def check(self, want_bytes):
        got = self.buf.cpu().numpy()
        want = np.full(got.size, GUARD_BYTE, dtype=np.uint8)
        want[self.at:self.at + want_bytes.size] = want_bytes
        if not np.array_equal(got, want):
            bad = int(np.flatnonzero(got != want)[0])
            raise AssertionError(f"byte {bad} of the buffer differs (got {got[bad]}, want {want[bad]}): byte {bad - self.at} of the packed output of {want_bytes.size}")

    def untouched(self):
        return bool((self.buf == GUARD_BYTE).all().item())


def expected(full, offs, lens):
    """the slices back to back, and the n + 1 offsets"""
    offs, lens = np.asarray(offs, dtype=np.int64), np.asarray(lens, dtype=np.int64)
    D = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    idx = np.arange(D[-1], dtype=np.int64) - np.repeat(D[:-1], lens) + np.repeat(offs, lens)
    return full[idx], D


def _gather_checked(st, torch, frame, T, csize, full, ranges, index_ptr=None, mis=0, with_offsets=True, unsigned=False, room=0):
    offs, lens = [o for o, _ in ranges], [n for _, n in ranges]
    want, D = expected(full, offs, lens)
    p = Packed(torch, want.size + room, mis)
    out_offsets = torch.full((len(ranges) + 1,), -1, dtype=torch.int64, device="cuda") if with_offsets else None
    if out_offsets is not None and unsigned and hasattr(torch, "uint64"):
        out_offsets = out_offsets.view(torch.uint64)
    got = st.gather_ranges(frame, T, csize, _u64(torch, offs, unsigned), _u64(torch, lens, unsigned), p.ptr, out_offsets, index_ptr, out_size=want.size + room)
    assert got == want.size, (got, want.size)
    p.check(want)
    if out_offsets is not None:
        assert np.array_equal(out_offsets.view(torch.int64).cpu().numpy(), D), "out_offsets is not the cumulative sum"
    return p


def _frame_index_ptr(st, frame, T, csize):
    n = ctypes.c_size_t(0)
    p = st.lib.stenos_hip_frame_index(st.ctx, frame.data_ptr(), T, csize, ctypes.byref(n), st._stream_ptr())
    assert p
    return p


def ragged_set(total, sb, T, rng, nrandom):
    """range_set of test_gpu_ranges.py (zero lengths, the whole array, both sides of superblock and block boundaries), then 64 and 65
    ranges of 7 bytes inside one superblock, duplicates, and all of it in a random order"""
    r = range_set(total, sb, 256 * T, rng, nrandom)
    s = (total // sb - 1) if total >= 2 * sb else 0
    lo, hi = s * sb, min(total, (s + 1) * sb)
    sets = []
    for count in (64, 65):
        inside = [(int(x), 7) for x in rng.integers(lo, hi - 7, count)]
        sets.append(inside)
        mixed = r + inside + [inside[0], inside[0], r[7]]
        sets.append([mixed[int(k)] for k in rng.permutation(len(mixed))])
    return sets


# ---- 1. delivered bytes, across types, sizes and index forms -------------------------------------------------------------

@pytest.mark.parametrize("T", TS)
def test_delivered_bytes(T):
    torch = _cuda()
    st = Stenos(level=1)
    try:
        sb = _sb(T)
        rng = np.random.default_rng([61, T])
        for k, total in enumerate(_sizes(T, sb)):
            data = _data(("walk", "dict16", "runs", "slopes", "walk")[k], T, total, 7 * T + k)
            frame = torch.zeros(st.bound(total), dtype=torch.uint8, device="cuda")
            csize = st.compress(torch.from_numpy(data).cuda(), T, frame)
            last, nsb = st.last_index()
            assert last and nsb == (total + sb - 1) // sb
            sets = ragged_set(total, sb, T, rng, 60 if k == 3 else 25)
            # the index of the compression first: the calls without one overwrite the context's index
            for i, ranges in enumerate(sets):
                _gather_checked(st, torch, frame, T, csize, data, ranges, last, mis=5 * (i % 2), unsigned=i == 1)
            for i, ranges in enumerate(sets):
                _gather_checked(st, torch, frame, T, csize, data, ranges, None, mis=5 * ((i + 1) % 2), with_offsets=i % 2 == 0, room=(i % 3) * 1000)
            p = _frame_index_ptr(st, frame, T, csize)
            # the caller's index pointer: the same bytes on three calls in a row
            outs = [_gather_checked(st, torch, frame, T, csize, data, sets[3], p, mis=5, with_offsets=j != 1).buf.cpu().numpy() for j in range(3)]
            assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])
            _gather_checked(st, torch, frame, T, csize, data, sets[0], p)
    finally:
        st.close()


# ---- 2. mixed codes ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T", [4, 2])
def test_mixed_codes(T):
    """copied superblocks and mini-LZ blocks among block streams; the 2 sb + 100 size, whose last superblock is zstd-coded and is
    finished on the host, with ranges that end in it"""
    torch = _cuda()
    st = Stenos(level=1)
    try:
        sb = _sb(T)
        rng = np.random.default_rng([62, T])
        for k, total in enumerate(_sizes(T, sb)):
            data = _mixed_data(T, total, sb, 3 * T + k)
            frame = torch.zeros(st.bound(total), dtype=torch.uint8, device="cuda")
            csize = st.compress(torch.from_numpy(data).cuda(), T, frame)
            sets = ragged_set(total, sb, T, rng, 40)
            if total == 2 * sb + 100:
                ends = [(total - 100, 100), (total - 1, 1), (2 * sb - 3, 103), (sb + 5, sb + 50), (total - 60, 20), (0, total), (total, 0)]
                sets = [ends, sets[1] + ends, sets[3]]
            p = _frame_index_ptr(st, frame, T, csize)
            for i, ranges in enumerate(sets):
                _gather_checked(st, torch, frame, T, csize, data, ranges, p if i % 2 else None, mis=5 * (i % 2))
    finally:
        st.close()


def test_level2_frame_read_by_a_level1_context():
    """every superblock went through zstd: offsets and lengths come down and the host finishes every piece"""
    torch = _cuda()
    T, sb = 8, _sb(8)
    total = 2 * sb + 4000 + 3
    data = _mixed_data(T, total, sb, 2)
    hi = Stenos(level=2)
    try:
        frame = torch.zeros(hi.bound(total), dtype=torch.uint8, device="cuda")
        csize = hi.compress(torch.from_numpy(data).cuda(), T, frame)
    finally:
        hi.close()
    st = Stenos(level=1)
    try:
        rng = np.random.default_rng(63)
        ranges = range_set(total, sb, 256 * T, rng, 20)
        _gather_checked(st, torch, frame, T, csize, data, ranges)
        _gather_checked(st, torch, frame, T, csize, data, ranges[::-1], _frame_index_ptr(st, frame, T, csize), mis=5, with_offsets=False)
    finally:
        st.close()


# ---- 3. the scan across workgroups ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [5_000, 70_001])
def test_scan_across_workgroups(n):
    """20 and 274 blocks of 256 ranges: the blocks' sums, the one workgroup over them (runs of one block per thread), the apply pass"""
    torch = _cuda()
    st = Stenos(level=1)
    try:
        T, sb = 4, _sb(4)
        data, frame, csize = _walk_frame(st, torch, T, 2 * sb)
        rng = np.random.default_rng([64, n])
        lens = rng.integers(0, 17, n)
        offs = rng.integers(0, data.nbytes - 16, n)
        offs[::1000] = sb - 3  # (straddling the boundary)
        want, D = expected(data, offs, lens)
        p = Packed(torch, want.size, 5)
        out_offsets = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        assert st.gather_ranges(frame, T, csize, _u64(torch, offs), _u64(torch, lens), p.ptr, out_offsets, None, out_size=want.size) == want.size
        assert np.array_equal(out_offsets.cpu().numpy(), D)
        p.check(want)
    finally:
        st.close()


# ---- 4. gating -----------------------------------------------------------------------------------------------------------

def test_gating_happens_on_the_device_and_writes_nothing():
    torch = _cuda()
    st = Stenos(level=1)
    try:
        T, sb = 4, _sb(4)
        data, frame, csize = _walk_frame(st, torch, T, 2 * sb + 777)
        total = data.nbytes
        rng = np.random.default_rng(65)
        good = [(int(o), int(n)) for o, n in zip(rng.integers(0, total - 5000, 300), rng.integers(0, 5000, 300))] + [(sb - 2, 4), (0, 0), (total, 0)]
        room = sum(n for _, n in good)

        def call(offs, lens, p, dst_size):
            return _code(lambda: st.gather_ranges(frame, T, csize, offs, lens, p.ptr, None, None, out_size=dst_size))

        # four invalid ranges, one at a time in the middle of the valid set
        for bad in ((total, 1), (M64, 2), (5, M64), "negative"):
            ranges = list(good)
            ranges.insert(len(ranges) // 2, (0, 1) if bad == "negative" else bad)
            offs, lens = _u64(torch, [o for o, _ in ranges]), _u64(torch, [n for _, n in ranges])
            if bad == "negative":  # an int64 tensor: a huge unsigned value
                offs[len(ranges) // 2] = -1
            p = Packed(torch, room + 1)
            assert call(offs, lens, p, room + 1) == INVALID_PARAMETER, bad
            assert p.untouched(), bad
            # ... together with a too-small dst_size: still INVALID_PARAMETER
            assert call(offs, lens, p, room - 1) == INVALID_PARAMETER and p.untouched(), bad
        lens_neg = _u64(torch, [n for _, n in good])
        lens_neg[7] = -5
        p = Packed(torch, room)
        assert call(_u64(torch, [o for o, _ in good]), lens_neg, p, room) == INVALID_PARAMETER and p.untouched()
        # the lengths sum to one byte more than dst_size: DST_OVERFLOW, nothing written; dst_size == the sum succeeds
        offs, lens = _u64(torch, [o for o, _ in good]), _u64(torch, [n for _, n in good])
        p = Packed(torch, room)
        assert call(offs, lens, p, room - 1) == DST_OVERFLOW and p.untouched()
        assert call(offs, lens, p, 0) == DST_OVERFLOW and p.untouched()
        assert call(offs, lens, p, room) == room
        p.check(expected(data, [o for o, _ in good], [n for _, n in good])[0])
    finally:
        st.close()


# ---- 5. stream order -----------------------------------------------------------------------------------------------------

def test_offsets_computed_on_the_stream_of_the_call():
    """The offsets and lengths are computed by torch ops on a side stream behind a few milliseconds of other work there; nothing is
    synchronised before the call."""
    torch = _cuda()
    st = Stenos(level=1)
    try:
        T, sb = 8, _sb(8)
        data, frame, csize = _walk_frame(st, torch, T, 3 * sb + 4321)
        total, n = data.nbytes, 20_000
        busy = torch.zeros(64 << 20, dtype=torch.float32, device="cuda")
        p = Packed(torch, n * 64, 5)
        out_offsets = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            for _ in range(200):
                busy.add_(1.0)
            offs = (torch.randperm(n, device="cuda") * 7919 + 3) % (total - 64)
            lens = (offs * 31 + 7) % 64
            got = st.gather_ranges(frame, T, csize, offs, lens, p.ptr, out_offsets, None, out_size=n * 64)
        torch.cuda.synchronize()
        want, D = expected(data, offs.cpu().numpy(), lens.cpu().numpy())
        assert got == want.size and np.array_equal(out_offsets.cpu().numpy(), D)
        p.check(want)
    finally:
        st.close()


# ---- 6. damage -----------------------------------------------------------------------------------------------------------

def _audited_on_the_cpu_first(frame_np, size, T, total, sb, index, ranges, mis):
    """tests/test_gpu_decoder_streams.py's rule: a damaged payload reaches the device only after the audited emulation has run
    the same call on the CPU, at the alignment it will have in device memory, without an access outside its regions.  Returns the
    status word of the emulated call."""
    audit = tc._load("libstenos_emul_gather_ranges_audit.so")
    audit.emul_audit_gather_ranges.restype = ctypes.c_size_t
    audit.emul_audit_gather_ranges.argtypes = audit.emul_gather_ranges.argtypes + [ctypes.c_int, tc.U64P]
    audit.emul_audit_first_name.restype = ctypes.c_char_p
    audit.emul_set_lds_fill(0x37)
    room = sum(n for _, n in ranges)
    r, _, _, _, _, rep = tc.run_call(audit, tc.padded(frame_np[:size].tobytes()), size, T, total, sb, index, ranges, room, room, 64, 0, mis, audited=True)
    tc._audit_clean(audit, rep, "damaged frame")
    return r


def test_damage_is_seen_where_a_range_looks():
    torch = _cuda()
    st = Stenos(level=1)
    try:
        T, sb = 4, _sb(4, 2)  # superblocks of four blocks: the CPU decodes in front of the device stay short
        assert st.lib.stenos_set_block_size(st.ctx, 2) == 0
        data = _data("walk", T, 3 * sb + 500, 5)
        total = data.nbytes
        frame = torch.zeros(st.bound(total) + 8 * (total // sb + 2), dtype=torch.uint8, device="cuda")  # (stenos_bound counts default superblocks)
        csize = st.compress(torch.from_numpy(data).cuda(), T, frame)
        offs = st.frame_index(frame, T, csize)
        assert len(offs) == 5
        host = frame[:csize].cpu().numpy()
        whole = td._load("libstenos_emul_audit.so")
        whole.emul_audit_block_decompress.restype = ctypes.c_size_t
        whole.emul_audit_block_decompress.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int, tc.U64P]
        whole.emul_audit_first_name.restype = ctypes.c_char_p
        # one flipped payload byte in superblock 1 that the decoder rejects: found on the CPU, by the audited whole-superblock decode
        # (what stenos_hip_decompress runs), at the payload's alignment in device memory and through both register paths
        pay, pay_end = offs[1] + 4, offs[2]
        at = None
        for cand in range(pay, pay + 32):
            damaged = host.copy()
            damaged[cand] ^= 0xFF
            verdicts = [td.audit_decode(whole, damaged[pay:pay_end].tobytes(), T, sb, regs, pay % 16)[0] for regs in (1, 0)]
            # (rejected by a block's own checks, which the piece decoder shares -- not only by the whole decode's count of the payload's bytes)
            if all(v == tc.E(4) for v in verdicts) and _audited_on_the_cpu_first(damaged, csize, T, total, sb, offs, [(2 * sb - 1, 1)], 0) == 2:
                at = cand
                break
        assert at is not None, "no flipped byte among the first 32 of the payload is rejected"
        # (a flipped byte may be rejected only blocks later, where the chain has lost its footing: the ranges that must see it
        # reach the superblock's last byte, so every block the whole decode parses is parsed for them too)
        inside_0_and_2 = [(10, 100), (sb - 50, 50), (2 * sb, 300), (3 * sb - 7, 7), (sb + 50, 0)]
        touching_1 = inside_0_and_2[:2] + [(2 * sb - 1000, 1000)] + inside_0_and_2[2:]
        straddling = [(2 * sb - 2, 4)]
        for ranges, mis in ((inside_0_and_2, 5), (touching_1, 5), (straddling, 0)):
            status = _audited_on_the_cpu_first(damaged, csize, T, total, sb, offs, ranges, mis)
            assert status == (0 if ranges is inside_0_and_2 else 2), (status, ranges)
        flipped = torch.from_numpy(damaged).cuda()
        back = torch.zeros(total, dtype=torch.uint8, device="cuda")
        full_code = _code(lambda: st.decompress(flipped, T, csize, back))
        assert full_code in (INVALID_INPUT, SRC_OVERFLOW)
        for index_ptr in (None, _frame_index_ptr(st, flipped, T, csize)):
            _gather_checked(st, torch, flipped, T, csize, data, inside_0_and_2, index_ptr, mis=5)
            for ranges, mis in ((touching_1, 5), (straddling, 0)):
                want, _ = expected(data, [o for o, _ in ranges], [n for _, n in ranges])
                p = Packed(torch, want.size, mis)
                o, l = _u64(torch, [o for o, _ in ranges]), _u64(torch, [n for _, n in ranges])
                assert _code(lambda: st.gather_ranges(flipped, T, csize, o, l, p.ptr, None, index_ptr, out_size=want.size)) == full_code
                got = p.buf.cpu().numpy()  # nothing outside [d_dst, d_dst + D[n]) is written
                assert (got[:p.at] == GUARD_BYTE).all() and (got[p.at + want.size:] == GUARD_BYTE).all()
        # a truncated frame: a range in the missing part, with the intact frame's index and without one
        p_index = _frame_index_ptr(st, frame, T, csize)
        cut = offs[2] + 4 + 10
        for ranges in ([(10, 100), (3 * sb + 7, 50)], [(2 * sb + 100, 64)]):
            for index_ptr in (p_index, None):
                pk = Packed(torch, 150, 3)
                o, l = _u64(torch, [o for o, _ in ranges]), _u64(torch, [n for _, n in ranges])
                assert _code(lambda: st.gather_ranges(frame, T, cut, o, l, pk.ptr, None, index_ptr, out_size=150)) == SRC_OVERFLOW, (ranges, index_ptr)
                got = pk.buf.cpu().numpy()
                assert (got[:pk.at] == GUARD_BYTE).all() and (got[pk.at + 150:] == GUARD_BYTE).all()
            p_index = _frame_index_ptr(st, frame, T, csize)  # (the call without an index walked the cut frame into the context's index)
        _gather_checked(st, torch, frame, T, cut, data, [(10, 100), (sb + 7, 50)], p_index)  # ... which a call that stays in front does not see
    finally:
        st.close()


# ---- 7. host refusals ----------------------------------------------------------------------------------------------------

def test_refusals_write_nothing():
    torch = _cuda()
    st = Stenos(level=1)
    try:
        T, sb = 4, _sb(4)
        data, frame, csize = _walk_frame(st, torch, T, 2 * sb + 77)
        total = data.nbytes
        ranges = [(0, 16), (3, 100), (sb - 8, 16), (total - 16, 16)]
        o, l = _u64(torch, [a for a, _ in ranges]), _u64(torch, [n for _, n in ranges])
        p = Packed(torch, 148)
        raw = lambda **kw: st.lib.stenos_hip_gather_ranges(st.ctx, kw.get("frame", frame).data_ptr(), kw.get("T", T), kw.get("csize", csize), len(ranges), o.data_ptr(),  # noqa: E731
                                                           l.data_ptr(), kw.get("dst", p.ptr), kw.get("dst_size", 148), None, None, st._stream_ptr())
        for kw in (dict(T=0), dict(T=65)):
            assert raw(**kw) == INVALID_PARAMETER and p.untouched(), kw
        # a piece bound beyond 2^31 - 1, reached through dst_size alone: a raw address with no memory behind it
        for dst_size in ((1 << 31) * sb, ((1 << 31) - 8) * sb, 1 << 62):
            assert raw(dst=0x100000, dst_size=dst_size) == INVALID_PARAMETER, dst_size
        assert _code(lambda: st.gather_ranges(frame, T, csize, o, l, 0x100000, out_size=(1 << 31) * sb)) == INVALID_PARAMETER
        with pytest.raises(ValueError):
            st.gather_ranges(frame, T, csize, o, l, 0x100000)  # a raw address needs out_size
        assert st.gather_ranges(frame, T, csize, o[:0], l[:0], p.ptr, out_size=148) == 0 and p.untouched()
        # a frame header stenos_hip_decompress refuses: its code
        bad = frame.clone()
        bad[0] = 77
        assert raw(frame=bad) == INVALID_INPUT and p.untouched()
        assert raw(csize=5) == SRC_OVERFLOW and p.untouched()
        # a pending _async job: refused, and the job is left alone
        other = torch.zeros(st.bound(total), dtype=torch.uint8, device="cuda")
        st.compress(torch.from_numpy(data).cuda(), T, other, wait=False)
        assert raw() == INVALID_PARAMETER and p.untouched()
        assert st.finish() == csize
        assert torch.equal(other[:csize], frame[:csize])
        assert raw() == 148
        p.check(expected(data, [a for a, _ in ranges], [n for _, n in ranges])[0])
    finally:
        st.close()


def test_the_frame_of_an_empty_array():
    """accepted: only ranges of length 0 at offset 0 are valid in it"""
    torch = _cuda()
    st = Stenos(level=1)
    try:
        frame = torch.zeros(8, dtype=torch.uint8, device="cuda")  # [shift 0][0 bytes]
        p = Packed(torch, 64)
        out_offsets = torch.full((3,), -1, dtype=torch.int64, device="cuda")
        assert st.gather_ranges(frame, 4, 8, _u64(torch, [0, 0]), _u64(torch, [0, 0]), p.ptr, out_offsets, out_size=64) == 0
        assert out_offsets.tolist() == [0, 0, 0] and p.untouched()
        assert st.gather_ranges(frame, 4, 8, _u64(torch, [0]), _u64(torch, [0]), p.ptr, out_size=64) == 0
        for bad in ((0, 1), (1, 0)):
            assert _code(lambda: st.gather_ranges(frame, 4, 8, _u64(torch, [0, bad[0]]), _u64(torch, [0, bad[1]]), p.ptr, out_size=64)) == INVALID_PARAMETER, bad
            assert p.untouched()
        # No piece can exist, so no dst_size is refused and none sizes a table or a grid: capacities of 1 GiB, 3 GiB and 1 TiB (a raw
        # address with no memory behind it) cost what 64 bytes cost.  The calls above have brought up everything a call allocates.
        good, bad_o, bad_l = _u64(torch, [0, 0]), _u64(torch, [0, 0]), _u64(torch, [0, 1])
        torch.cuda.synchronize()
        free_before = torch.cuda.mem_get_info()[0]
        for dst_size in (1 << 30, 3 << 30, 1 << 40, (1 << 64) - 1):
            assert st.gather_ranges(frame, 4, 8, good, good, 0x100000, out_offsets, out_size=dst_size) == 0, dst_size
            assert out_offsets.tolist() == [0, 0, 0]
            assert _code(lambda: st.gather_ranges(frame, 4, 8, bad_o, bad_l, 0x100000, out_size=dst_size)) == INVALID_PARAMETER, dst_size
        torch.cuda.synchronize()
        assert free_before - torch.cuda.mem_get_info()[0] <= 1 << 20, "the call's tables grew with dst_size"
    finally:
        st.close()


# ---- 8. against the existing calls ---------------------------------------------------------------------------------------

def test_against_decompress_ranges_and_gather_rows():
    torch = _cuda()
    st = Stenos(level=1)
    try:
        T, sb = 4, _sb(4)
        data, frame, csize = _walk_frame(st, torch, T, 3 * sb + 500)
        total = data.nbytes
        p_index = _frame_index_ptr(st, frame, T, csize)
        rng = np.random.default_rng(66)
        ragged = [r for r in range_set(total, sb, 256 * T, rng, 100)]
        c = Carved(torch, ragged)
        assert st.decompress_ranges(frame, T, csize, ragged, c.ptrs, p_index) == sum(n for _, n in ragged)
        through_ranges = np.concatenate([c.buf[a:a + n].cpu().numpy() for (_, n), a in zip(ragged, c.at)])
        pk = _gather_checked(st, torch, frame, T, csize, data, ragged, p_index)
        assert np.array_equal(pk.buf[pk.at:pk.at + through_ranges.size].cpu().numpy(), through_ranges), "gather_ranges and decompress_ranges differ"
        # equal lengths: the rows of gather_rows
        rb = 300
        rows = [int(r) for r in rng.permutation(total // rb)[:500]] + [0, total // rb - 1, 0]
        out = torch.zeros(len(rows) * rb, dtype=torch.uint8, device="cuda")
        assert st.gather_rows(frame, T, csize, rb, _u64(torch, rows), out, p_index) == len(rows) * rb
        pk = _gather_checked(st, torch, frame, T, csize, data, [(r * rb, rb) for r in rows], p_index, mis=5)
        assert np.array_equal(pk.buf[pk.at:pk.at + out.numel()].cpu().numpy(), out.cpu().numpy()), "gather_ranges and gather_rows differ"
    finally:
        st.close()
