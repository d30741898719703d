"""Bytes appended in place to a frame on the device (include/stenos_hip.h: stenos_hip_append).  The oracle is exact: for a frame that
stenos_hip_compress made at the context's level into a destination of the bound's size, the result is, byte for byte and in size,
the frame stenos_hip_compress makes of A||B; for frames of other origin superblocks 0 .. keep are the input's bytes and the decode
is A||B.  The buffer is written only in the header's size field and from the header of A's last partial superblock to the
returned size, and not at all when the call fails; the new index is the context's afterwards; bytes written on the call's stream
need no synchronisation.

The buffer is pre-filled with 0xA5, misaligned by 5, has 64 guard bytes behind its capacity and is compared whole."""
import ctypes

import numpy as np
import pytest

from stenos_amd.api import Stenos, StenosError
from test_gpu_ranges import _data, _mixed_data, _sb

pytestmark = pytest.mark.gpu

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


class Buf:
    """a buffer of `cap` bytes 5 bytes behind a 256-byte boundary, 64 guard bytes behind it, everything 0xA5; then the frame in it"""

    def __init__(self, torch, cap, frame=None):
        self.at, self.cap = 256 + 5, cap
        self.buf = torch.full((self.at + cap + GUARD + 16,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 256 == 0
        self.view = self.buf[self.at:self.at + cap]
        if frame is not None:
            self.view[:frame.numel()] = frame
        self.before = self.buf.cpu().numpy()

    def holds(self, frame_np):
        """the whole buffer: the frame, and around it what was there before the call -- 0xA5 and, where the new frame is shorter than
        the old one (a last superblock that codes better with the bytes appended), the old frame's bytes behind the new size"""
        got = self.buf.cpu().numpy()
        want = self.before.copy()
        want[self.at:self.at + frame_np.size] = frame_np
        if not np.array_equal(got, want):
            bad = int(np.flatnonzero(got != want)[0]) - self.at
            raise AssertionError(f"byte {bad} of the buffer (frame of {frame_np.size} bytes, capacity {self.cap}) differs")
        self.before = got

    def unchanged(self):
        return np.array_equal(self.buf.cpu().numpy(), self.before)


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


def _src(torch, B, mis=3):
    """B on the device, `mis` bytes off a 256-byte boundary: (the tensor that keeps it alive, (address, length))"""
    t = torch.zeros(mis + B.size + 8, dtype=torch.uint8, device="cuda")
    t[mis:mis + B.size] = torch.from_numpy(B).cuda()
    return t, (t.data_ptr() + mis, B.size)


def _old_totals(T, sb):
    return [100, 127, 128, sb - 1, sb, sb + 1, 2 * sb + 256 * T + 3, 3 * sb]


def _appended(sb, r):
    return [1, sb - r, sb - r + 1, sb - r + 100, 2 * sb + 5]


def _parity(T, level, shift):
    torch = _cuda()
    st, ref = Stenos(level=level), Stenos(level=level)
    try:
        if shift is not None:
            for s in (st, ref):
                assert s.lib.stenos_set_block_size(s.ctx, shift) == 0
        sb = _sb(T, shift)
        cases = 0
        for kind in ("walk", "rand"):
            for i, old in enumerate(_old_totals(T, sb)):
                keep, r = old // sb, old % sb
                for j, new in enumerate(_appended(sb, r)):
                    ab = _data(kind, T, old + new, 7 * i + j + T)
                    extra = 8 * ((old + new) // sb + 2) if shift is not None else 0  # (stenos_bound counts default superblocks)
                    want_frame, want_size = _compress(ref, torch, ab, T, extra)
                    want = want_frame[:want_size].cpu().numpy()
                    want_index = ref.frame_index(want_frame, T, want_size)
                    for own_index in (False, True):
                        frame, csize = _compress(st, torch, ab[:old], T, extra)
                        p = None
                        if own_index:
                            p, n = st.last_index()
                            assert p and n == keep + (1 if r else 0)
                        buf = Buf(torch, st.bound(old + new) + extra, frame[:csize])
                        keepalive, src = _src(torch, ab[old:])
                        got = st.append(buf.view, T, csize, src, p)
                        assert got == want_size, (kind, old, new, own_index, got, want_size)
                        buf.holds(want)
                        lp, ln = st.last_index()
                        assert lp and ln == len(want_index) - 1
                        assert _download(torch, lp, ln + 1) == want_index, (kind, old, new, own_index)
                        del keepalive
                        cases += 1
        assert cases == 2 * 8 * 5 * 2
    finally:
        st.close()
        ref.close()


@pytest.mark.parametrize("level", [1, 0])
@pytest.mark.parametrize("T", TS)
def test_parity_with_compressing_the_concatenation(T, level):
    _parity(T, level, None)


@pytest.mark.parametrize("T", [4, 3])
def test_parity_custom_block_size(T):
    """stenos_set_block_size on both contexts: a 12-byte frame header, byte identity holds"""
    _parity(T, 1, 2)


@pytest.mark.parametrize("level", [1, 0])
def test_onto_the_frame_of_an_empty_array(level):
    """no geometry in the frame: stenos_hip_compress of B under the context's settings, into the buffer"""
    torch = _cuda()
    st, ref = Stenos(level=level), Stenos(level=level)
    try:
        for T in TS:
            for n in (127, 128, _sb(T) + 5):
                B = _data("walk", T, n, T + n)
                frame, csize = torch.zeros(8, dtype=torch.uint8, device="cuda"), 8  # (shift 0, size 0: the frame of an empty array)
                want_frame, want_size = _compress(ref, torch, B, T)
                buf = Buf(torch, st.bound(n), frame[:csize])
                keepalive, src = _src(torch, B)
                assert st.append(buf.view, T, csize, src) == want_size
                got = buf.buf.cpu().numpy()
                assert np.array_equal(got[buf.at:buf.at + want_size], want_frame[:want_size].cpu().numpy()), (T, n)
                assert (got[:buf.at] == GUARD_BYTE).all() and (got[buf.at + buf.cap:] == GUARD_BYTE).all()  # (behind the frame, inside the capacity: scratch)
                # nothing appended to nothing: the header's size, nothing written
                empty = Buf(torch, 64, frame[:csize])
                assert st.append(empty.view, T, csize, (None, 0)) == 8 and empty.unchanged()
    finally:
        st.close()
        ref.close()


def test_a_chain_of_appends():
    """1 000 bytes, then 20 chunks, each with the index the call before left: every intermediate frame is the compression of the
    concatenation so far; at the end the gather call with the context's index returns the right rows"""
    torch = _cuda()
    st, ref = Stenos(level=1), Stenos(level=1)
    try:
        T, sb = 4, _sb(4)
        rng = np.random.default_rng(71)
        sizes = [1, 77, sb // 3, sb, sb + 9]
        chunks = [sizes[int(k)] for k in rng.integers(0, len(sizes), 20)]
        chunks[:5] = sizes  # (every size at least once)
        total = 1000 + sum(chunks)
        data = _mixed_data(T, total, sb, 3)
        frame, csize = _compress(st, torch, data[:1000], T)
        buf = Buf(torch, st.bound(total), frame[:csize])
        have = 1000
        for n in chunks:
            p, _ = st.last_index()
            keepalive, src = _src(torch, data[have:have + n])
            csize = st.append(buf.view, T, csize, src, p)
            have += n
            want_frame, want_size = _compress(ref, torch, data[:have], T)
            assert csize == want_size, (have, n)
            buf.holds(want_frame[:want_size].cpu().numpy())
        assert have == total
        lp, ln = st.last_index()
        assert ln == -(-total // sb)
        rb = 300
        rows = [int(x) for x in rng.permutation(total // rb)[:200]] + [0, total // rb - 1]
        out = torch.zeros(len(rows) * rb, dtype=torch.uint8, device="cuda")
        rt = torch.tensor(rows, dtype=torch.int64, device="cuda")
        assert st.gather_rows(buf.view, T, csize, rb, rt, out, lp) == len(rows) * rb
        assert np.array_equal(out.cpu().numpy().reshape(-1, rb), np.stack([data[x * rb:(x + 1) * rb] for x in rows]))
        # no bytes: the end of the chain after the checks, nothing written
        lp, ln = st.last_index()
        for p in (lp, None):
            assert st.append(buf.view, T, csize, (None, 0), p) == csize
        buf.holds(want_frame[:want_size].cpu().numpy())
    finally:
        st.close()
        ref.close()


def test_bytes_made_on_the_stream_need_no_synchronisation():
    """The contract, not the mechanism: B produced by a torch op on the call's stream right in front of the call, behind a few
    milliseconds of other work there, is what the call appends, with no synchronisation by the caller."""
    torch = _cuda()
    st, ref = Stenos(level=1), Stenos(level=1)
    try:
        T, sb = 8, _sb(8)
        old, new = 2 * sb + 4321, 3 * sb + 77
        data = _data("sine", T, old, 9)
        frame, csize = _compress(st, torch, data, T)
        buf = Buf(torch, st.bound(old + new), frame[:csize])
        s = torch.cuda.Stream()
        busy = torch.zeros(32 << 20, dtype=torch.float32, device="cuda")
        seed = torch.arange(new, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            for _ in range(100):
                busy.add_(1.0)
            b_t = ((seed * 2654435761) >> 16).to(torch.uint8)
            r = st.append(buf.view, T, csize, b_t)
        torch.cuda.synchronize()
        want_frame, want_size = _compress(ref, torch, np.concatenate([data, b_t.cpu().numpy()]), T)
        assert r == want_size
        buf.holds(want_frame[:want_size].cpu().numpy())
    finally:
        st.close()
        ref.close()


def test_failures_write_nothing():
    torch = _cuda()
    st = Stenos(level=1)
    try:
        T, sb = 4, _sb(4)
        old, new = 2 * sb + 500, sb + 300
        data = _data("walk", T, old + new, 5)
        frame, csize = _compress(st, torch, data[:old], T)
        offs = st.frame_index(frame, T, csize)
        keepalive, src = _src(torch, data[old:])
        roomy = Buf(torch, st.bound(old + new), frame[:csize])
        size = st.append(roomy.view, T, csize, src)
        want = roomy.buf[roomy.at:roomy.at + size].cpu().numpy()

        def call(cap=st.bound(old + new), f=frame[:csize], bytes_=csize, T_=T, index=None, src_=src):
            buf = Buf(torch, cap, f)
            d_idx = torch.tensor(index, dtype=torch.int64, device="cuda") if index is not None else None
            r = _code(lambda: st.append(buf.view, T_, bytes_, src_, d_idx.data_ptr() if d_idx is not None else None))
            return r, buf

        # exactly enough; one byte short
        r, buf = call(cap=size)
        assert r == size
        buf.holds(want)
        r, buf = call(cap=size - 1)
        assert r == DST_OVERFLOW and buf.unchanged()
        r, buf = call(cap=size - 1, index=offs)
        assert r == DST_OVERFLOW and buf.unchanged()
        # capacity < bytes, and the other refusals of the host
        r, buf = call(cap=csize - 1, f=frame[:csize - 1])
        assert r == INVALID_PARAMETER and buf.unchanged()
        for kw in (dict(T_=0), dict(T_=65), dict(T_=1), dict(bytes_=7), dict(src_=(src[0], 1 << 56)),
                   dict(src_=(src[0], 1 << 50))):  # (a size the header cannot hold; more than 2^31 - 1 superblocks: refused before B is looked at)
            r, buf = call(**kw)
            assert r in (INVALID_PARAMETER, SRC_OVERFLOW) and (r == SRC_OVERFLOW) == ("bytes_" in kw) and buf.unchanged(), kw
        badshift = frame[:csize].clone()
        badshift[0] = 9
        r, buf = call(f=badshift)
        assert r == INVALID_INPUT and buf.unchanged()
        for level in (2, 9):
            st.lib.stenos_set_level(st.ctx, level)
            r, buf = call()
            assert r == INVALID_PARAMETER and buf.unchanged(), level
        st.lib.stenos_set_level(st.ctx, 1)
        st.lib.stenos_set_max_nanoseconds(st.ctx, 10**9)
        r, buf = call()
        assert r == INVALID_PARAMETER and buf.unchanged()
        st.lib.stenos_set_max_nanoseconds(st.ctx, 0)
        # a pending _async job: refused, and the job is left alone
        other = torch.zeros(st.bound(old), dtype=torch.uint8, device="cuda")
        st.compress(torch.from_numpy(data[:old]).cuda(), T, other, wait=False)
        r, buf = call()
        assert r == INVALID_PARAMETER and buf.unchanged()
        assert st.finish() == csize
        # an index with each bad entry (keep = 2, r > 0: entries 2 and 3 are the ones the call uses)
        for at, value, code in ((2, 7, INVALID_INPUT), (3, offs[2] + 3, INVALID_INPUT), (3, offs[2] - 1, INVALID_INPUT), (3, csize + 1, SRC_OVERFLOW),
                                (2, csize - 3, INVALID_INPUT), (2, 2**63 - 1, INVALID_INPUT)):
            idx = list(offs)
            idx[at] = value
            r, buf = call(index=idx)
            assert r == code and buf.unchanged(), (at, value, hex(r))
        # entries in front of `keep` are not looked at
        idx = list(offs)
        idx[0], idx[1] = 2**62, 3
        r, buf = call(index=idx)
        assert r == size
        buf.holds(want)
        # the partial last superblock cut short, with and without an index; its code made invalid
        for index in (offs, None):
            r, buf = call(f=frame[:csize - 10], bytes_=csize - 10, index=index)
            assert r == SRC_OVERFLOW and buf.unchanged(), index
        short = frame[:csize].clone()
        short[offs[2] + 1:offs[2] + 4] = torch.tensor([0xFF, 0xFF, 0x7F], dtype=torch.uint8, device="cuda")  # a payload far beyond the frame
        r, buf = call(f=short, index=offs)
        assert r == SRC_OVERFLOW and buf.unchanged()
        for what in ("code", "csize"):
            bad = frame[:csize].clone()
            if what == "code":
                bad[offs[2]] = bad[offs[2]] ^ 0xFF
            else:
                bad[offs[2] + 1:offs[2] + 4] = torch.tensor([7, 0, 0], dtype=torch.uint8, device="cuda")  # a block stream that ends too early
            r, buf = call(f=bad, index=offs)
            assert r == INVALID_INPUT and buf.unchanged(), what
        # and the context still works
        r, buf = call()
        assert r == size
        buf.holds(want)
    finally:
        st.close()


def test_superblocks_in_front_are_not_checked():
    """a byte flipped in the payload of superblock 0 of a three-superblock frame: the append succeeds and the byte arrives unchanged"""
    torch = _cuda()
    st, ref = Stenos(level=1), Stenos(level=1)
    try:
        T, sb = 4, _sb(4)
        old, new = 2 * sb + 700, 1234
        data = _data("walk", T, old + new, 8)
        frame, csize = _compress(st, torch, data[:old], T)
        offs = st.frame_index(frame, T, csize)
        want_frame, want_size = _compress(ref, torch, data, T)
        want = want_frame[:want_size].cpu().numpy()
        at = offs[0] + 4 + 100
        for index in (offs, None):
            bad = frame[:csize].clone()
            bad[at] = bad[at] ^ 0x55
            buf = Buf(torch, st.bound(old + new), bad)
            keepalive, src = _src(torch, data[old:])
            d_idx = torch.tensor(index, dtype=torch.int64, device="cuda") if index else None
            r = st.append(buf.view, T, csize, src, d_idx.data_ptr() if index else None)
            assert r == want_size
            want[at] ^= 0x55
            buf.holds(want)
            want[at] ^= 0x55
    finally:
        st.close()
        ref.close()


def _check_foreign(st, ref, torch, frame_np, T, data, sb, B):
    """a frame another encoder wrote: superblocks 0 .. keep and every header byte but the size field unchanged, the decode is A||B"""
    old = data.size
    keep = old // sb
    frame = torch.from_numpy(frame_np).cuda()
    old_index = ref.frame_index(frame, T, frame_np.size)
    buf = Buf(torch, frame_np.size + st.bound(old + B.size), frame)  # (the last superblock may grow when it is encoded again at level 1)
    keepalive, src = _src(torch, B)
    r = st.append(buf.view, T, frame_np.size, src)
    got = buf.buf.cpu().numpy()
    end = max(r, frame_np.size)  # (behind a new frame that is shorter than the old one, the old one's bytes are still there)
    assert (got[:buf.at] == GUARD_BYTE).all() and (got[buf.at + end:] == GUARD_BYTE).all()
    assert np.array_equal(got[buf.at + r:buf.at + end], frame_np[r:end])
    got = got[buf.at:buf.at + r]
    p = old_index[keep]
    assert np.array_equal(got[old_index[0]:p], frame_np[old_index[0]:p]) and got[0] == frame_np[0] and np.array_equal(got[8:old_index[0]], frame_np[8:old_index[0]])
    assert int.from_bytes(bytes(got[1:8]), "little") == old + B.size
    lp, ln = st.last_index()
    new_index = _download(torch, lp, ln + 1)
    assert new_index == ref.frame_index(buf.view, T, r) and new_index[:keep + 1] == old_index[:keep + 1]
    assert np.array_equal(_decode(ref, torch, buf.view, T, r, old + B.size), np.concatenate([data, B]))


@pytest.mark.parametrize("level", [2, 9])
def test_frames_of_higher_levels(level):
    """frames the host-pointer call made at level 2 and 9 (zstd-based codes in every superblock), appended to by a level-1 context"""
    torch = _cuda()
    st, ref, host = Stenos(level=1), Stenos(level=1), Stenos(level=level)
    try:
        for T in (4, 8):
            sb = _sb(T)
            for old, new in ((2 * sb + 300, 500), (sb + 77, 2 * sb + 5), (3 * sb, 100)):
                data = _mixed_data(T, old, sb, T + level)
                cap = host.bound(old)
                dst = np.zeros(cap, dtype=np.uint8)
                r = host.lib.stenos_compress_generic(host.ctx, data.ctypes.data, T, old, dst.ctypes.data, cap)
                assert r < E(100), hex(r)
                frame_np = dst[:r].copy()
                fsb = _sb(T) << int(frame_np[0]) if frame_np[0] != 255 else int.from_bytes(bytes(frame_np[8:12]), "little")
                B = _data("walk", T, new, level + new)
                _check_foreign(st, ref, torch, frame_np, T, data, fsb, B)
    finally:
        st.close()
        ref.close()
        host.close()


def test_the_frames_geometry_wins():
    """a frame made under stenos_set_block_size, appended to by a context without that setting: the header's superblock size holds"""
    torch = _cuda()
    st, ref, maker = Stenos(level=1), Stenos(level=1), Stenos(level=1)
    try:
        T, shift = 4, 2
        assert maker.lib.stenos_set_block_size(maker.ctx, shift) == 0
        sb = _sb(T, shift)
        for old, new in ((5 * sb + 321, 3 * sb + 7), (4 * sb, sb - 1)):
            data = _mixed_data(T, old + new, sb, 4)
            extra = 8 * ((old + new) // sb + 2)
            frame, csize = _compress(maker, torch, data[:old], T, extra)
            want_frame, want_size = _compress(maker, torch, data, T, extra)
            frame_np = frame[:csize].cpu().numpy()
            assert frame_np[0] == 255
            buf = Buf(torch, maker.bound(old + new) + extra, frame[:csize])
            keepalive, src = _src(torch, data[old:])
            r = st.append(buf.view, T, csize, src)
            assert r == want_size
            buf.holds(want_frame[:want_size].cpu().numpy())  # (both contexts are at level 1: the bytes are the maker's too)
            _check_foreign(st, ref, torch, frame_np, T, data[:old], sb, data[old:])
    finally:
        st.close()
        ref.close()
        maker.close()


def test_offsets_beyond_4_gib():
    """a full-entropy array just beyond 4 GiB (stored as copies, so p >= 2^32), 1 MiB + 5 bytes appended behind a partial superblock"""
    torch = _cuda()
    GIB, SB, P32 = 1 << 30, 131072, 1 << 32
    torch.cuda.empty_cache()
    if torch.cuda.mem_get_info()[0] < 16 * GIB:
        pytest.skip("needs 16 GiB of free device memory")
    T, old, new = 4, P32 + 3 * SB + 1000, (1 << 20) + 5
    st, ref = Stenos(level=1), Stenos(level=1)
    try:
        g = torch.Generator(device="cuda")
        g.manual_seed(81)
        src = torch.empty(old + new, dtype=torch.uint8, device="cuda")
        for o in range(0, old + new, GIB):
            n = min(GIB, old + new - o)
            src[o:o + n] = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda", generator=g)
        at, cap = 256 + 5, st.bound(old + new)
        whole = torch.full((at + cap + GUARD + 16,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
        view = whole[at:at + cap]
        first = torch.empty(st.bound(old), dtype=torch.uint8, device="cuda")
        csize = st.compress(src[:old], T, first)
        view[:csize] = first[:csize]
        del first
        keep = old // SB
        p, n = st.last_index()
        assert n == keep + 1
        old_index = _download(torch, p, n + 1)
        assert old_index[keep] >= P32
        torch.cuda.synchronize()
        r = st.append(view, T, csize, src[old:], p)
        assert r > csize
        for o in range(at + r, whole.numel(), GIB):
            assert bool((whole[o:o + GIB] == GUARD_BYTE).all().item()), "a byte behind the returned size changed"
        lp, ln = st.last_index()
        nsb = -(-(old + new) // SB)
        assert ln == nsb
        new_index = _download(torch, lp, ln + 1)
        assert new_index[:keep + 1] == old_index[:keep + 1] and new_index[-1] == r
        want_index = ref.frame_index(view, T, r)
        assert new_index == want_index and all(x > P32 for x in new_index[keep:])
        span = 2 << 20
        out = torch.zeros(span, dtype=torch.uint8, device="cuda")
        assert st.decompress_range(view, T, r, old + new - span, span, out, lp) == span
        assert torch.equal(out, src[old + new - span:])
        # the stored superblocks in front, around 2^32: still the source's bytes
        probe = torch.zeros(4096, dtype=torch.uint8, device="cuda")
        for lo in (0, P32 - 2048, keep * SB - 4096):
            assert st.decompress_range(view, T, r, lo, 4096, probe, lp) == 4096
            assert torch.equal(probe, src[lo:lo + 4096]), lo
    finally:
        st.close()
        ref.close()
        del src, whole
        torch.cuda.empty_cache()
