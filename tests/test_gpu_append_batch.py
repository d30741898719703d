"""Bytes appended in place to many frames on the device in one call (include/stenos_hip.h: stenos_hip_append_batch).  The oracle is
exact: every frame ends up, byte for byte and in size, as stenos_hip_append alone would leave it -- for frames stenos_hip_compress
made at the context's level into destinations of the bound's size, the frame stenos_hip_compress makes of A_f||B_f.  All or
nothing: after any failure every buffer is what it was, results[] is untouched and the context holds no many-frame index.  The
context's index afterwards is that of the new frames.

Every frame of every case lies in a Buf of tests/test_gpu_append.py: 5 bytes behind a 256-byte boundary, pre-filled with 0xA5,
64 guard bytes behind its capacity, compared whole."""
from ctypes import c_size_t, c_void_p

import numpy as np
import pytest

from stenos_amd.api import Stenos
from test_gpu_append import (DST_OVERFLOW, GUARD_BYTE, INVALID_INPUT, INVALID_PARAMETER, SRC_OVERFLOW, TS, Buf, _appended, _compress, _cuda, _decode, _download, _old_totals,
                             _src)
from test_gpu_ranges import _data, _mixed_data, _sb

pytestmark = pytest.mark.gpu

E = lambda k: (1 << 64) - k  # noqa: E731
NONE = np.zeros(0, dtype=np.uint8)


def _empty_frame(torch):
    return torch.zeros(8, dtype=torch.uint8, device="cuda"), 8  # (shift 0, size 0: the frame of an empty array)


class Case:
    """frames of A_f (None: the frame of an empty array) in Bufs sized for A_f||B_f, and the B_f on the device, misaligned by 3"""

    def __init__(self, st, torch, T, pairs, extra=0, caps=None):
        self.torch, self.T, self.pairs = torch, T, pairs
        self.bufs, self.sizes, self.srcs, self.keepalive = [], [], [], []
        for f, (A, B) in enumerate(pairs):
            frame, csize = _empty_frame(torch) if A is None else _compress(st, torch, A, T, extra)
            total = (0 if A is None else A.size) + B.size
            self.bufs.append(Buf(torch, caps[f] if caps and caps[f] is not None else st.bound(total) + extra, frame[:csize]))
            self.sizes.append(csize)
            if B.size:
                k, s = _src(torch, B)
                self.keepalive.append(k)
                self.srcs.append(s)
            else:
                self.srcs.append(None)

    @property
    def views(self):
        return [b.view for b in self.bufs]

    def raw(self, st, index_ptr=None, frames=None, sizes=None, caps=None, srcs=None, T=None):
        """the C call itself, results pre-filled with 77: (return value, results)"""
        m = len(self.bufs)
        P, Z = c_void_p * m, c_size_t * m
        fr = frames or [b.view.data_ptr() for b in self.bufs]
        cp = caps or [b.cap for b in self.bufs]
        pairs = [(None, 0) if s is None else s for s in (srcs or self.srcs)]
        res = Z(*([77] * m))
        r = st.lib.stenos_hip_append_batch(st.ctx, m, self.T if T is None else T, P(*fr), Z(*(sizes or self.sizes)), Z(*cp), P(*[p if n else None for p, n in pairs]),
                                           Z(*[n for _, n in pairs]), res, index_ptr, st._stream_ptr())
        return r, list(res)

    def unchanged(self):
        return all(b.unchanged() for b in self.bufs)


def _wants(ref, torch, T, pairs, extra=0):
    """per frame: the frame stenos_hip_compress makes of A_f||B_f (nothing appended to an empty array: its 8 bytes)"""
    out = []
    for A, B in pairs:
        whole = B if A is None else np.concatenate([A, B])
        if whole.size == 0:
            out.append(np.zeros(8, dtype=np.uint8))
            continue
        frame, size = _compress(ref, torch, whole, T, extra)
        out.append(frame[:size].cpu().numpy())
    return out


def _index_of(ref, torch, views, T, sizes):
    p, n = ref.frames_index(views, T, sizes)
    return _download(torch, p, n)


def _check(case, st, ref, results, wants):
    torch = case.torch
    assert results == [w.size for w in wants], (results, [w.size for w in wants])
    for f, (b, w) in enumerate(zip(case.bufs, wants)):
        try:
            b.holds(w)
        except AssertionError as err:
            raise AssertionError(f"frame {f}: {err}") from None
    lp, ln = st.last_frames_index()
    assert lp, "no many-frame index after a successful call"
    assert _download(torch, lp, ln) == _index_of(ref, torch, case.views, case.T, results), "the context's index is not that of the new frames"
    assert not st.last_index()[0]  # (as after any batch)


def _index(case, st, torch, mode):
    """d_index: NULL ("walk"), a caller's copy ("copy"), the context's own pointer ("own") -> (pointer, what keeps it alive)"""
    if mode == "walk":
        return None, None
    p, n = st.frames_index(case.views, case.T, case.sizes)
    if mode == "own":
        return p, None
    copy = torch.tensor(_download(torch, p, n), dtype=torch.int64, device="cuda")
    return copy.data_ptr(), copy


def _parity_pairs(T, sb, seed):
    """nine frames: seven different (old, new) of the single call's grid (the first an array under 128 bytes), one with nothing
    appended, one frame of an empty array with bytes appended"""
    olds = _old_totals(T, sb)
    pairs = []
    for i in range(7):
        old = olds[(i * 3 + seed) % len(olds)] if i else 100
        new = _appended(sb, old % sb)[(i + seed) % 5] if i else 1
        ab = _data(("walk", "rand")[i % 2], T, old + new, 7 * i + seed)
        pairs.append((ab[:old], ab[old:]))
    pairs.insert(3, (_data("walk", T, olds[(seed + 5) % len(olds)], seed), NONE))
    pairs.insert(6, (None, _data("rand", T, (127, sb + 5, 128)[seed % 3], seed + 1)))
    return pairs


@pytest.mark.parametrize("level", [1, 0])
@pytest.mark.parametrize("T", TS)
def test_parity_with_compressing_the_concatenations(T, level):
    torch = _cuda()
    st, ref = Stenos(level=level), Stenos(level=level)
    try:
        sb = _sb(T)
        pairs = _parity_pairs(T, sb, T + level)
        assert len(pairs) == 9
        wants = _wants(ref, torch, T, pairs)
        for mode in ("walk", "copy", "own"):
            case = Case(st, torch, T, pairs)
            index_ptr, keep = _index(case, st, torch, mode)
            results = st.append_batch(case.views, T, case.sizes, case.srcs, index_ptr)
            _check(case, st, ref, results, wants)
            del keep
    finally:
        st.close()
        ref.close()


@pytest.mark.parametrize("m", [1, 5])
def test_equal_to_the_single_call(m):
    """buffers grown by one stenos_hip_append each against the same buffers grown by one batch call: byte-identical, whole"""
    torch = _cuda()
    st, one = Stenos(level=1), Stenos(level=1)
    try:
        T, sb = 4, _sb(4)
        shapes = [(2 * sb + 500, sb + 300), (sb, 1), (100, 27), (sb - 1, 1), (3 * sb + 7, 2 * sb + 5)][:m]
        pairs = []
        for i, (old, new) in enumerate(shapes):
            ab = _mixed_data(T, old + new, sb, i + 3)
            pairs.append((ab[:old], ab[old:]))
        batch, single = Case(st, torch, T, pairs), Case(one, torch, T, pairs)
        results = st.append_batch(batch.views, T, batch.sizes, batch.srcs)
        for f in range(m):
            assert one.append(single.bufs[f].view, T, single.sizes[f], single.srcs[f]) == results[f]
            assert np.array_equal(batch.bufs[f].buf.cpu().numpy(), single.bufs[f].buf.cpu().numpy()), f
    finally:
        st.close()
        one.close()


@pytest.mark.parametrize("T", [4, 3])
def test_custom_block_size(T):
    """stenos_set_block_size on both contexts: 12-byte frame headers, also for the page that starts empty; a frame made under
    another setting than the rest is refused with nothing written"""
    torch = _cuda()
    st, ref, other = Stenos(level=1), Stenos(level=1), Stenos(level=1)
    try:
        shift = 2
        for s in (st, ref):
            assert s.lib.stenos_set_block_size(s.ctx, shift) == 0
        sb = _sb(T, shift)
        pairs = []
        for i, (old, new) in enumerate(((2 * sb + 77, sb + 9), (sb, sb - 1), (500, 3 * sb), (3 * sb + 1, 0))):
            ab = _mixed_data(T, old + new, sb, i + T)
            pairs.append((ab[:old], ab[old:]))
        pairs.append((None, _data("walk", T, sb + 100, 5)))
        extra = 8 * 10
        wants = _wants(ref, torch, T, pairs, extra)
        assert wants[4][0] == 255
        for with_index in (False, True):
            case = Case(st, torch, T, pairs, extra)
            p = st.frames_index(case.views, T, case.sizes)[0] if with_index else None
            _check(case, st, ref, st.append_batch(case.views, T, case.sizes, case.srcs, p), wants)
        # frame 1 made without the setting: another superblock size
        case = Case(st, torch, T, pairs, extra)
        foreign, fsize = _compress(other, torch, pairs[1][0], T)
        case.bufs[1] = Buf(torch, st.bound(2 * sb) + extra, foreign[:fsize])
        case.sizes[1] = fsize
        assert case.raw(st) == (INVALID_PARAMETER, [77] * 5) and case.unchanged()
        assert st.last_frames_index() == (None, 0)
    finally:
        st.close()
        ref.close()
        other.close()


def test_a_chain_of_batch_appends():
    """16 pages, half of them starting empty, 6 rounds, each with the index the round before left: every intermediate frame is the
    compression of its concatenation so far; at the end the batched gather with the context's index returns the right rows"""
    torch = _cuda()
    st, ref = Stenos(level=1), Stenos(level=1)
    try:
        T, sb, m, rounds = 4, _sb(4), 16, 6
        rng = np.random.default_rng(72)
        choices = [0, 1, 77, sb // 3, sb, sb + 9]
        plan = rng.integers(0, len(choices), (rounds, m))
        plan[0, :6] = np.arange(6)  # (every size at least once)
        start = [0 if f % 2 else 1000 for f in range(m)]
        totals = [start[f] + sum(choices[int(k)] for k in plan[:, f]) for f in range(m)]
        data = [_mixed_data(T, max(totals[f], 1), sb, f + 3)[:totals[f]] for f in range(m)]
        case = Case(st, torch, T, [(data[f][:start[f]] if start[f] else None, NONE) for f in range(m)], caps=[st.bound(t) for t in totals])
        have, sizes, index_ptr = list(start), list(case.sizes), None
        for rnd in range(rounds):
            keep, srcs = [], []
            for f in range(m):
                n = choices[int(plan[rnd, f])]
                k, s = _src(torch, data[f][have[f]:have[f] + n]) if n else (None, None)
                keep.append(k)
                srcs.append(s)
                have[f] += n
            sizes = st.append_batch(case.views, T, sizes, srcs, index_ptr)
            wants = _wants(ref, torch, T, [(None, data[f][:have[f]]) for f in range(m)])
            _check(case, st, ref, sizes, wants)
            index_ptr = st.last_frames_index()[0]
        assert have == totals
        rb = 100
        ids, rows = [], []
        for f in range(m):
            for x in rng.permutation(max(totals[f] // rb, 1))[:8]:
                if totals[f] >= rb:
                    ids.append(f)
                    rows.append(int(x))
        out = torch.zeros(len(rows) * rb, dtype=torch.uint8, device="cuda")
        it, rt = torch.tensor(ids, dtype=torch.int64, device="cuda"), torch.tensor(rows, dtype=torch.int64, device="cuda")
        assert st.gather_rows_batch(case.views, T, sizes, rb, it, rt, out, index_ptr) == len(rows) * rb
        assert np.array_equal(out.cpu().numpy().reshape(-1, rb), np.stack([data[f][x * rb:(x + 1) * rb] for f, x in zip(ids, rows)]))
    finally:
        st.close()
        ref.close()


def test_many_frames():
    """300 frames of 1 000-byte int32 arrays, 77 bytes appended to each: more frames than a planning workgroup has threads; ten of
    them are arrays under 128 bytes, before and after, so the host's zstd paths run on both sides"""
    torch = _cuda()
    st, ref = Stenos(level=1), Stenos(level=1)
    try:
        T, m = 4, 300
        pairs = []
        for f in range(m):
            old = 40 if f % 30 == 7 else 1000
            ab = _data(("walk", "rand", "sine")[f % 3], T, old + 77, f)
            pairs.append((ab[:old], ab[old:]))
        assert sum(1 for a, b in pairs if a.size + b.size < 128) == 10
        wants = _wants(ref, torch, T, pairs)
        case = Case(st, torch, T, pairs)
        p, _ = st.frames_index(case.views, T, case.sizes)
        _check(case, st, ref, st.append_batch(case.views, T, case.sizes, case.srcs, p), wants)
    finally:
        st.close()
        ref.close()


def test_bytes_made_on_the_stream_need_no_synchronisation():
    """The contract, not the mechanism: the B_f produced by torch ops on the call's stream right in front of the call, behind a few
    milliseconds of other work there, are what the call appends, with no synchronisation by the caller."""
    torch = _cuda()
    st, ref = Stenos(level=1), Stenos(level=1)
    try:
        T, sb = 8, _sb(8)
        olds, news = [2 * sb + 4321, 900, sb], [3 * sb + 77, sb + 1, 555]
        data = [_data("sine", T, old, 9 + i) for i, old in enumerate(olds)]
        case = Case(st, torch, T, [(d, NONE) for d in data], caps=[st.bound(o + n) for o, n in zip(olds, news)])
        s = torch.cuda.Stream()
        busy = torch.zeros(32 << 20, dtype=torch.float32, device="cuda")
        seeds = [torch.arange(n, dtype=torch.int64, device="cuda") for n in news]
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            for _ in range(100):
                busy.add_(1.0)
            made = [((seed * (2654435761 + 2 * i)) >> 16).to(torch.uint8) for i, seed in enumerate(seeds)]
            results = st.append_batch(case.views, T, case.sizes, made)
        torch.cuda.synchronize()
        wants = _wants(ref, torch, T, [(d, b.cpu().numpy()) for d, b in zip(data, made)])
        _check(case, st, ref, results, wants)
    finally:
        st.close()
        ref.close()


def test_failures_write_nothing():
    """m = 4, the fault in frame 2: every buffer unchanged, results untouched, no many-frame index; then a good call succeeds"""
    torch = _cuda()
    st, ref = Stenos(level=1), Stenos(level=1)
    try:
        T, sb = 4, _sb(4)
        shapes = [(sb + 300, 100), (2 * sb + 700, sb), (2 * sb + 500, sb + 300), (700, 2000)]
        pairs = []
        for i, (old, new) in enumerate(shapes):
            ab = _data("walk", T, old + new, 5 + i)
            pairs.append((ab[:old], ab[old:]))
        wants = _wants(ref, torch, T, pairs)
        good = Case(ref, torch, T, pairs)
        whole = _index_of(ref, torch, good.views, T, good.sizes)
        at0 = (2 + 1) + (3 + 1)  # frame 2's entries start behind those of frames 0 (2 superblocks) and 1 (3)
        frame2 = good.bufs[2].view[:good.sizes[2]].clone()
        csize = good.sizes[2]
        offs = whole[at0:at0 + 4]
        assert offs[0] == 8 and offs[3] == csize

        def failed(code, index=None, caps=None, frame=None, size=None, **kw):
            caps = [None] * 4 if caps is None else caps
            case = Case(ref, torch, T, pairs, caps=caps)
            sizes = list(case.sizes)
            if frame is not None:
                case.bufs[2] = Buf(torch, case.bufs[2].cap, frame)
                sizes[2] = frame.numel() if size is None else size
            d_idx = torch.tensor(index, dtype=torch.int64, device="cuda") if index is not None else None
            r, results = case.raw(st, d_idx.data_ptr() if index is not None else None, sizes=sizes, **kw)
            assert r == code, (hex(r), hex(code))
            assert case.unchanged(), "a refused call wrote to a buffer"
            assert results == [77] * 4, "a refused call wrote to results[]"
            assert st.last_frames_index() == (None, 0)
            return case

        # capacity exact succeeds; one byte short is refused, with and without an index
        case = Case(ref, torch, T, pairs, caps=[None, None, wants[2].size, None])
        _check(case, st, ref, st.append_batch(case.views, T, case.sizes, case.srcs), wants)
        for index in (None, whole):
            failed(DST_OVERFLOW, index=index, caps=[None, None, wants[2].size - 1, None])
        # each bad index entry of the single call's test (keep = 2, r > 0: entries 2 and 3 of frame 2 are the ones the call uses)
        for at, value, code in ((2, 7, INVALID_INPUT), (3, offs[2] + 3, INVALID_INPUT), (3, offs[2] - 1, INVALID_INPUT), (3, csize + 1, SRC_OVERFLOW),
                                (2, csize - 3, INVALID_INPUT), (2, 2**63 - 1, INVALID_INPUT)):
            idx = list(whole)
            idx[at0 + at] = value
            failed(code, index=idx)
        # the partial last superblock cut short, with and without an index
        for index in (whole, None):
            failed(SRC_OVERFLOW, index=index, frame=frame2[:csize - 10])
        # a bad code, and a block stream that ends too early
        bad = frame2.clone()
        bad[offs[2]] = bad[offs[2]] ^ 0xFF
        failed(INVALID_INPUT, index=whole, frame=bad)
        bad = frame2.clone()
        bad[offs[2] + 1:offs[2] + 4] = torch.tensor([7, 0, 0], dtype=torch.uint8, device="cuda")
        failed(INVALID_INPUT, index=whole, frame=bad)
        # a frame header stenos_hip_decompress refuses
        bad = frame2.clone()
        bad[0] = 9
        failed(INVALID_INPUT, frame=bad)
        # the context: levels 2 and 9, a time limit, a pending _async job
        for level in (2, 9):
            st.lib.stenos_set_level(st.ctx, level)
            failed(INVALID_PARAMETER)
        st.lib.stenos_set_level(st.ctx, 1)
        st.lib.stenos_set_max_nanoseconds(st.ctx, 10**9)
        failed(INVALID_PARAMETER)
        st.lib.stenos_set_max_nanoseconds(st.ctx, 0)
        other = torch.zeros(st.bound(1000), dtype=torch.uint8, device="cuda")
        pending = torch.from_numpy(pairs[3][0]).cuda()
        st.compress(pending, T, other, wait=False)
        failed(INVALID_PARAMETER)
        assert st.finish() == good.sizes[3]
        # overlapping buffers: two frame buffers, a source inside a frame buffer; capacity < size; T
        probe = Case(ref, torch, T, pairs)
        ptrs = [b.view.data_ptr() for b in probe.bufs]
        for kw in (dict(frames=[ptrs[0], ptrs[1], ptrs[1] + probe.bufs[1].cap - 1, ptrs[3]]), dict(srcs=[probe.srcs[0], probe.srcs[1], (ptrs[3] + 5, 100), probe.srcs[3]]),
                   dict(caps=[probe.bufs[0].cap, probe.bufs[1].cap, csize - 1, probe.bufs[3].cap]), dict(T=0), dict(T=65), dict(T=1)):
            r, results = probe.raw(st, **kw)
            assert r == INVALID_PARAMETER and results == [77] * 4 and probe.unchanged(), kw
            assert st.last_frames_index() == (None, 0)
        # and the context still works
        case = Case(ref, torch, T, pairs)
        _check(case, st, ref, st.append_batch(case.views, T, case.sizes, case.srcs), wants)
    finally:
        st.close()
        ref.close()


def test_superblocks_in_front_are_not_checked():
    """a byte flipped in the payload of superblock 0 of one frame: the call succeeds and the byte arrives unchanged"""
    torch = _cuda()
    st, ref = Stenos(level=1), Stenos(level=1)
    try:
        T, sb = 4, _sb(4)
        pairs = []
        for i, (old, new) in enumerate(((sb + 5, 99), (2 * sb + 700, 1234), (300, sb))):
            ab = _data("walk", T, old + new, 8 + i)
            pairs.append((ab[:old], ab[old:]))
        wants = _wants(ref, torch, T, pairs)
        at = 8 + 4 + 100
        for with_index in (True, False):
            case = Case(st, torch, T, pairs)
            p = st.frames_index(case.views, T, case.sizes)[0] if with_index else None
            flipped = Buf(torch, case.bufs[1].cap, case.bufs[1].view[:case.sizes[1]])
            flipped.view[at] = flipped.view[at] ^ 0x55
            flipped.before = flipped.buf.cpu().numpy()
            case.bufs[1] = flipped
            results = st.append_batch(case.views, T, case.sizes, case.srcs, p)
            assert results == [w.size for w in wants]
            wants[1][at] ^= 0x55
            for b, w in zip(case.bufs, wants):
                b.holds(w)
            wants[1][at] ^= 0x55
    finally:
        st.close()
        ref.close()


def test_a_foreign_frame_in_the_batch():
    """a level-2 frame from the host-pointer call (zstd-based codes in every superblock) among level-1 frames of the same superblock
    size: its superblocks 0 .. keep are unchanged and its decode is A||B; the others are the compressions of their concatenations"""
    torch = _cuda()
    st, ref, host = Stenos(level=1), Stenos(level=1), Stenos(level=2)
    try:
        T, sb = 4, _sb(4)
        old, new = 2 * sb + 300, sb + 500
        data = _mixed_data(T, old, sb, 6)
        cap = host.bound(old)
        dst = np.zeros(cap, dtype=np.uint8)
        r = host.lib.stenos_compress_generic(host.ctx, data.ctypes.data, T, old, dst.ctypes.data, cap)
        assert r < E(100), hex(r)
        frame_np = dst[:r].copy()
        assert frame_np[0] == 0  # (level 2 does not shift: the superblock size of the level-1 frames)
        B = _data("walk", T, new, 9)
        pairs = [(_data("walk", T, sb + 77, 1), _data("rand", T, 500, 2)), (data, B), (_data("sine", T, 3 * sb, 3), _data("walk", T, 100, 4))]
        wants = _wants(ref, torch, T, [pairs[0], pairs[2]])
        case = Case(st, torch, T, pairs)
        foreign = Buf(torch, frame_np.size + st.bound(old + new), torch.from_numpy(frame_np).cuda())
        case.bufs[1], case.sizes[1] = foreign, frame_np.size
        old_index = ref.frame_index(foreign.view, T, frame_np.size)
        keep = old // sb
        results = st.append_batch(case.views, T, case.sizes, case.srcs)
        assert [results[0], results[2]] == [w.size for w in wants]
        case.bufs[0].holds(wants[0])
        case.bufs[2].holds(wants[1])
        r = results[1]
        got = foreign.buf.cpu().numpy()
        end = max(r, frame_np.size)  # (behind a new frame that is shorter than the old one, the old one's bytes are still there)
        assert (got[:foreign.at] == GUARD_BYTE).all() and (got[foreign.at + end:] == GUARD_BYTE).all()
        assert np.array_equal(got[foreign.at + r:foreign.at + end], frame_np[r:end])
        got = got[foreign.at:foreign.at + r]
        p = old_index[keep]
        assert np.array_equal(got[8:p], frame_np[8:p]) and got[0] == frame_np[0]
        assert int.from_bytes(bytes(got[1:8]), "little") == old + new
        lp, ln = st.last_frames_index()
        assert _download(torch, lp, ln) == _index_of(ref, torch, case.views, T, results)
        assert np.array_equal(_decode(ref, torch, foreign.view, T, r, old + new), np.concatenate([data, B]))
    finally:
        st.close()
        ref.close()
        host.close()


def test_offsets_beyond_4_gib():
    """two frames, one of them a full-entropy array just beyond 4 GiB (stored as copies, so p >= 2^32); 1 MiB + 5 bytes appended to each"""
    torch = _cuda()
    GIB, SB, P32 = 1 << 30, 131072, 1 << 32
    torch.cuda.empty_cache()
    if torch.cuda.mem_get_info()[0] < 16 * GIB:
        pytest.skip("needs 16 GiB of free device memory")
    T, old, new = 4, P32 + 3 * SB + 1000, (1 << 20) + 5
    st, ref = Stenos(level=1), Stenos(level=1)
    src = whole = None
    try:
        g = torch.Generator(device="cuda")
        g.manual_seed(82)
        src = torch.empty(old + new, dtype=torch.uint8, device="cuda")
        for o in range(0, old + new, GIB):
            n = min(GIB, old + new - o)
            src[o:o + n] = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda", generator=g)
        at, cap = 256 + 5, st.bound(old + new)
        whole = torch.full((at + cap + 64 + 16,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
        view = whole[at:at + cap]
        first = torch.empty(st.bound(old), dtype=torch.uint8, device="cuda")
        csize = st.compress(src[:old], T, first)
        view[:csize] = first[:csize]
        del first
        small_old = 2 * SB + 999
        small = _data("walk", T, small_old + new, 4)
        case = Case(st, torch, T, [(small[:small_old], small[small_old:])])
        want_small = _wants(ref, torch, T, case.pairs)[0]
        keep = old // SB
        views, sizes = [case.bufs[0].view, view], [case.sizes[0], csize]
        p, n = st.frames_index(views, T, sizes)
        old_index = _download(torch, p, n)
        big0 = 3 + 1  # the big frame's entries start behind the small frame's (3 superblocks)
        assert n == 3 + keep + 1 + 2 and old_index[big0 + keep] >= P32
        torch.cuda.synchronize()
        results = st.append_batch(views, T, sizes, [case.srcs[0], src[old:]], p)
        r = results[1]
        assert results[0] == want_small.size and r > csize
        case.bufs[0].holds(want_small)  # (the guards behind the small frame)
        for o in range(at + r, whole.numel(), GIB):
            assert bool((whole[o:o + GIB] == GUARD_BYTE).all().item()), "a byte behind the returned size changed"
        lp, ln = st.last_frames_index()
        new_index = _download(torch, lp, ln)
        nsb_small = -(-(small_old + new) // SB)
        big1 = nsb_small + 1
        assert new_index[:big1] == ref.frame_index(case.bufs[0].view, T, results[0])
        want_index = ref.frame_index(view, T, r)
        assert new_index[big1:] == want_index and new_index[big1:big1 + keep + 1] == old_index[big0:big0 + keep + 1]
        assert all(x > P32 for x in new_index[big1 + keep:]) and new_index[-1] == r
        span = 2 << 20
        out = torch.zeros(span, dtype=torch.uint8, device="cuda")
        assert ref.decompress_range(view, T, r, old + new - span, span, out) == span
        assert torch.equal(out, src[old + new - span:])
    finally:
        st.close()
        ref.close()
        del src, whole
        torch.cuda.empty_cache()
