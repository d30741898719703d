"""Rows of many frames on the device replaced in one call by device-resident (frame number, row number) pairs (include/stenos_hip.h:
stenos_hip_update_rows_batch).  The oracle is exact: every output frame is, byte for byte and in size, the frame stenos_hip_compress
makes of the numpy-updated array (through a second context of the same settings), and what stenos_hip_update_rows gives for that
frame alone.  All or nothing: after any failure every output is still 0xA5.  The context's index is the new frames' afterwards.

All frames of a call share one geometry: the default superblock, and stenos_set_block_size(ctx, 2) (four blocks per superblock);
both have their own batch.  The outputs are pre-filled with 0xA5, misaligned by 5 and compared whole (Out of test_gpu_update.py)."""
import numpy as np
import pytest

from stenos_amd.api import Stenos
from test_gpu_gather import _row_sizes, _rows_tensor
from test_gpu_gather_batch import Batch, _device_words, pair_set
from test_gpu_ranges import _mixed_data, _sb, _sizes
from test_gpu_update import DST_OVERFLOW, INVALID_INPUT, INVALID_PARAMETER, SRC_OVERFLOW, TS, Out, _code, _sources

pytestmark = pytest.mark.gpu

SHIFT = 2  # the small custom superblock: four blocks


def _cuda():
    import torch

    assert torch.cuda.is_available()
    return torch


def _ctx(shift, level=1, lib=None):
    st = Stenos(level=level, lib=lib)
    if shift is not None:
        assert st.lib.stenos_set_block_size(st.ctx, shift) == 0
    return st


def make_batch(torch, T, shift, seed=0):
    """eight frames of one geometry, made partly by compress and partly by compress_batch: 0: 2 superblocks + 300 bytes, 1: one
    superblock, 2: a last superblock under 128 bytes (the host path), 3: an empty array, 4: exactly 2 superblocks, 5: 4 superblocks,
    6: frame 0 listed again, 7: 3 superblocks and a partial block"""
    sb = _sb(T, shift)
    s = _sizes(T, sb)
    st = _ctx(shift)
    try:
        bt = Batch()
        bt.add_single(st, torch, T, _mixed_data(T, s[1], sb, seed + 1), sb)
        bt.add_batch(st, torch, T, [_mixed_data(T, s[0], sb, seed + 2), _mixed_data(T, s[2], sb, seed + 3)], sb)
        bt.add_empty(torch)
        bt.add_single(st, torch, T, _mixed_data(T, s[4], sb, seed + 4), sb)
        bt.add_batch(st, torch, T, [_mixed_data(T, 4 * sb, sb, seed + 5)], sb)
        bt.add(bt.frames[0], bt.csizes[0], bt.datas[0], sb)
        bt.add_batch(st, torch, T, [_mixed_data(T, s[3], sb, seed + 7)], sb)
        return bt
    finally:
        st.close()


def unique_pairs(fids, rows):
    """the pairs without their repetitions, in the order of their first appearance"""
    key = np.asarray(fids, dtype=np.int64) * (1 << 40) + np.asarray(rows, dtype=np.int64)
    _, first = np.unique(key, return_index=True)
    first.sort()
    return np.asarray(fids, dtype=np.int64)[first], np.asarray(rows, dtype=np.int64)[first]


def updated_arrays(bt, row_bytes, fids, rows, src_rows):
    out = [d.copy() for d in bt.datas]
    col = np.arange(row_bytes, dtype=np.int64)
    for f in range(bt.m):
        mine = np.flatnonzero(np.asarray(fids) == f)
        if mine.size:
            out[f][(np.asarray(rows, dtype=np.int64)[mine] * row_bytes)[:, None] + col] = src_rows[mine]
    return out


def caps(bt, st):
    return [f.numel() + 64 for f in bt.frames]


def run_update(st, torch, bt, T, row_bytes, fids, rows, src_t, outs, index_ptr=None, stride=None, src_ptr=None):
    n = len(rows)
    return st.update_rows_batch(bt.frames, T, bt.csizes, row_bytes, _rows_tensor(torch, fids) if n else None, _rows_tensor(torch, rows) if n else None,
                                src_ptr if src_ptr is not None else src_t, [o.view for o in outs], index_ptr, stride)


def reference_frames(ref, torch, T, bt, want):
    """stenos_hip_compress of every updated array (the frame of the empty array is its input: 8 bytes)"""
    frames = []
    for f, d in enumerate(want):
        if d.size == 0:
            frames.append(bt.frames[f][:bt.csizes[f]].cpu().numpy())
            continue
        dst = torch.zeros(bt.frames[f].numel(), dtype=torch.uint8, device="cuda")
        r = ref.compress(torch.from_numpy(d).cuda(), T, dst)
        frames.append(dst[:r].cpu().numpy())
    return frames


def check_outputs(outs, sizes, frames, what):
    for f, (o, r, want) in enumerate(zip(outs, sizes, frames)):
        got = o.frame(r)
        assert r == want.size, (what, f, r, want.size)
        if not np.array_equal(got, want):
            raise AssertionError(f"{what}: byte {int(np.flatnonzero(got != want)[0])} of frame {f} differs")


def all_untouched(outs):
    return all(o.untouched() for o in outs)


@pytest.mark.parametrize("T", TS)
def test_parity(T):
    torch = _cuda()
    cases, strides = 0, set()
    for shift in (None, SHIFT):
        bt = make_batch(torch, T, shift)
        st, single, ref, other = (_ctx(shift) for _ in range(4))
        try:
            sb = _sb(T, shift)
            rng = np.random.default_rng([81, T, shift or 9])
            for row_bytes in _row_sizes(T, sb, max(d.size for d in bt.datas)):
                fa, ra = unique_pairs(*pair_set(bt, row_bytes, rng))
                assert np.unique(fa).size >= 2
                if sb // row_bytes >= 66:  # exactly 64 and 65 rows of one interior superblock are among them
                    first = -(-sb // row_bytes)
                    assert {(5, first + k) for k in range(65)} <= set(zip(fa.tolist(), ra.tolist()))
                inside = np.flatnonzero(fa == 5)
                for name, (fids, rows) in (("all", (fa, ra)), ("none", (fa[:0], ra[:0])), ("one frame", (fa[inside], ra[inside]))):
                    n = len(rows)
                    strided = cases % 2 == 1 and n * (row_bytes + 67) <= 32 << 20  # (sources 67 bytes apart, 3 bytes off their alignment)
                    stride, mis = (row_bytes + 67, 3) if strided else (row_bytes, 0)
                    strides.add(stride != row_bytes)
                    src_np, src_rows = _sources(rng, n, row_bytes, stride, mis)
                    src_t = torch.from_numpy(src_np).cuda()
                    want = updated_arrays(bt, row_bytes, fids, rows, src_rows)
                    frames = reference_frames(ref, torch, T, bt, want)
                    outs = [Out(torch, c) for c in caps(bt, st)]
                    sizes = run_update(st, torch, bt, T, row_bytes, fids, rows, src_t, outs, None, stride, src_t.data_ptr() + mis)
                    check_outputs(outs, sizes, frames, (shift, row_bytes, name, "against compress"))
                    # ... and what stenos_hip_update_rows gives, frame by frame
                    for f in range(bt.m):
                        mine = np.flatnonzero(fids == f)
                        o = Out(torch, outs[f].cap)
                        s_rows = np.ascontiguousarray(src_rows[mine]).reshape(-1)
                        r = single.update_rows(bt.frames[f], T, bt.csizes[f], row_bytes, _rows_tensor(torch, rows[mine]) if mine.size else None,
                                               torch.from_numpy(s_rows).cuda() if mine.size else None, o.view)
                        assert r == sizes[f] and np.array_equal(o.frame(r), outs[f].frame(r)), (shift, row_bytes, name, f)
                    # the context's index is the new frames'
                    p, entries = st.last_frames_index()
                    views = [o.view for o in outs]
                    q, entries2 = other.frames_index(views, T, sizes)
                    assert p and entries == entries2 and _device_words(p, entries) == _device_words(q, entries2), (shift, row_bytes, name)
                    assert st.last_index() == (None, 0)
                    if n:  # a gather on the outputs with that pointer returns the updated rows
                        b2 = Batch()
                        for v, r, d in zip(views, sizes, want):
                            b2.add(v, r, d, sb)
                        b2.gather(st, torch, T, row_bytes, fids.tolist(), rows.tolist(), p)
                    cases += 1
        finally:
            for s in (st, single, ref, other):
                s.close()
    assert cases >= 18 and strides == {True, False}


@pytest.mark.parametrize("row_bytes", [1, 300, 4096 + 5])
def test_repeated_pairs(row_bytes):
    """different sources for one pair: every piece (a row cut at superblock boundaries) is one of its candidates, whole.  Every
    source row carries a marker of its own in all its bytes, so a piece mixed from two sources would show"""
    torch = _cuda()
    T = 4
    bt = make_batch(torch, T, None, seed=20)
    st, ref = _ctx(None), _ctx(None)
    try:
        sb, rb = _sb(T), row_bytes
        rng = np.random.default_rng([82, rb])
        uniq = []
        for f in (0, 5, 6, 7):
            nrows = bt.datas[f].size // rb
            straddler = sb // rb if sb % rb else 5
            uniq += [(f, straddler), (f, 0), (f, nrows - 1)] + [(f, int(r)) for r in rng.integers(0, nrows, 12)]
        pick = rng.integers(0, len(uniq), 600)  # (more than 64 pieces in a superblock: several chunks)
        fids = np.array([uniq[i][0] for i in pick])
        rows = np.array([uniq[i][1] for i in pick])
        src_rows = np.repeat((np.arange(len(rows)) % 251).astype(np.uint8)[:, None], rb, axis=1)  # source i: the byte i % 251 throughout
        outs = [Out(torch, c) for c in caps(bt, st)]
        sizes = run_update(st, torch, bt, T, rb, fids, rows, torch.from_numpy(src_rows.reshape(-1)).cuda(), outs)
        for f in range(bt.m):
            d = bt.datas[f]
            if d.size == 0:
                continue
            back = torch.zeros(d.size, dtype=torch.uint8, device="cuda")
            assert ref.decompress(outs[f].view, T, sizes[f], back) == d.size
            back = back.cpu().numpy()
            covered = np.zeros(d.size, dtype=bool)
            for row in set(rows[fids == f].tolist()):
                cands = {int(src_rows[i][0]) for i in np.flatnonzero((fids == f) & (rows == row))}
                lo, hi = row * rb, (row + 1) * rb
                covered[lo:hi] = True
                cuts = [lo] + [b for b in range(sb, d.size, sb) if lo < b < hi] + [hi]
                for a, b in zip(cuts, cuts[1:]):
                    piece = back[a:b]
                    assert (piece == piece[0]).all() and int(piece[0]) in cands, (f, row, a, b)
            assert np.array_equal(back[~covered], d[~covered]), f
    finally:
        st.close()
        ref.close()


def _damage_touched(torch, bt, f, st, T):
    """frame f with the code byte of its superblock 0 damaged"""
    offs = st.frame_index(bt.frames[f], T, bt.csizes[f])
    bad = bt.frames[f].clone()
    bad[offs[0]] = bad[offs[0]] ^ 0xFF
    return bad


def test_invalid_pairs():
    torch = _cuda()
    T, rb = 4, 64
    bt = make_batch(torch, T, None, seed=30)
    st, aux = _ctx(None), _ctx(None)
    try:
        rng = np.random.default_rng(83)
        ok = [(0, 1), (5, 7), (7, 3), (1, 0)]
        src_np, _ = _sources(rng, 8, rb, rb)
        src = torch.from_numpy(src_np).cuda()
        nrows1 = bt.datas[1].size // rb
        cases = {"frame m": (bt.m, 0), "frame 2^32 + a valid one": ((1 << 32) + 5, 0), "row at the bound": (1, nrows1), "the empty frame": (3, 0)}
        for name, bad in cases.items():
            pairs = ok[:2] + [bad] + ok[2:]
            outs = [Out(torch, c) for c in caps(bt, st)]
            r = _code(lambda: run_update(st, torch, bt, T, rb, [f for f, _ in pairs], [x for _, x in pairs], src, outs))
            assert r == INVALID_PARAMETER and all_untouched(outs), name
        # with a damaged touched superblock in addition: the invalid pair wins
        frames = list(bt.frames)
        bt.frames[7] = _damage_touched(torch, bt, 7, aux, T)
        pairs = ok + [(bt.m, 0)]
        outs = [Out(torch, c) for c in caps(bt, st)]
        r = _code(lambda: run_update(st, torch, bt, T, rb, [f for f, _ in pairs], [x for _, x in pairs], src, outs))
        assert r == INVALID_PARAMETER and all_untouched(outs)
        outs = [Out(torch, c) for c in caps(bt, st)]
        r = _code(lambda: run_update(st, torch, bt, T, rb, [f for f, _ in ok], [x for _, x in ok], src, outs))
        assert r == INVALID_INPUT and all_untouched(outs)
        bt.frames[:] = frames
        # and the context still works
        outs = [Out(torch, c) for c in caps(bt, st)]
        sizes = run_update(st, torch, bt, T, rb, [f for f, _ in ok], [x for _, x in ok], src, outs)
        assert all(o.frame(r).size == r for o, r in zip(outs, sizes))
    finally:
        st.close()
        aux.close()


def test_failures_write_nothing_anywhere():
    torch = _cuda()
    T, rb = 4, 64
    bt = make_batch(torch, T, None, seed=40)
    st, aux = _ctx(None), _ctx(None)
    try:
        sb = _sb(T)
        rng = np.random.default_rng(84)
        pairs = [(0, 1), (5, sb // rb + 2), (7, 3), (2, bt.datas[2].size // rb - 1), (6, 9)]
        fids, rows = [f for f, _ in pairs], [x for _, x in pairs]
        src_np, _ = _sources(rng, len(pairs), rb, rb)
        src = torch.from_numpy(src_np).cuda()

        def call(b=bt, cap=None, index_ptr=None, ctx=st, f=fids, r=rows):
            outs = [Out(torch, c) for c in (cap or caps(b, ctx))]
            return _code(lambda: run_update(ctx, torch, b, T, rb, f, r, src, outs, index_ptr)), outs

        good, good_outs = call()
        assert isinstance(good, list)
        # one output one byte short of its new size, the others ample
        for f in (0, 3, 7):
            cap = caps(bt, st)
            cap[f] = good[f] - 1
            r, outs = call(cap=cap)
            assert r == DST_OVERFLOW and all_untouched(outs), f
        cap = list(good)
        r, outs = call(cap=cap)  # exactly the new sizes
        assert r == good
        check_outputs(outs, r, [o.frame(s).copy() for o, s in zip(good_outs, good)], "exact capacities")
        # mixed superblock sizes in one call
        small = _ctx(SHIFT)
        try:
            mixed = Batch()
            for k in range(3):
                mixed.add(bt.frames[k], bt.csizes[k], bt.datas[k], sb)
            mixed.add_single(small, torch, T, _mixed_data(T, 3 * _sb(T, SHIFT) + 40, _sb(T, SHIFT), 1), _sb(T, SHIFT))
            r, outs = call(b=mixed, f=[0, 1], r=[1, 0])
            assert r == INVALID_PARAMETER and all_untouched(outs)
        finally:
            small.close()
        # a level-2 context; a time limit
        hi = _ctx(None, level=2)
        try:
            r, outs = call(ctx=hi)
            assert r == INVALID_PARAMETER and all_untouched(outs)
        finally:
            hi.close()
        # a pending _async job: refused, and the job is left alone
        other = torch.zeros(st.bound(bt.datas[5].size), dtype=torch.uint8, device="cuda")
        st.compress(torch.from_numpy(bt.datas[5]).cuda(), T, other, wait=False)
        r, outs = call()
        assert r == INVALID_PARAMETER and all_untouched(outs)
        assert st.finish() == bt.csizes[5]
        # a damaged touched superblock in the last frame: the decoder's code
        frames = list(bt.frames)
        bt.frames[7] = _damage_touched(torch, bt, 7, aux, T)
        r, outs = call()
        assert r == INVALID_INPUT and all_untouched(outs)
        # the same damage where no pair touches: not seen, and it arrives in the output byte for byte
        r, outs = call(f=fids[:2], r=rows[:2])
        assert isinstance(r, list) and np.array_equal(outs[7].frame(r[7]), bt.frames[7][:bt.csizes[7]].cpu().numpy())
        bt.frames[:] = frames
        # bad index entries in the first, a middle and the last frame: a decreasing offset, a superblock under 4 bytes, a last
        # entry past the frame, an entry far outside its frame (where another frame may lie)
        p, entries = aux.frames_index(bt.frames, T, bt.csizes)
        idx = _device_words(p, entries)
        first = np.cumsum([0] + [-(-d.size // sb) for d in bt.datas])
        for f in (0, 5, 7):
            at = int(first[f]) + f  # frame f's entry of superblock 0; its last entry is at first[f + 1] + f
            end = int(first[f + 1]) + f
            for name, k, value, code in (("decreasing", at + 1, idx[at] - 1, INVALID_INPUT), ("under 4 bytes", at + 1, idx[at] + 3, INVALID_INPUT),
                                         ("past the frame", end, bt.csizes[f] + 1, SRC_OVERFLOW), ("far outside", at + 1, idx[at] + (1 << 30), None)):
                bad = list(idx)
                bad[k] = value
                d_idx = torch.tensor(bad, dtype=torch.int64, device="cuda")
                r, outs = call(index_ptr=d_idx.data_ptr(), f=[0, 5, 7], r=[1, 2, 3])  # (superblock 0 of each: the damage is the index's alone)
                assert r in ((code,) if code else (INVALID_INPUT, SRC_OVERFLOW)) and all_untouched(outs), (f, name, r if not isinstance(r, list) else "ran")
        # and the context still works
        r, outs = call()
        assert r == good
    finally:
        st.close()
        aux.close()


def test_index_forms():
    """no index; the pointer of frames_index, the context's own, twice in a row; a caller's device copy: the same outputs"""
    torch = _cuda()
    T, rb = 4, 300
    bt = make_batch(torch, T, None, seed=50)
    st = _ctx(None)
    try:
        rng = np.random.default_rng(85)
        fids, rows = unique_pairs(*pair_set(bt, rb, rng))
        fids, rows = fids[:700], rows[:700]
        src_np, _ = _sources(rng, len(rows), rb, rb)
        src = torch.from_numpy(src_np).cuda()
        results = []

        def call(index_ptr):
            outs = [Out(torch, c) for c in caps(bt, st)]
            sizes = run_update(st, torch, bt, T, rb, fids, rows, src, outs, index_ptr)
            results.append((sizes, [o.frame(r).copy() for o, r in zip(outs, sizes)]))

        call(None)
        for _ in range(2):
            p, entries = st.frames_index(bt.frames, T, bt.csizes)
            call(p)
        p, entries = st.frames_index(bt.frames, T, bt.csizes)
        mine = torch.tensor(_device_words(p, entries), dtype=torch.int64, device="cuda")
        call(mine.data_ptr())
        for sizes, frames in results[1:]:
            assert sizes == results[0][0] and all(np.array_equal(a, b) for a, b in zip(frames, results[0][1]))
    finally:
        st.close()


def test_long_chains():
    """a frame of 300 superblocks at block-size setting 0 takes the parallel walk, beside short frames, with no index; more than
    1 024 superblocks in the batch and more than 1 024 of them touched"""
    torch = _cuda()
    T, rb = 4, 100
    sb = _sb(T, 0)
    make, st, ref = _ctx(0, level=0), _ctx(0), _ctx(0)
    try:
        rng = np.random.default_rng(86)
        bt = Batch()
        for nsb in (300, 250, 250, 250, 3):
            bt.add_single(make, torch, T, rng.integers(0, 256, nsb * sb + 20, dtype=np.uint8), sb)
        bt.add_empty(torch)
        fids = np.concatenate([np.full(d.size // rb, f, dtype=np.int64) for f, d in enumerate(bt.datas)])
        rows = np.concatenate([np.arange(d.size // rb, dtype=np.int64) for d in bt.datas])
        keep = rng.permutation(rows.size)[:rows.size // 2]  # (every other row: every superblock is touched)
        fids, rows = fids[keep], rows[keep]
        assert sum(-(-d.size // sb) for d in bt.datas) > 1024
        src_np, src_rows = _sources(rng, len(rows), rb, rb)
        want = updated_arrays(bt, rb, fids, rows, src_rows)
        outs = [Out(torch, c) for c in caps(bt, st)]
        sizes = run_update(st, torch, bt, T, rb, fids, rows, torch.from_numpy(src_np).cuda(), outs)
        for f, d in enumerate(want):
            if d.size == 0:
                assert np.array_equal(outs[f].frame(sizes[f]), bt.frames[f][:8].cpu().numpy())
                continue
            back = torch.zeros(d.size, dtype=torch.uint8, device="cuda")
            assert ref.decompress(outs[f].view, T, sizes[f], back) == d.size
            assert np.array_equal(back.cpu().numpy(), d), f
            dst = torch.zeros(bt.frames[f].numel(), dtype=torch.uint8, device="cuda")
            r = ref.compress(torch.from_numpy(d).cuda(), T, dst)
            assert r == sizes[f] and np.array_equal(dst[:r].cpu().numpy(), outs[f].frame(r)), f
    finally:
        for s in (make, st, ref):
            s.close()


def test_pairs_and_sources_made_on_the_stream_need_no_synchronisation():
    torch = _cuda()
    T, rb, n = 8, 512, 150
    bt = make_batch(torch, T, None, seed=60)
    st, ref = _ctx(None), _ctx(None)
    try:
        nrows = min(bt.datas[f].size // rb for f in (0, 5, 7))
        assert 2 * n < nrows
        s = torch.cuda.Stream()
        busy = torch.zeros(32 << 20, dtype=torch.float32, device="cuda")
        seed = torch.arange(n * rb, dtype=torch.int64, device="cuda")
        base = torch.arange(n, dtype=torch.int64, device="cuda")
        choice = torch.tensor([0, 5, 7], dtype=torch.int64, device="cuda")
        outs = [Out(torch, c) for c in caps(bt, st)]
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            for _ in range(100):
                busy.add_(1.0)
            rows_t = torch.flip(base, [0]) * 2 + 1  # (unique per frame, below 2 n < nrows)
            fids_t = choice[base % 3].contiguous()
            src_t = ((seed * 2654435761) >> 7).to(torch.uint8)
            sizes = st.update_rows_batch(bt.frames, T, bt.csizes, rb, fids_t, rows_t, src_t, [o.view for o in outs])
        torch.cuda.synchronize()
        fids, rows = fids_t.cpu().numpy(), rows_t.cpu().numpy()
        want = updated_arrays(bt, rb, fids, rows, src_t.cpu().numpy().reshape(n, rb))
        check_outputs(outs, sizes, reference_frames(ref, torch, T, bt, want), "stream order")
    finally:
        st.close()
        ref.close()
