"""History independence of a context (include/stenos_hip.h): whatever ran on a stenos_context before, a call returns, writes and
leaves behind exactly what the header promises for that call alone.  One context lives through the 197 steps of
tests/context_history.py -- every ordered pair of the 14 classes of calls once, large calls in front of small ones, three index
forms, three streams, failing calls in between -- on a store of 14 frames in three groups.  The oracle is a second context made
fresh for every step and closed after it: expected frames are its stenos_hip_compress of the model's arrays, expected indices its
stenos_hip_frame_index; reads are compared with numpy slices of the model.

After every step: the return values; every destination whole, with its guard bytes (Carved, Slots, Buf of the existing tests);
every frame the step wrote, byte for byte, in a buffer that is compared whole; after a failing call every buffer as it was and
results[] untouched; the context's index where the header promises one (stenos_hip_last_index after compress, update and append,
and after ranges and gather calls that were given it; NULL after compress_batch, decompress_batch, update_rows_batch and
append_batch; stenos_hip_last_frames_index after frames_index, update_rows_batch and append_batch, NULL after their failures);
and whenever stenos_hip_last_frames_index gives a pointer, its entries are those of the many-frame call it stems from.  Nothing is
asserted where the header leaves the index unspecified; after an invalid row in a gather call the header leaves the other slots
unspecified, so there the gaps, the guards and the invalid row's slot are checked.  About every 20 steps and at the end every frame
of the store decodes on the long-lived context to its model array and equals a fresh compression.

A failure names the step and prints the list of (class, regime, group, frame) up to it; test_replay runs such a list."""
import contextlib
import ctypes
from ctypes import c_size_t, c_void_p
from functools import lru_cache

import numpy as np
import pytest

import context_history as ch
from stenos_amd.api import Stenos, StenosError
from test_gpu_append import GUARD, GUARD_BYTE, Buf, _download, _src
from test_gpu_gather import Slots, _rows_tensor
from test_gpu_ranges import Carved

pytestmark = pytest.mark.gpu

AUDIT_EVERY = 20


def _cuda():
    import torch

    assert torch.cuda.is_available()
    return torch


def _code(call):
    try:
        return call()
    except StenosError as err:
        return err.code


@lru_cache(maxsize=None)
def _initial_model():
    return ch.Model()


class Frame:
    """a frame of the store: the Buf it lies in, its size, its bytes as a fresh context made them; its index, made by a fresh context
    when first asked for (the bytes on the device have been compared with `want` by then)"""

    def __init__(self, buf, csize, want):
        self.buf, self.csize, self.want, self._index = buf, csize, want, None

    @property
    def view(self):
        return self.buf.view

    def index(self, ref, T):
        if self._index is None:
            self._index = [8] if self.want.size == 8 else ref.frame_index(self.buf.view, T, self.csize)  # (an empty array: one entry, its end)
        return self._index


def _guarded(torch, n):
    """n bytes with 64 guard bytes on both sides, all 0xA5: (the whole tensor, the view)"""
    whole = torch.full((n + 2 * GUARD,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
    return whole, whole[GUARD:GUARD + n]


def _is(whole, data):
    got = whole.cpu().numpy()
    return np.array_equal(got[GUARD:GUARD + data.size], data) and (got[:GUARD] == GUARD_BYTE).all() and (got[GUARD + data.size:] == GUARD_BYTE).all()


def _slots_hold(sl, expect, skip=None):
    """the slot buffer whole: the expected rows in their slots, 0xA5 everywhere else (and in the slot `skip`)"""
    want = np.full(sl.buf.numel(), GUARD_BYTE, dtype=np.uint8)
    at = (sl.at + np.arange(len(expect), dtype=np.int64) * sl.stride)[:, None] + np.arange(sl.row_bytes, dtype=np.int64)
    want[at] = expect
    got = sl.buf.cpu().numpy()
    if skip is not None:
        want[at[skip]] = GUARD_BYTE
    if not np.array_equal(got, want):
        bad = int(np.flatnonzero(got != want)[0])
        raise AssertionError(f"byte {bad} of the slot buffer differs (got {got[bad]}, want {want[bad]}): slot {(bad - sl.at) // sl.stride}")


class Run:
    def __init__(self, torch, level, lib=None):
        self.torch, self.level, self.lib = torch, level, lib
        self.st = Stenos(level, lib=lib)
        self.model = _initial_model().copy()
        self.streams = [None, torch.cuda.Stream(), torch.cuda.Stream()]
        self.many = None  # the entries of the last many-frame index a call on st made
        self.frames = {g: [None] * n for g, (_, n) in ch.GROUPS.items()}
        ref = self.fresh()
        try:
            for g, (T, n) in ch.GROUPS.items():
                for f in range(n):
                    arr = self.model.arrays[g][f]
                    want = self.want_frame(ref, arr, T)
                    if arr.size:
                        self.frames[g][f] = self.compressed(arr, T, want, lambda src, view: self.st.compress(src, T, view))
                    else:
                        self.frames[g][f] = Frame(Buf(torch, 16, torch.from_numpy(want).cuda()), 8, want)
        finally:
            ref.close()

    def close(self):
        self.st.close()

    def fresh(self, level=None):
        return Stenos(self.level if level is None else level, lib=self.lib)

    @contextlib.contextmanager
    def on(self, step):
        """the step's stream; what the test prepared on the default stream is there by then"""
        self.torch.cuda.synchronize()
        s = self.streams[step.stream]
        with (self.torch.cuda.stream(s) if s is not None else contextlib.nullcontext()):
            yield
        self.torch.cuda.synchronize()

    # --- the oracle
    def want_frame(self, ref, arr, T):
        if arr.size == 0:
            return np.zeros(8, dtype=np.uint8)  # (shift 0, size 0)
        dst = self.torch.zeros(ref.bound(arr.size), dtype=self.torch.uint8, device="cuda")
        r = ref.compress(self.torch.from_numpy(arr).cuda(), T, dst)
        return dst[:r].cpu().numpy()

    def truth(self, ref, T, frames):
        return [x for fr in frames for x in fr.index(ref, T)]

    def compressed(self, arr, T, want, call):
        """arr compressed by `call` into a new Buf of the bound's size: the frame equals `want`, nothing is written outside the
        destination (behind the frame and inside it the bytes are scratch)"""
        torch = self.torch
        src = torch.from_numpy(arr).cuda()
        buf = Buf(torch, self.st.bound(arr.size))
        r = call(src, buf.view)
        assert r == want.size, (r, want.size)
        got = buf.buf.cpu().numpy()
        assert np.array_equal(got[buf.at:buf.at + r], want), f"byte {int(np.flatnonzero(got[buf.at:buf.at + r] != want)[0])} of the frame differs"
        assert (got[:buf.at] == GUARD_BYTE).all() and (got[buf.at + buf.cap:] == GUARD_BYTE).all(), "a byte outside the destination changed"
        buf.before = got
        return Frame(buf, r, want)

    # --- what the context must hold
    def single_index_is(self, fr, ref, T):
        p, n = self.st.last_index()
        want = fr.index(ref, T)
        assert p and n == len(want) - 1, ("stenos_hip_last_index", p, n, len(want) - 1)
        assert _download(self.torch, p, n + 1) == want, "stenos_hip_last_index: the entries are not the frame's"

    def no_single_index(self):
        p, n = self.st.last_index()
        assert not p and n == 0, ("stenos_hip_last_index after a batch", p, n)

    def many_index_is(self, ref, T, frames):
        want = self.truth(ref, T, frames)
        p, n = self.st.last_frames_index()
        assert p and n == len(want), ("stenos_hip_last_frames_index", p, n, len(want))
        assert _download(self.torch, p, n) == want, "stenos_hip_last_frames_index: the entries are not the frames'"
        self.many = want

    def no_many_index(self):
        assert self.st.last_frames_index() == (None, 0), "a many-frame index after a failed call"
        self.many = None

    def invariant(self):
        p, n = self.st.last_frames_index()
        if p:
            assert self.many is not None, "a many-frame index that no call made"
            assert n == len(self.many) and _download(self.torch, p, n) == self.many, "a stale many-frame index is handed out"

    def index_arg(self, step, ref, T, frames):
        """d_index in the step's form: (pointer, what keeps it alive)"""
        if step.form == "null":
            return None, None
        if step.form == "own":
            if step.cls in ch.SINGLE_INDEX:
                p, n = self.st.last_index()
                want = frames[0].index(ref, T)
                assert p and n == len(want) - 1 and _download(self.torch, p, n + 1) == want, "the index the step before left is not the frame's"
            else:
                p, n = self.st.last_frames_index()
                want = self.truth(ref, T, frames)
                assert p and n == len(want) and _download(self.torch, p, n) == want, "the many-frame index the step before left is not the frames'"
            return p, None
        copy = self.torch.tensor(self.truth(ref, T, frames), dtype=self.torch.int64, device="cuda")
        return copy.data_ptr(), copy

    def unchanged(self, g):
        for f, fr in enumerate(self.frames[g]):
            assert fr.buf.unchanged(), f"frame {f} of group {g} or the bytes around it changed"

    # --- the steps
    def step(self, step):
        op = self.model.apply(step)
        ref = self.fresh()
        try:
            getattr(self, "_" + step.cls)(step, op, ref, ch.GROUPS[step.group][0])
            self.invariant()
        finally:
            ref.close()

    def _compress(self, step, op, ref, T, wait=True):
        g, f = step.group, step.frame
        arr = op["after"][f]
        want = self.want_frame(ref, arr, T)

        def call(src, view):
            with self.on(step):
                r = self.st.compress(src, T, view, wait=wait)
                if not wait:
                    assert r == 0
                    self.refused_while_pending(g, T)
                    r = self.st.finish()
            return r

        self.frames[g][f] = self.compressed(arr, T, want, call)
        self.single_index_is(self.frames[g][f], ref, T)

    def _compress_async(self, step, op, ref, T):
        self._compress(step, op, ref, T, wait=False)

    def refused_while_pending(self, g, T):
        """a batch call and a ranges call while the _async job is unfinished: refused, nothing written"""
        torch, st = self.torch, self.st
        fr = self.frames[g][ch.SLOTS[g]["large"][-1]]
        whole, view = _guarded(torch, 64)
        P, Z = c_void_p * 1, c_size_t * 1
        res = Z(77)
        r = st.lib.stenos_hip_decompress_batch(st.ctx, 1, T, P(fr.view.data_ptr()), Z(fr.csize), P(view.data_ptr()), Z(64), res, st._stream_ptr())
        assert r == ch.INVALID_PARAMETER and res[0] == 77, (hex(r), res[0])
        c = Carved(torch, [(0, 16), (5, 7)])
        assert _code(lambda: st.decompress_ranges(fr.view, T, fr.csize, c.ranges, c.ptrs)) == ch.INVALID_PARAMETER
        assert c.untouched() and bool((whole == GUARD_BYTE).all().item())

    def _batch(self, step, op, ref, T):
        torch, st, g = self.torch, self.st, step.group
        arrays = self.model.arrays[g]
        wants = [self.want_frame(ref, a, T) for a in arrays]
        srcs = [torch.from_numpy(a).cuda() if a.size else torch.empty(0, dtype=torch.uint8, device="cuda") for a in arrays]
        bufs = [Buf(torch, max(st.bound(a.size), 16)) for a in arrays]
        with self.on(step):
            results = st.compress_batch(srcs, T, [b.view for b in bufs])
        assert results == [w.size for w in wants], (results, [w.size for w in wants])
        for f, (b, w) in enumerate(zip(bufs, wants)):
            got = b.buf.cpu().numpy()
            assert np.array_equal(got[b.at:b.at + w.size], w), f"frame {f} of the batch differs"
            assert (got[:b.at] == GUARD_BYTE).all() and (got[b.at + b.cap:] == GUARD_BYTE).all(), f"frame {f}: a byte outside the destination changed"
            b.before = got
        self.no_single_index()
        assert st.last_frames_index() == (None, 0)
        outs = [_guarded(torch, a.size) for a in arrays]
        with self.on(step):
            sizes = st.decompress_batch([b.view for b in bufs], T, results, [v for _, v in outs])
        assert sizes == [a.size for a in arrays]
        for f, ((whole, _), a) in enumerate(zip(outs, arrays)):
            assert _is(whole, a), f"item {f} of the decompress batch differs"
        self.no_single_index()
        self.frames[g] = [Frame(b, w.size, w) for b, w in zip(bufs, wants)]

    def _decompress(self, step, op, ref, T):
        fr, arr = self.frames[step.group][step.frame], op["before"][step.frame]
        whole, view = _guarded(self.torch, arr.size)
        p, keep = self.index_arg(step, ref, T, [fr])
        with self.on(step):
            r = self.st.decompress(fr.view, T, fr.csize, view, p)
        assert r == arr.size and _is(whole, arr)

    def _ranges(self, step, op, ref, T):
        fr = self.frames[step.group][step.frame]
        c = Carved(self.torch, op["ranges"])
        p, keep = self.index_arg(step, ref, T, [fr])
        with self.on(step):
            r = self.st.decompress_ranges(fr.view, T, fr.csize, op["ranges"], c.ptrs, p)
        assert r == sum(n for _, n in op["ranges"])
        want = np.full(c.buf.numel(), GUARD_BYTE, dtype=np.uint8)
        for a, e in zip(c.at, op["expect"]):
            want[a:a + e.size] = e
        got = c.buf.cpu().numpy()
        assert np.array_equal(got, want), f"byte {int(np.flatnonzero(got != want)[0]) if got.size == want.size else -1} of the destinations differs"
        if step.form == "own":  # (calls that are given the context's index leave it as it is)
            self.single_index_is(fr, ref, T)

    def _gather(self, step, op, ref, T):
        fr, rb, rows = self.frames[step.group][step.frame], op["row_bytes"], op["rows"]
        sl = Slots(self.torch, len(rows), rb, rb + 9, 3)
        p, keep = self.index_arg(step, ref, T, [fr])
        rt = _rows_tensor(self.torch, rows)
        with self.on(step):
            r = self.st.gather_rows(fr.view, T, fr.csize, rb, rt, sl.ptr, p, rb + 9)
        assert r == len(rows) * rb
        _slots_hold(sl, op["expect"])
        if step.form == "own":
            self.single_index_is(fr, ref, T)

    def _gather_batch(self, step, op, ref, T):
        frames = [self.frames[step.group][f] for f in op["listed"]]
        rb, n = op["row_bytes"], len(op["rows"])
        sl = Slots(self.torch, n, rb, rb + 9, 3)
        p, keep = self.index_arg(step, ref, T, frames)
        ft, rt = _rows_tensor(self.torch, op["fids"]), _rows_tensor(self.torch, op["rows"])
        with self.on(step):
            r = self.st.gather_rows_batch([fr.view for fr in frames], T, [fr.csize for fr in frames], rb, ft, rt, sl.ptr, p, rb + 9)
        assert r == n * rb
        _slots_hold(sl, op["expect"])
        if step.form == "own":
            self.many_index_is(ref, T, frames)

    def _update(self, step, op, ref, T):
        torch, g, f = self.torch, step.group, step.frame
        fr, rb, rows = self.frames[g][f], op["row_bytes"], op["rows"]
        want = self.want_frame(ref, op["after"][f], T)
        out = Buf(torch, self.st.bound(op["after"][f].size))
        p, keep = self.index_arg(step, ref, T, [fr])
        rt, src = _rows_tensor(torch, rows), torch.from_numpy(op["src_rows"].reshape(-1)).cuda()
        with self.on(step):
            r = self.st.update_rows(fr.view, T, fr.csize, rb, rt, src, out.view, p)
        assert r == want.size, (r, want.size)
        out.holds(want)
        assert fr.buf.unchanged(), "the update modified its input frame"
        self.frames[g][f] = Frame(out, r, want)
        self.single_index_is(self.frames[g][f], ref, T)

    def _update_batch(self, step, op, ref, T):
        torch, g = self.torch, step.group
        frames = self.frames[g]
        wants = [self.want_frame(ref, a, T) for a in self.model.arrays[g]]
        outs = [Buf(torch, max(self.st.bound(a.size), 16)) for a in self.model.arrays[g]]
        p, keep = self.index_arg(step, ref, T, frames)
        ft, rt, src = _rows_tensor(torch, op["fids"]), _rows_tensor(torch, op["rows"]), torch.from_numpy(op["src_rows"].reshape(-1)).cuda()
        with self.on(step):
            results = self.st.update_rows_batch([fr.view for fr in frames], T, [fr.csize for fr in frames], op["row_bytes"], ft, rt, src, [o.view for o in outs], p)
        assert results == [w.size for w in wants], (results, [w.size for w in wants])
        for f, (o, w) in enumerate(zip(outs, wants)):
            try:
                o.holds(w)
            except AssertionError as err:
                raise AssertionError(f"output {f}: {err}") from None
        self.unchanged(g)
        self.frames[g] = [Frame(o, w.size, w) for o, w in zip(outs, wants)]
        self.no_single_index()
        self.many_index_is(ref, T, self.frames[g])

    def in_place(self, fr, total):
        """the frame in a new buffer with room for `total` bytes of array"""
        return Buf(self.torch, max(self.st.bound(total), 16), fr.view[:fr.csize])

    def _append(self, step, op, ref, T):
        g, f = step.group, step.frame
        fr = self.frames[g][f]
        want = self.want_frame(ref, op["after"][f], T)
        p, keep = self.index_arg(step, ref, T, [fr])  # (in front of the copy below, which is no call on the context)
        buf = self.in_place(fr, op["after"][f].size)
        alive, src = _src(self.torch, op["src"])
        with self.on(step):
            r = self.st.append(buf.view, T, fr.csize, src, p)
        assert r == want.size, (r, want.size)
        buf.holds(want)
        self.frames[g][f] = Frame(buf, r, want)
        self.single_index_is(self.frames[g][f], ref, T)

    def _append_batch(self, step, op, ref, T):
        g = step.group
        frames = self.frames[g]
        wants = [self.want_frame(ref, a, T) for a in self.model.arrays[g]]
        p, keep = self.index_arg(step, ref, T, frames)
        bufs = [self.in_place(fr, a.size) for fr, a in zip(frames, self.model.arrays[g])]
        held = [_src(self.torch, op["srcs"][f]) if op["srcs"][f].size else (None, None) for f in op["listed"]]
        with self.on(step):
            results = self.st.append_batch([b.view for b in bufs], T, [fr.csize for fr in frames], [s for _, s in held], p)
        assert results == [w.size for w in wants], (results, [w.size for w in wants])
        for f, (b, w) in enumerate(zip(bufs, wants)):
            try:
                b.holds(w)
            except AssertionError as err:
                raise AssertionError(f"frame {f}: {err}") from None
        self.frames[g] = [Frame(b, w.size, w) for b, w in zip(bufs, wants)]
        self.no_single_index()
        self.many_index_is(ref, T, self.frames[g])

    def _index(self, step, op, ref, T):
        st, g = self.st, step.group
        fr = self.frames[g][step.frame]
        want = fr.index(ref, T)
        n = c_size_t(0)
        with self.on(step):
            p = st.lib.stenos_hip_frame_index(st.ctx, fr.view.data_ptr(), T, fr.csize, ctypes.byref(n), st._stream_ptr())
        assert p and n.value == len(want) - 1 and _download(self.torch, p, n.value + 1) == want, "stenos_hip_frame_index"
        frames = self.frames[g]
        with self.on(step):
            p, entries = st.frames_index([x.view for x in frames], T, [x.csize for x in frames])
        assert entries == len(self.truth(ref, T, frames))
        self.many_index_is(ref, T, frames)

    def _host(self, step, op, ref, T):
        torch, st = self.torch, self.st
        arr = op["host_array"]
        made = []
        for s in (st, ref):
            dst = np.zeros(s.bound(arr.size), dtype=np.uint8)
            r = s.lib.stenos_compress_generic(s.ctx, arr.ctypes.data, T, arr.size, dst.ctypes.data, dst.size)
            assert r < ch.E(100), hex(r)
            made.append(dst[:r].copy())
        assert np.array_equal(made[0], made[1]), "the host-pointer frame differs from a fresh context's"
        back = np.zeros(arr.size, dtype=np.uint8)
        assert st.lib.stenos_decompress_generic(st.ctx, made[0].ctypes.data, T, made[0].size, back.ctypes.data, back.size) == arr.size
        assert np.array_equal(back, arr)
        # level 2: the strategy layer's buffers and its bookkeeping, then back
        small = op["level2_array"]
        src = torch.from_numpy(small).cuda()
        try:
            frames = []
            for s in (st, ref):
                assert s.lib.stenos_set_level(s.ctx, 2) == 0
                whole, view = _guarded(torch, s.bound(small.size))
                with self.on(step):
                    r = s.compress(src, T, view)
                got = whole.cpu().numpy()
                assert (got[:GUARD] == GUARD_BYTE).all() and (got[GUARD + view.numel():] == GUARD_BYTE).all()
                frames.append((view, r, got[GUARD:GUARD + r]))
            assert np.array_equal(frames[0][2], frames[1][2]), "the level-2 frame differs from a fresh context's"
            whole, view = _guarded(torch, small.size)
            with self.on(step):
                assert st.decompress(frames[0][0], T, frames[0][1], view) == small.size
            assert _is(whole, small)
        finally:
            assert st.lib.stenos_set_level(st.ctx, self.level) == 0

    def _fail(self, step, op, ref, T):
        torch, st, g, kind = self.torch, self.st, step.group, step.kind
        frames = self.frames[g]
        fr = frames[op["frame"]]
        arrays = self.model.arrays[g]
        P, Z = c_void_p * len(frames), c_size_t * len(frames)
        res = Z(*([77] * len(frames)))
        many = False
        if kind in ("gather_bad_row", "gather_damaged", "gather_batch_bad_pair"):
            rb, rows = op["row_bytes"], op["rows"]
            sl = Slots(torch, len(rows), rb, rb + 9, 3)
            rt = _rows_tensor(torch, rows)
            if kind == "gather_batch_bad_pair":
                ft = _rows_tensor(torch, op["fids"])
                call = lambda: st.gather_rows_batch([x.view for x in frames], T, [x.csize for x in frames], rb, ft, rt, sl.ptr, None, rb + 9)  # noqa: E731
            elif kind == "gather_bad_row":
                call = lambda: st.gather_rows(fr.view, T, fr.csize, rb, rt, sl.ptr, None, rb + 9)  # noqa: E731
            else:  # an unknown code in superblock 0, which every row touches; the index is given, so the chain is not walked
                offs = fr.index(ref, T)
                bad = fr.view[:fr.csize].clone()
                bad[offs[0]] = 9
                idx = torch.tensor(offs, dtype=torch.int64, device="cuda")
                call = lambda: st.gather_rows(bad, T, fr.csize, rb, rt, sl.ptr, idx.data_ptr(), rb + 9)  # noqa: E731
            with self.on(step):
                r = _code(call)
            assert r == op["error"], (hex(r), hex(op["error"]))
            assert sl.gaps_intact(), "a byte outside the slots changed"
            if op["bad_slot"] is not None:
                got = sl.buf.cpu().numpy()
                at = sl.at + op["bad_slot"] * sl.stride
                assert (got[at:at + rb] == GUARD_BYTE).all(), "the slot of the invalid row was written"
        elif kind in ("update_bad_row", "update_dst_overflow"):
            cap = st.bound(arrays[op["frame"]].size) if kind == "update_bad_row" else self.want_frame(ref, op["would_be"], T).size - 1
            out = Buf(torch, cap)
            rt, src = _rows_tensor(torch, op["rows"]), torch.from_numpy(op["src_rows"].reshape(-1)).cuda()
            with self.on(step):
                r = _code(lambda: st.update_rows(fr.view, T, fr.csize, op["row_bytes"], rt, src, out.view))
            assert r == op["error"], (hex(r), hex(op["error"]))
            assert out.unchanged(), "a failed update wrote to its output"
        elif kind == "update_batch_bad_pair":
            many = True
            outs = [Buf(torch, max(st.bound(a.size), 16)) for a in arrays]
            ft, rt, src = _rows_tensor(torch, op["fids"]), _rows_tensor(torch, op["rows"]), torch.from_numpy(op["src_rows"].reshape(-1)).cuda()
            with self.on(step):
                r = st.lib.stenos_hip_update_rows_batch(st.ctx, len(frames), T, P(*[x.view.data_ptr() for x in frames]), Z(*[x.csize for x in frames]), op["row_bytes"],
                                                        len(op["rows"]), ft.data_ptr(), rt.data_ptr(), src.data_ptr(), op["row_bytes"], P(*[o.view.data_ptr() for o in outs]),
                                                        Z(*[o.cap for o in outs]), res, None, st._stream_ptr())
            assert r == op["error"], (hex(r), hex(op["error"]))
            assert all(o.unchanged() for o in outs), "a failed update wrote to an output"
        elif kind in ("append_dst_overflow", "append_damaged"):
            alive, src = _src(torch, op["src"])
            if kind == "append_dst_overflow":
                cap = self.want_frame(ref, op["would_be"], T).size - 1
                assert cap >= fr.csize
                buf, size = Buf(torch, cap, fr.view[:fr.csize]), fr.csize
            else:  # the partial last superblock cut short
                size = fr.csize - op["cut"]
                buf = Buf(torch, st.bound(arrays[op["frame"]].size + op["src"].size), fr.view[:size])
            with self.on(step):
                r = _code(lambda: st.append(buf.view, T, size, src))
            assert r == op["error"], (hex(r), hex(op["error"]))
            assert buf.unchanged(), "a failed append wrote to the buffer"
        elif kind == "append_batch_damaged":
            many = True
            sizes = [x.csize - (op["cut"] if f == op["frame"] else 0) for f, x in enumerate(frames)]
            bufs = [Buf(torch, max(st.bound(a.size + op["srcs"][f].size), 16), x.view[:n]) for f, (x, a, n) in enumerate(zip(frames, arrays, sizes))]
            held = [_src(torch, op["srcs"][f]) if op["srcs"][f].size else (None, (None, 0)) for f in range(len(frames))]
            with self.on(step):
                r = st.lib.stenos_hip_append_batch(st.ctx, len(frames), T, P(*[b.view.data_ptr() for b in bufs]), Z(*sizes), Z(*[b.cap for b in bufs]),
                                                   P(*[s[0] for _, s in held]), Z(*[s[1] for _, s in held]), res, None, st._stream_ptr())
            assert r == op["error"], (hex(r), hex(op["error"]))
            assert all(b.unchanged() for b in bufs), "a failed append wrote to a buffer"
        else:
            raise ValueError(kind)
        assert list(res) == [77] * len(frames), "a failed call wrote to results[]"
        self.unchanged(g)
        if many:
            self.no_many_index()

    def audit(self):
        """every frame of the store decodes on the long-lived context to its model array and is a fresh context's compression"""
        ref = self.fresh()
        try:
            for g, (T, n) in ch.GROUPS.items():
                for f in range(n):
                    fr, arr = self.frames[g][f], self.model.arrays[g][f]
                    want = self.want_frame(ref, arr, T)
                    got = fr.view[:fr.csize].cpu().numpy()
                    assert fr.csize == want.size and np.array_equal(got, want), f"audit: frame {f} of group {g} is not the compression of its array"
                    if arr.size:
                        whole, view = _guarded(self.torch, arr.size)
                        assert self.st.decompress(fr.view, T, fr.csize, view) == arr.size and _is(whole, arr), f"audit: frame {f} of group {g} does not decode to its array"
        finally:
            ref.close()
        self.invariant()


def run(specs, level, lib=None, before=None, after=None):
    torch = _cuda()
    steps = ch.steps_of(specs)
    r = Run(torch, level, lib)
    try:
        if before:
            before(r.st)
        due = False
        for step in steps:
            try:
                r.step(step)
                # (the audit's decodes walk chains into the context's index: it waits for a step that is not given that index)
                due |= (step.i + 1) % AUDIT_EVERY == 0
                if step.i + 1 == len(steps) or (due and steps[step.i + 1].form != "own"):
                    r.audit()
                    due = False
            except (AssertionError, StenosError) as err:
                raise AssertionError(f"step {step.i}: {step.cls}{'/' + step.kind if step.kind else ''} after {step.prev}, {step.regime}, group {step.group}, frame "
                                     f"{step.frame}, index form {step.form}, stream {step.stream}, level {level}: {err}\nto replay: {list(specs[:step.i + 1])!r}") from err
        if after:
            after(r.st)
    finally:
        r.close()


@pytest.mark.parametrize("level", [1, 0])
def test_one_context_through_every_pair_of_calls(level):
    run(ch.sequence(), level)


REPLAYS = {
    # compress(large, noise) -> compress(small) -> gather(small) -> append(small) -> gather_batch -> fail -> append_batch: the replay path itself
    "the_replay_path": [("compress", "large", "A", 1), ("compress", "small", "A", 3), ("gather", "small", "A", 3), ("append", "small", "A", 3),
                        ("gather_batch", "small", "A", -1), ("fail", "small", "A", "append_batch_damaged"), ("append_batch", "small", "A", -1)],
}


@pytest.mark.parametrize("prefix", list(REPLAYS), ids=list(REPLAYS))
def test_replay(prefix):
    """a list as a failure of the test above prints it, run the same way with the same checks; shortest failing prefixes go here"""
    run(REPLAYS[prefix], 1)


def test_a_fused_launch_that_gave_up_changes_nothing_after_it(hooks_lib):
    """The test build's switch makes the host treat the fused launch of a large compress as having given up (nothing on the device
    misbehaves): the frame is made again without the fused kernel, and every other class of call, once, in the small regime, gives
    what it gives on a fresh context."""
    specs = [("compress", "large", "A", 1)]
    for k, c in enumerate(x for x in ch.CLASSES if x != "compress"):
        g = "ABC"[k % 3]
        frame = ch.FAILS[k % len(ch.FAILS)] if c == "fail" else ch.SLOTS[g]["small"][k % 2] if c in ch.SINGLE_INDEX + ("index", "compress_async") else -1
        specs.append((c, "small", g, frame))
    assert [s[0] for s in specs] == ["compress"] + [c for c in ch.CLASSES if c != "compress"] and len(specs) == 14

    def check(st):
        assert st.lib.stenos_hip_fused_fallbacks(st.ctx) == 1

    run(specs, 1, hooks_lib, before=lambda st: st.lib.stenos_hip_test_fused_timeouts(st.ctx, 1), after=check)
