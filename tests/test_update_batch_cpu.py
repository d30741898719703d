"""CPU-side checks of stenos_hip_update_rows_batch (include/stenos_hip.h): what one thread or wavefront of update_batch_plan,
update_batch_apply, update_batch_splice_plan and update_batch_splice does (csrc/update_codec.h) in the host emulation
(tests/emul_update_batch: plain and with the access audit) against a numpy model of the compact list over all frames, the per-frame
counts, the overlaid slots, the new indices and the spliced frames; refused indices; declared, exported and bound; the refusals that
need no device; loud failure without one; the build properties of csrc/update_batch_kernels.hip.

Every case runs in both builds.  The audited one checks every global access: reads against an arena that, while a frame's work is
emulated, ENDS with that frame's last byte; writes against the planning tables, then each slot's bytes, then [0, new total_f) of
output f.  Slots and every output stand between 64 guard bytes of 0xA5 and are shifted off their alignment; after a refusal every
output arena must still be 0xA5.  The frames are made of stored superblocks (code 6), as in tests/test_update_cpu.py."""
import ctypes
import os
import re
import shutil
import subprocess
from ctypes import c_char_p, c_int, c_size_t, c_uint32, c_void_p

import numpy as np
import pytest

from _libs import ROOT, np_ptr
from stenos_amd.api import load_library
from test_gather_cpu import model_cut, model_pieces_per_row
from test_update_cpu import MIS, NO_SLOT, PIECE, ST_HOST_CODES, ST_INVALID, ST_TRUNCATED, W_K, W_STATUS, E, encode_again, stored_frame

NAME = "stenos_hip_update_rows_batch"


def _load(name):
    d = os.path.join(ROOT, "tests", "emul_update_batch")
    subprocess.check_call(["make", "-C", d], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    lib = ctypes.CDLL(os.path.join(d, name))
    vp, u32, sz = c_void_p, c_uint32, c_size_t
    lib.emul_ub_plan_apply.restype = sz
    lib.emul_ub_plan_apply.argtypes = [u32, vp, sz, vp, vp, vp, vp, u32, vp, vp, vp, sz, vp, sz, vp, vp, c_int, c_int, vp, vp, vp, vp, vp, vp, vp]
    lib.emul_ub_splice.restype = sz
    lib.emul_ub_splice.argtypes = [u32, vp, sz, vp, vp, vp, vp, u32, vp, vp, vp, sz, vp, vp, u32, vp, c_int, c_int, vp, vp, vp, vp, vp]
    lib.emul_audit_first_name.restype = c_char_p
    lib.emul_update_batch_audited.restype = c_int
    return lib


@pytest.fixture(scope="module")
def builds():
    plain, audit = _load("libstenos_emul_update_batch.so"), _load("libstenos_emul_update_batch_audit.so")
    assert plain.emul_update_batch_audited() == 0 and audit.emul_update_batch_audited() == 1
    return plain, audit


def _clean(lib, rep, what):
    off = int(rep[3]) - (1 << 64) if int(rep[3]) >> 63 else int(rep[3])
    assert rep[0] == 0, (f"{what}: {rep[0]} accesses outside their arena, first: {lib.emul_audit_first_name().decode()} kind {rep[2]} "
                         f"(1 global read, 2 global write) at arena offset {off}, {rep[4]} bytes")
    if lib.emul_update_batch_audited():
        assert rep[1] > 0, what


def u64(x):
    return np.ascontiguousarray(x, dtype=np.uint64)


# ---- the model ----------------------------------------------------------------------------------------------------------

class Frames:
    """m frames of stored superblocks of `sb` bytes; entry f names frame `same[f]`'s bytes where given (the same frame listed twice)"""

    def __init__(self, rng, sb, totals, headers=None, codes=None, same=None):
        self.sb, self.m = sb, len(totals)
        self.totals = list(totals)
        self.headers = list(headers or [8] * self.m)
        self.datas, self.frames, self.idxs = [], [], []
        self.off, cat = [], []
        at = 0
        for f, total in enumerate(totals):
            if same and f in same:
                g = same[f]
                self.datas.append(self.datas[g])
                self.frames.append(self.frames[g])
                self.idxs.append(self.idxs[g])
                self.off.append(self.off[g])
                continue
            data = rng.integers(0, 256, total, dtype=np.uint8)
            if total:
                frame, idx = stored_frame(data, sb, self.headers[f], (codes or {}).get(f))
            else:  # the frame of an empty array: its header, one index entry
                frame, idx = np.frombuffer(bytes(8), dtype=np.uint8).copy(), np.array([8], dtype=np.uint64)
            self.datas.append(data)
            self.frames.append(frame)
            self.idxs.append(idx)
            self.off.append(at)
            cat.append(frame)
            at += frame.size
        self.cat = np.concatenate(cat)
        self.nsb = [-(-t // sb) for t in self.totals]
        self.first = np.concatenate(([0], np.cumsum(self.nsb))).astype(np.int64)
        self.S = int(self.first[-1])
        self.idx = np.concatenate(self.idxs).astype(np.uint64)  # frame f's nsb_f + 1 entries start at first[f] + f
        self.sizes = [fr.size for fr in self.frames]
        self.codes = codes or {}
        dec = [d for d in self.datas]
        self.dec_off = np.concatenate(([0], np.cumsum([d.size for d in dec])))[:-1]
        self.dec = np.concatenate(dec) if sum(d.size for d in dec) else np.zeros(1, dtype=np.uint8)

    def frame_of(self, g):
        return int(np.searchsorted(self.first, g, side="right")) - 1


def grouped_pieces(fr, pairs, row_bytes, stride, rng):
    """what gather_batch_count / gather_scan / gather_batch_fill leave: (ppre, the table ordered by the batch's superblock numbers)"""
    P = max([model_pieces_per_row(row_bytes, fr.sb) for t in fr.totals if t] or [1])
    per = [[] for _ in range(fr.S)]
    for i, (f, row) in enumerate(pairs):
        for j in range(P):
            if j >= model_pieces_per_row(row_bytes, fr.sb):
                continue
            c = model_cut(row_bytes, stride, fr.totals[f], fr.sb, int(row), i, j)
            if c:
                per[int(fr.first[f]) + c[0]].append(c[1:])
    for lst in per:
        rng.shuffle(lst)
    ppre = np.zeros(fr.S + 1, dtype=np.uint32)
    ppre[1:] = np.cumsum([len(x) for x in per])
    tab = np.zeros(int(ppre[-1]), dtype=PIECE)
    k = 0
    for lst in per:
        for lo, hi, dst in lst:
            tab[k] = (lo, hi, dst)
            k += 1
    return ppre, tab, per


def plan_apply(lib, fr, idx, ppre, tab, src, mis):
    S, m = fr.S, fr.m
    slot, touched, flags = (np.zeros(max(S, 1), dtype=np.uint32) for _ in range(3))
    words = np.zeros(16, dtype=np.uint32)
    kf = np.zeros(2 * m, dtype=np.uint32)
    raw = np.zeros(S * fr.sb + 16, dtype=np.uint8)
    rep = np.zeros(5, dtype=np.uint64)
    off, sizes, totals, headers, dec_off = (u64(x) for x in (fr.off, fr.sizes, fr.totals, fr.headers, fr.dec_off))  # (kept alive over the call)
    r = lib.emul_ub_plan_apply(m, np_ptr(fr.cat), fr.cat.size, np_ptr(off), np_ptr(sizes), np_ptr(totals), np_ptr(headers), fr.sb,
                               np_ptr(idx), np_ptr(ppre), np_ptr(tab) if tab.size else None, tab.size, np_ptr(src) if src.size else None, src.size, np_ptr(fr.dec),
                               np_ptr(dec_off), mis[0], mis[1], np_ptr(slot), np_ptr(touched), np_ptr(flags), np_ptr(words), np_ptr(kf), np_ptr(raw), np_ptr(rep))
    assert r != E(7), "a byte outside the slots' decoded bytes changed"
    assert r == 0
    _clean(lib, rep, "update_batch_plan / update_batch_apply")
    return slot[:S], touched, flags[:S], words, kf.reshape(m, 2), raw


def splice(lib, fr, idx, slot, enc, enc_base, enc_off, K, caps, mis):
    S, m = fr.S, fr.m
    new_idx = np.zeros(S + m, dtype=np.uint64)
    totals = np.zeros(m, dtype=np.uint64)
    words = np.zeros(16, dtype=np.uint32)
    out = np.zeros(int(sum(int(c) for c in caps)) + 16, dtype=np.uint8)
    rep = np.zeros(5, dtype=np.uint64)
    slot = np.ascontiguousarray(np.concatenate((slot, np.zeros(1, dtype=np.uint32))))
    off, sizes, old_totals, headers, enc_base, enc_off, caps = (u64(x) for x in (fr.off, fr.sizes, fr.totals, fr.headers, enc_base, enc_off, caps))  # (kept alive)
    r = lib.emul_ub_splice(m, np_ptr(fr.cat), fr.cat.size, np_ptr(off), np_ptr(sizes), np_ptr(old_totals), np_ptr(headers), fr.sb, np_ptr(idx),
                           np_ptr(slot), np_ptr(enc) if enc.size else None, enc.size, np_ptr(enc_base), np_ptr(enc_off), K, np_ptr(caps), mis[0], mis[1],
                           np_ptr(new_idx), np_ptr(totals), np_ptr(words), np_ptr(out), np_ptr(rep))
    assert r != E(7), "a byte of an output arena outside [0, new total) changed"
    assert r != E(3)
    _clean(lib, rep, "update_batch_splice_plan / update_batch_splice")
    return r, new_idx, totals, words, out


def run_case(builds, rng, fr, row_bytes, pairs, how, turn=0, dup_sources=False):
    sb, m, S = fr.sb, fr.m, fr.S
    stride = row_bytes + (turn % 3) * 67
    n = len(pairs)
    src = np.full(max(1, (n - 1) * stride + row_bytes) if n else 0, 0xEE, dtype=np.uint8)
    for i in range(n):
        src[i * stride:i * stride + row_bytes] = rng.integers(0, 256, row_bytes, dtype=np.uint8)
    ppre, tab, per = grouped_pieces(fr, pairs, row_bytes, stride, rng)
    want_touched = [g for g in range(S) if per[g]]
    K = len(want_touched)
    want_slot = np.full(S, NO_SLOT, dtype=np.uint32)
    want_slot[want_touched] = np.arange(K, dtype=np.uint32)
    want_kf = np.zeros((m, 2), dtype=np.uint32)
    for g in want_touched:
        f = fr.frame_of(g)
        want_kf[f, 0] += 1
        want_kf[f, 1] = max(want_kf[f, 1], g - int(fr.first[f]))
    code_of = lambda g: fr.codes.get(fr.frame_of(g), {}).get(g - int(fr.first[fr.frame_of(g)]), 6)  # noqa: E731
    order = {}
    for g in range(S):
        for lo, hi, d in per[g]:
            order.setdefault((g, lo), []).append(src[d:d + hi - lo].copy())
    results = []
    for lib in builds:
        mis = MIS[(turn + (lib is builds[1])) % len(MIS)]
        slot, touched, flags, words, kf, raw = plan_apply(lib, fr, fr.idx, ppre, tab, src, mis)
        assert words[W_K] == K and np.array_equal(slot, want_slot) and touched[:K].tolist() == want_touched
        assert np.array_equal(kf, want_kf), (kf.tolist(), want_kf.tolist())
        want_flags = [1 if per[g] and code_of(g) in (2, 3, 4, 5) else 0 for g in range(S)]
        assert flags.tolist() == want_flags and bool(words[W_STATUS] & ST_HOST_CODES) == any(want_flags)
        assert not words[W_STATUS] & (ST_TRUNCATED | ST_INVALID)
        # the slots: the superblock's bytes with every piece replaced by (one of) its sources, whole
        slots = []
        for c, g in enumerate(want_touched):
            f = fr.frame_of(g)
            s = g - int(fr.first[f])
            dsize = min(sb, fr.totals[f] - s * sb)
            got = raw[c * sb:c * sb + dsize]
            covered = np.zeros(dsize, dtype=bool)
            for lo, hi, _ in per[g]:
                cands = order[(g, lo)]
                assert any(np.array_equal(got[lo:hi], x) for x in cands), (g, lo, hi, "a piece is not one of its sources, whole")
                if not dup_sources:
                    assert len(cands) == 1 or all(np.array_equal(cands[0], x) for x in cands)
                covered[lo:hi] = True
            assert np.array_equal(got[~covered], fr.datas[f][s * sb:s * sb + dsize][~covered]), "bytes no piece covers changed"
            slots.append(got.copy())
        # any new bytes for the touched superblocks, frame by frame: a stream per frame, its offsets at entry c_f + f
        enc_parts, enc_base, enc_off, parts_of = [], [], np.zeros(K + m, dtype=np.uint64), {}
        at = c0 = 0
        for f in range(m):
            k = int(want_kf[f, 0])
            enc, off, parts = encode_again(slots[c0:c0 + k], np.random.default_rng([7, turn, f]), how)
            enc_base.append(at)
            enc_off[c0 + f:c0 + f + k + 1] = off
            for i, p in enumerate(parts):
                parts_of[want_touched[c0 + i]] = p
            pad = bytes(rng.integers(0, 256, 5 + f % 3, dtype=np.uint8))  # (the streams do not touch)
            enc_parts += [bytes(enc), pad]
            at += enc.size + len(pad)
            c0 += k
        enc = np.frombuffer(b"".join(enc_parts), dtype=np.uint8).copy()
        want, want_idx = [], []
        for f in range(m):
            gs = range(int(fr.first[f]), int(fr.first[f + 1]))
            pieces = [parts_of[g] if g in parts_of else bytes(fr.frames[f][int(fr.idxs[f][g - gs.start]):int(fr.idxs[f][g - gs.start + 1])]) for g in gs]
            want.append(bytes(fr.frames[f][:fr.headers[f]]) + b"".join(pieces))
            want_idx += np.cumsum([fr.headers[f]] + [len(p) for p in pieces]).tolist()
        caps = [len(w) for w in want]
        r, new_idx, totals, words2, out = splice(lib, fr, fr.idx, slot, enc, enc_base, enc_off, K, caps, mis)
        assert r == 0 and new_idx.tolist() == want_idx and totals.tolist() == caps
        at = 0
        for f in range(m):
            assert bytes(out[at:at + caps[f]]) == want[f], f
            at += caps[f]
        # one output one byte short: refused, every arena untouched (checked inside: -7 otherwise)
        short = list(caps)
        short[turn % m] -= 1
        r2 = splice(lib, fr, fr.idx, slot, enc, enc_base, enc_off, K, short, mis)[0]
        assert r2 == E(6)
        results.append((bytes(raw[:K * sb]) if not dup_sources else b"", bytes(out[:sum(caps)])))
    if not dup_sources:
        assert results[0] == results[1], "the result depends on the build"
    return K


def batches(rng, sb):
    """1, 3 and 8 frames: an empty array, a one-superblock frame, a frame with a short last superblock, the same frame twice"""
    yield Frames(rng, sb, [2 * sb + 300 % sb + 7])
    yield Frames(rng, sb, [sb, 0, 3 * sb + 41], headers=[8, 8, 12])
    yield Frames(rng, sb, [2 * sb + 9, sb, 0, 4 * sb, 2 * sb + 9, 3 * sb + 41, sb - 5, 2 * sb], headers=[8, 12, 8, 8, 8, 12, 8, 8], same={4: 0})


@pytest.mark.parametrize("sb", [1024, 96])
def test_plan_apply_and_splice_against_the_model(builds, sb):
    rng = np.random.default_rng([91, sb])
    turn, seen = 0, set()
    for fr in batches(rng, sb):
        for row_bytes in (1, 7, sb // 4, sb, sb + 5):
            every = [(f, r) for f in range(fr.m) for r in range(fr.totals[f] // row_bytes)]
            if row_bytes == 1 and len(every) > 3000:
                every = [every[i] for i in sorted(rng.choice(len(every), 3000, replace=False).tolist())]
            big = max(range(fr.m), key=lambda f: fr.totals[f])
            sets = {"none": [], "one": every[len(every) // 2:len(every) // 2 + 1], "every row, permuted across the frames": every,
                    "one frame only": [p for p in every if p[0] == big]}
            for name, pairs in sets.items():
                pairs = list(pairs)
                rng.shuffle(pairs)
                how = ("mixed", "grow", "shrink", "same")[turn % 4]
                K = run_case(builds, rng, fr, row_bytes, pairs, how, turn)
                seen.add("nothing" if K == 0 else "everything" if K == fr.S else "some")
                turn += 1
    assert seen == {"nothing", "everything", "some"} and turn == 60


def test_more_superblocks_than_planning_threads(builds):
    """2 600 superblocks in six frames, more than 1 024 of them touched: a planning thread takes a run of three, which frames' ends cut"""
    rng = np.random.default_rng(92)
    sb = 64
    fr = Frames(rng, sb, [1000 * sb - 11, 0, 599 * sb, sb + 3, 997 * sb + 1, 3 * sb])
    assert fr.S == 2602
    rows = [(f, r) for f in range(fr.m) for r in range(fr.totals[f] // sb) if rng.random() < 0.6 or r < 3 or r >= fr.totals[f] // sb - 3]
    K = run_case(builds, rng, fr, sb, rows, "mixed", turn=3)
    assert 1024 < K < fr.S
    # 53-byte rows straddle; every row of every frame
    K = run_case(builds, rng, fr, 53, [(f, r) for f in range(fr.m) for r in range(fr.totals[f] // 53)], "grow", turn=4)
    assert K > 2500


def test_zstd_based_codes_of_touched_superblocks_are_flagged_in_the_right_frame(builds):
    rng = np.random.default_rng(93)
    sb = 256
    # frame 0: superblock 1 zstd-coded and touched, 3 zstd-coded and untouched; frame 2: its last superblock zstd-coded and touched,
    # superblock 1 (the number that is flagged in frame 0) stored and touched
    fr = Frames(rng, sb, [5 * sb + 30, sb, 3 * sb + 30], codes={0: {1: 3, 3: 5}, 2: {3: 2}})
    pairs = [(0, 0), (0, 17), (0, 18), (2, (3 * sb + 30) // 16 - 1), (2, 17), (1, 2)]
    run_case(builds, rng, fr, 16, pairs, "same", turn=1)


def test_repeated_pairs_hold_one_of_their_sources_whole(builds):
    rng = np.random.default_rng(94)
    sb = 1024
    fr = Frames(rng, sb, [3 * sb + 100, 2 * sb, 3 * sb + 100], same={2: 0})
    for row_bytes, pairs in ((100, [(0, 3), (0, 3), (2, 3), (0, 10), (1, 10), (1, 10), (0, 3)]), (1, [(1, 5)] * 70 + [(0, 5)] * 70), (1500, [(0, 1), (0, 1), (2, 0), (0, 1)])):
        run_case(builds, rng, fr, row_bytes, pairs, "same", turn=row_bytes, dup_sources=True)


def test_bad_indices_are_refused_with_nothing_written(builds):
    """in the first, a middle and the last frame: a decreasing offset, a superblock under 4 bytes, a last entry past sizes[f], an
    entry that points into another frame's slice of the frames' memory"""
    rng = np.random.default_rng(95)
    sb = 512
    fr = Frames(rng, sb, [4 * sb + 9, sb, 3 * sb, 0, 2 * sb + 100])
    slot = np.full(fr.S, NO_SLOT, dtype=np.uint32)
    caps = [4 * s for s in fr.sizes]
    none = np.zeros(0, dtype=np.uint8)
    for lib in builds:
        ok = splice(lib, fr, fr.idx, slot, none, [0] * fr.m, np.zeros(fr.m, dtype=np.uint64), 0, caps, MIS[1])
        assert ok[0] == 0 and ok[2].tolist() == fr.sizes  # (no pair: every frame is copied)
        for f in (0, 2, 4):
            at, end = int(fr.first[f]) + f, int(fr.first[f + 1]) + f
            other = (f + 2) % fr.m
            cases = []
            bad = fr.idx.copy()
            bad[at + 1] = bad[at] - 1
            cases.append((bad, E(4)))
            bad = fr.idx.copy()
            bad[at + 1] = bad[at] + 3
            cases.append((bad, E(4)))
            bad = fr.idx.copy()
            bad[end] = fr.sizes[f] + 1
            cases.append((bad, E(2)))
            bad = fr.idx.copy()  # where frame `other` lies, seen from frame f: behind f's end, or in front of its start
            delta = (fr.off[other] + 8) - fr.off[f]
            bad[end] = np.uint64(delta % (1 << 64))
            cases.append((bad, None))
            for bad, code in cases:
                r, _, _, words, _ = splice(lib, fr, bad, slot, none, [0] * fr.m, np.zeros(fr.m, dtype=np.uint64), 0, caps, MIS[2])
                assert r in ((code,) if code else (E(2), E(4))), (f, bad.tolist(), hex(r))
                assert words[W_STATUS] & (ST_INVALID | ST_TRUNCATED)


def test_plan_bounds_a_bad_index_entry_of_a_touched_superblock(builds):
    """update_batch_plan reads the code byte of a touched superblock only inside its own frame (the read arena ends with it)"""
    rng = np.random.default_rng(96)
    sb = 256
    fr = Frames(rng, sb, [3 * sb, 2 * sb, 3 * sb])
    pairs = [(f, r) for f in range(3) for r in (0, 20)]
    ppre, tab, _ = grouped_pieces(fr, pairs, 16, 16, rng)
    src = rng.integers(0, 256, 16 * len(pairs), dtype=np.uint8)
    for f in range(3):
        for at in (fr.sizes[f] - 3, fr.sizes[f], fr.sizes[f] + 100, (1 << 64) - 2):
            bad = fr.idx.copy()
            bad[int(fr.first[f]) + f + 1] = at  # (superblock 1 of frame f is touched: row 20)
            for lib in builds:
                _, _, _, words, _, _ = plan_apply(lib, fr, bad, ppre, tab, src, MIS[3])
                assert words[W_STATUS] & ST_TRUNCATED and words[W_K] == 6


# ---- the entry point --------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    so = os.path.join(ROOT, "stenos_amd", "lib", "libstenos.so")
    if not os.path.exists(so):
        import __graft_entry__

        __graft_entry__.build()
    return load_library()


def test_declared_exported_and_bound(lib):
    text = open(os.path.join(ROOT, "include", "stenos_hip.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "stenos_amd", "lib", "libstenos.so")], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in (NAME, "stenos_hip_last_frames_index"):
        assert re.search(r"STENOS_EXPORT[^;(]*\b" + name + r"\s*\(", text), name
        assert name in exported and name in lib._stenos_symbols, name
    from stenos_amd.api import Stenos

    assert callable(Stenos.update_rows_batch) and callable(Stenos.last_frames_index)
    comment = text[:text.index("STENOS_EXPORT size_t " + NAME)].rsplit("/*", 1)[1]
    for phrase in ("WHAT IS CHECKED", "NOT detected", "WRITES TO d_outs", "REPEATED PAIRS", "DEVICE MEMORY", "never shrink", "ONE GEOMETRY", "one superblock size",
                   "one block-size setting", "WHO IS SERVED BY WHAT", "profiles/update_batch_rate.txt", "stenos_hip_last_frames_index", "all or nothing"):
        assert phrase in comment, phrase


def _call(lib, ctx, n, T=4, m=2, row_bytes=16, stride=16, ids=0x200000, rows=0x210000, src=0x300000, frames=(0x1000, 0x9000), outs=(0x100000, 0x180000),
          tables=True):
    P, Z = c_void_p * max(m, 1), c_size_t * max(m, 1)
    fr = P(*frames[:m]) if tables else None
    ou = P(*outs[:m]) if tables else None
    return lib.stenos_hip_update_rows_batch(ctx, m, T, fr, Z(*([4096] * m)), row_bytes, n, ids, rows, src, stride, ou, Z(*([1 << 19] * m)), Z(*([0] * m)), None, None)


def test_refusals_that_need_no_device(lib):
    """(the device pointers are made up: a call that went on would fault)"""
    ctx = lib.stenos_make_context()
    try:
        bad = E(9)  # STENOS_ERROR_INVALID_PARAMETER
        # every shape refusal of the single call
        assert _call(lib, ctx, 3, row_bytes=0) == bad and _call(lib, ctx, 0, row_bytes=0) == bad
        assert _call(lib, ctx, 3, row_bytes=16, stride=15) == bad
        assert _call(lib, ctx, 3, T=0) == bad and _call(lib, ctx, 3, T=65) == bad
        assert _call(lib, ctx, 1 << 61, row_bytes=8, stride=8) == bad  # n * row_bytes
        assert _call(lib, ctx, 3, row_bytes=1 << 63, stride=1 << 63) == bad
        assert _call(lib, ctx, (1 << 40) + 1, row_bytes=1, stride=1 << 24) == bad  # (n - 1) * src_stride + row_bytes
        assert _call(lib, ctx, 2, row_bytes=16, stride=(1 << 64) - 8) == bad
        assert _call(lib, ctx, 3, rows=None) == bad and _call(lib, ctx, 3, src=None) == bad and _call(lib, ctx, 3, ids=None) == bad
        assert _call(lib, ctx, 3, tables=False) == bad
        # no frame; more frames than one thread each; a NULL table entry
        assert _call(lib, ctx, 3, m=0) == bad and _call(lib, ctx, 0, m=0) == bad
        assert lib.stenos_hip_update_rows_batch(ctx, 1 << 31, 4, (c_void_p * 1)(0x1000), (c_size_t * 1)(4096), 16, 0, None, None, None, 16, (c_void_p * 1)(0x100000),
                                                (c_size_t * 1)(1 << 19), (c_size_t * 1)(0), None, None) == bad
        assert _call(lib, ctx, 3, frames=(0x1000, None)) == bad and _call(lib, ctx, 3, frames=(None, 0x9000)) == bad
        assert _call(lib, ctx, 3, outs=(0x100000, None)) == bad and _call(lib, ctx, 0, outs=(None, 0x180000)) == bad
        # what stenos_hip_compress_batch refuses to compress
        for level in (2, 5, 9):
            lib.stenos_set_level(ctx, level)
            assert _call(lib, ctx, 3) == bad, level
        lib.stenos_set_level(ctx, 1)
        assert _call(lib, ctx, 3, T=1, row_bytes=16) == bad  # bytesoftype 1 at level 1
        lib.stenos_set_max_nanoseconds(ctx, 1000)
        assert _call(lib, ctx, 3) == bad
        # and no many-frame index was left
        n = c_size_t(7)
        assert not lib.stenos_hip_last_frames_index(ctx, ctypes.byref(n)) and n.value == 0
    finally:
        lib.stenos_destroy_context(ctx)


def test_no_gpu_means_loud_failure(lib):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    ctx = lib.stenos_make_context()
    try:
        assert _call(lib, ctx, 3) == E(5)  # STENOS_ERROR_INVALID_INSTRUCTION_SET
        assert _call(lib, ctx, 0) == E(5)
    finally:
        lib.stenos_destroy_context(ctx)


# ---- build properties of update_batch_kernels.hip ---------------------------------------------------------------------------

KEYS = [f"update_batch_decodeILj{T}E" for T in (2, 4, 8, 0)]
OTHERS = ["update_batch_planE", "update_batch_applyE", "update_batch_splice_planE", "update_batch_spliceE"]


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_update_batch_decoder_has_no_divergent_branch():
    p = subprocess.run([os.path.join(ROOT, "tools", "divergent_branches.sh"), "update_batch_kernels.hip"] + KEYS, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert [l for l in lines if l.startswith("== ")] == [f"== {k}" for k in KEYS], p.stdout[-1500:]
    assert [l for l in lines if not l.startswith("== ")] == [], "divergent branches:\n" + p.stdout[-1500:]


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_update_batch_kernel_resources():
    """no scratch memory, no spilled vector register, eight waves per SIMD; and no name an existing budget test keys on is part of
    a new kernel's name"""
    cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-c",
           os.path.join(ROOT, "stenos_amd", "csrc", "update_batch_kernels.hip"), "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage", "-mllvm",
           "-structurizecfg-skip-uniform-regions=1"]
    err = subprocess.run(cmd, capture_output=True, text=True, timeout=900).stderr
    res, cur = {}, None
    for line in err.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = res.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[bytes/lane\]| \[waves/SIMD\])?: (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    for key in KEYS + OTHERS:
        hits = [v for k, v in res.items() if key in k]
        assert len(hits) == 1, (key, list(res))
        assert hits[0]["ScratchSize"] == 0 and hits[0]["VGPRs Spill"] == 0, (key, hits[0])
        assert hits[0]["Occupancy"] == 8, (key, hits[0])
    for name in res:
        for old in ("decode_superblocksILj", "encode_superblocksILj", "decode_frames_batchILj", "decode_rangesILj", "gather_decodeILj", "gather_batch_decodeILj",
                    "update_decodeILj", "update_planE", "update_applyE", "update_splice_planE", "update_spliceE"):
            assert old not in name, (old, name)
