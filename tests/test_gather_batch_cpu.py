"""CPU-side checks of stenos_hip_gather_rows_batch and stenos_hip_frames_index (include/stenos_hip.h): the pair-cutting function
of csrc/gather_codec.h (gather_cut_pair) against a Python model built on model_cut of test_gather_cpu.py; the whole piece plan
-- count, scan, fill, chunks -- in the host emulation (tests/emul_gather_batch) against that model; declared, exported and bound;
the refusals that need no device; loud failure without one; the build properties of gather_batch_decode
(csrc/gather_batch_kernels.hip).  The decoding of a chunk is decode_superblock_pieces, unchanged: test_gather_cpu.py covers it."""
import ctypes
import os
import re
import shutil
import subprocess
from collections import Counter
from ctypes import c_int, c_uint64

import numpy as np
import pytest

import streamgen as sg
from _libs import ROOT
from stenos_amd.api import load_library
from test_gather_cpu import _totals, model_cut, model_pieces_per_row

NAMES = ("stenos_hip_gather_rows_batch", "stenos_hip_frames_index")
E = lambda k: (1 << 64) - k  # noqa: E731
U64P = ctypes.POINTER(c_uint64)
PIECE, NONE, INVALID = 1, 0, -1


@pytest.fixture(scope="module")
def emul():
    d = os.path.join(ROOT, "tests", "emul_gather_batch")
    subprocess.check_call(["make", "-C", d], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    lib = ctypes.CDLL(os.path.join(d, "libstenos_emul_gather_batch.so"))
    lib.emul_gb_table.restype = None
    lib.emul_gb_table.argtypes = [c_uint64, U64P, U64P, c_uint64, U64P]
    lib.emul_gb_cut_pair.restype = c_int
    lib.emul_gb_cut_pair.argtypes = [c_uint64, U64P, U64P] + [c_uint64] * 6 + [U64P]
    lib.emul_gb_plan.restype = c_int
    lib.emul_gb_plan.argtypes = [c_uint64, U64P, U64P, c_uint64, c_uint64, c_uint64, U64P, U64P, U64P, U64P, c_uint64, U64P]
    return lib


def arr(values):
    return (c_uint64 * max(1, len(values)))(*values)


# ---- the model -----------------------------------------------------------------------------------------------------------

class ModelBatch:
    """frames as (total, sb); superblocks numbered through; P of the call the largest of the frames' own"""

    def __init__(self, frames, row_bytes):
        self.frames, self.row_bytes = frames, row_bytes
        self.nsb = [-(-t // sb) if t else 0 for t, sb in frames]
        self.first = [sum(self.nsb[:f]) for f in range(len(frames))]
        self.S = sum(self.nsb)
        self.own = [model_pieces_per_row(row_bytes, sb) if t else 0 for t, sb in frames]
        self.P = max([1] + self.own)
        self.valid = [t // row_bytes for t, _ in frames]

    def cut(self, stride, fid, row, i, j):
        """(global superblock, lo, hi, dst), None for no piece, INVALID for an invalid pair"""
        if fid >= len(self.frames) or row >= self.valid[fid]:
            return INVALID
        total, sb = self.frames[fid]
        c = model_cut(self.row_bytes, stride, total, sb, row, i, j)
        return None if c is None else (self.first[fid] + c[0],) + c[1:]


def batch_of(T):
    """both geometries of test_cutting_against_the_model with the totals of _totals, and one empty array in the middle"""
    bs = 256 * T
    a, b = sg.base_superblock(T), 3 * bs
    frames = [(t, a) for t in _totals(T, a)[:3]] + [(0, a)] + [(t, b) for t in _totals(T, b)] + [(_totals(T, a)[3], a)]
    assert len(frames) >= 5 and len({sb for _, sb in frames}) == 2
    return frames


def row_sizes_of(T):
    """1 and the block size divide both superblock sizes; 3 * 256 * T and its half divide the small one only (for T where the
    large one is no multiple of three blocks), so the call's P exceeds that frame's own; the others divide neither"""
    bs = 256 * T
    a, b = sg.base_superblock(T), 3 * bs
    return [1, 7, bs, b // 2, b, a, a + 1, 2 * a + 5], a, b


def interesting_rows(total, sb, row_bytes):
    nrows = total // row_bytes
    if nrows == 0:
        return []
    rows = {0, nrows - 1}
    for bnd in range(sb, total + 1, sb):
        rows |= {r for r in ((bnd - 1) // row_bytes, bnd // row_bytes, bnd // row_bytes - 1) if 0 <= r < nrows}
    return sorted(rows)


# ---- the pair-cutting function -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T", [1, 2, 4, 12])
def test_pair_cutting_against_the_model(emul, T):
    frames = batch_of(T)
    m = len(frames)
    totals, sbs = arr([t for t, _ in frames]), arr([s for _, s in frames])
    sizes, a, b = row_sizes_of(T)
    out = (c_uint64 * 4)()
    compared = beyond_own = 0
    for row_bytes in sizes:
        mb = ModelBatch(frames, row_bytes)
        tab = (c_uint64 * (2 + 4 * m))()
        emul.emul_gb_table(m, totals, sbs, row_bytes, tab)
        assert (tab[0], tab[1]) == (mb.P, mb.S), row_bytes
        for f in range(m):
            assert tuple(tab[2 + 4 * f:6 + 4 * f]) == (mb.first[f], mb.nsb[f], mb.valid[f] if frames[f][0] else 0, mb.own[f]), (row_bytes, f)
        if row_bytes in (b // 2, b) and a % row_bytes:
            assert mb.P == 2 and 1 in mb.own, "the call's P exceeds a frame's own"
        i = 0
        for f, (total, sb) in enumerate(frames):
            for row in interesting_rows(total, sb, row_bytes):
                i += 1
                stride = row_bytes + (i % 3) * 67
                covered = 0
                for j in range(mb.P + 1):  # (every j up to P, and P itself: the row has ended)
                    want = mb.cut(stride, f, row, i, j)
                    got = emul.emul_gb_cut_pair(m, totals, sbs, row_bytes, stride, f, row, i, j, out)
                    assert (tuple(out) if got == PIECE else got) == (NONE if want is None else want), (row_bytes, f, row, j)
                    if want is not None:
                        g, lo, hi, dst = want
                        assert j < mb.own[f], "no piece for j beyond the frame's own count"
                        assert mb.first[f] <= g < mb.first[f] + mb.nsb[f] and g - mb.first[f] == row * row_bytes // sb + j
                        assert lo < hi <= min(sb, total - (g - mb.first[f]) * sb) and dst == i * stride + covered
                        covered += hi - lo
                        compared += 1
                    elif mb.own[f] <= j < mb.P:
                        beyond_own += 1
                assert covered == row_bytes, "the pieces of a row are the row"
            # the pairs no frame accepts: the row behind the last, huge values, frame numbers from m on
            for fid, row in ((f, total // row_bytes), (f, 1 << 63), (f, (1 << 64) - 1), (m, 0), (1 << 63, 0), ((1 << 64) - 1, 0)):
                for j in range(mb.P):
                    assert emul.emul_gb_cut_pair(m, totals, sbs, row_bytes, row_bytes, fid, row, 3, j, out) == INVALID, (row_bytes, fid, row)
    assert compared > 200 and beyond_own > 10, (compared, beyond_own)


def test_pair_cutting_at_large_values(emul):
    """arrays beyond 2^32 bytes among small ones, slot offsets beyond 2^40: Python integers are the model, nothing wraps there"""
    sb = 131072
    frames = [(3 * sb + 5, sb), ((1 << 32) + 5 * sb + 1003, sb), (0, sb), ((1 << 40) + 77, 3 * 1024), (2 * sb, sb)]
    m = len(frames)
    totals, sbs = arr([t for t, _ in frames]), arr([s for _, s in frames])
    out = (c_uint64 * 4)()
    slots = [(0, lambda rb: rb), (1, lambda rb: (1 << 32) + rb), ((1 << 20) + 2, lambda rb: max(rb, 4096)), ((1 << 40) // 4101 + 1, lambda rb: rb + 4101),
             (5, lambda rb: (1 << 40) + rb)]
    n = passed40 = big_g = 0
    for row_bytes in (1, 7, 4101, sb + 5):
        mb = ModelBatch(frames, row_bytes)
        assert mb.S < (1 << 31)
        for f, (total, fsb) in enumerate(frames):
            nrows = total // row_bytes
            rows = {r for r in (0, nrows - 1, nrows - 2, (1 << 32) // row_bytes, ((1 << 32) - 1) // row_bytes, (1 << 31) // row_bytes) if 0 <= r < nrows}
            for row in sorted(rows):
                for i, fs in slots:
                    stride = fs(row_bytes)
                    covered = 0
                    for j in range(mb.P + 1):
                        want = mb.cut(stride, f, row, i, j)
                        got = emul.emul_gb_cut_pair(m, totals, sbs, row_bytes, stride, f, row, i, j, out)
                        assert (tuple(out) if got == PIECE else got) == (NONE if want is None else want), (row_bytes, f, row, i, j)
                        if want is not None:
                            g, lo, hi, dst = want
                            assert j < mb.own[f] and g < (1 << 31) and hi < (1 << 32) and dst < (1 << 64) and dst == i * stride + covered
                            covered += hi - lo
                            passed40 += dst >= (1 << 40)
                            big_g += g >= (1 << 24)
                            n += 1
                    assert covered == row_bytes
            assert emul.emul_gb_cut_pair(m, totals, sbs, row_bytes, row_bytes, f, nrows, 0, 0, out) == INVALID
    assert n > 200 and passed40 > 40 and big_g > 40, (n, passed40, big_g)


# ---- the whole plan ------------------------------------------------------------------------------------------------------

def run_plan(emul, frames, row_bytes, stride, pairs):
    m, n = len(frames), len(pairs)
    mb = ModelBatch(frames, row_bytes)
    totals, sbs = arr([t for t, _ in frames]), arr([s for _, s in frames])
    bound = min(mb.S, n * mb.P) + n * mb.P // 64  # stenos_g_decode_waves(S, n * P) of csrc/gather.h
    pieces, chunks, info = (c_uint64 * (4 * n * mb.P + 4))(), (c_uint64 * (4 * bound + 4))(), (c_uint64 * 5)()
    r = emul.emul_gb_plan(m, totals, sbs, row_bytes, stride, n, arr([p[0] for p in pairs]), arr([p[1] for p in pairs]), pieces, chunks, bound, info)
    assert r == 0, "more wavefronts with work than stenos_g_decode_waves allows"
    npieces, waves, bad, P, S = info
    assert (P, S) == (mb.P, mb.S) and waves <= bound
    got = [tuple(pieces[4 * k:4 * k + 4]) for k in range(npieces)]
    ch = [tuple(chunks[4 * w:4 * w + 4]) for w in range(waves)]
    return mb, got, ch, bool(bad)


def check_plan(emul, frames, row_bytes, stride, pairs):
    mb, got, ch, bad = run_plan(emul, frames, row_bytes, stride, pairs)
    want, any_bad = [], False
    for i, (fid, row) in enumerate(pairs):
        for j in range(mb.P):
            c = mb.cut(stride, fid, row, i, j)
            if c == INVALID:
                any_bad = True
            elif c is not None:
                want.append(c)
    assert bad == any_bad, "the flag is set exactly when a pair is invalid"
    assert Counter(got) == Counter(want), "the multiset of pieces is the model's"
    # the chunks tile the table in order; each holds 1..64 pieces of exactly one superblock, which lies in the frame it names
    at = 0
    per_sb = Counter(g for g, _, _, _ in got)
    seen = Counter()
    for g, f, first, count in ch:
        assert first == at and 1 <= count <= 64, (g, first, count)
        assert all(p[0] == g for p in got[first:first + count]), "a chunk holds pieces of one superblock"
        assert mb.first[f] <= g < mb.first[f] + mb.nsb[f], "the frame found holds the superblock"
        seen[g] += count
        at += count
    assert at == len(got) and seen == per_sb
    assert len(ch) == sum(-(-c // 64) for c in per_sb.values()), "ceil(count / 64) wavefronts per superblock"
    return mb, got, ch


@pytest.mark.parametrize("T", [2, 4, 12])
def test_plan_against_the_model(emul, T):
    frames = batch_of(T)
    rng = np.random.default_rng([61, T])
    sizes, a, b = row_sizes_of(T)
    full = chunks = 0
    for row_bytes in sizes:
        pairs = []
        for f, (total, sb) in enumerate(frames):
            nrows = total // row_bytes
            if nrows:
                pairs += [(f, int(r)) for r in rng.integers(0, nrows, min(200, 3 * nrows))]
                pairs += [(f, r) for r in interesting_rows(total, sb, row_bytes)]
        # exactly 64 and 65 rows of one interior superblock of a middle frame (where 65 rows fit in one)
        f, (total, sb) = 5, frames[5]
        if sb // row_bytes >= 66:
            first = -(-sb // row_bytes)
            pairs += [(f, first + k) for k in range(64)] + [(f, first + k) for k in range(65)]
        order = rng.permutation(len(pairs))
        pairs = [pairs[int(k)] for k in order] + pairs[:5]
        _, got, ch = check_plan(emul, frames, row_bytes, row_bytes + 67, pairs)
        full += sum(c == 64 for _, _, _, c in ch)
        chunks += len(ch)
    assert full >= 4 and chunks > 100, (full, chunks)


def test_invalid_pairs_make_no_piece_and_set_the_flag(emul):
    T = 4
    a, b = sg.base_superblock(T), 3 * 256 * T
    frames = [(b + 100, b), (3 * a + 300, a), (0, a), (2 * b, b)]
    m, row_bytes = len(frames), 100
    small_rows, large_rows = frames[0][0] // row_bytes, frames[1][0] // row_bytes
    assert small_rows < large_rows  # (the row the small frame refuses is one the larger frame accepts)
    good = [(0, 0), (1, large_rows - 1), (3, 5), (1, small_rows), (0, small_rows - 1)]
    mb, got, _ = check_plan(emul, frames, row_bytes, 128, good)
    assert len(got) >= len(good)
    for bad_pair in ((m, 0), (1 << 63, 0), (0, small_rows), (2, 0), (1, 1 << 63)):
        pairs = good[:2] + [bad_pair] + good[2:]
        mb, with_bad, ch, flag = run_plan(emul, frames, row_bytes, 128, pairs)
        assert flag, bad_pair
        # the same pieces as without it, the slots behind it one further on
        _, without, _, flag0 = run_plan(emul, frames, row_bytes, 128, good[:2] + [(0, 0)] + good[2:])
        assert not flag0
        drop = Counter(without) - Counter(with_bad)
        assert sum(drop.values()) == 1 and list(drop)[0][3] // 128 == 2, "only the bad pair's slot gets nothing"
        assert not Counter(with_bad) - Counter(without)
        check_plan(emul, frames, row_bytes, 128, pairs)
    # nothing but invalid pairs, and a batch of empty arrays only: no piece, no wavefront
    for fr, pairs in ((frames, [(m, 0), (2, 0)]), ([(0, a), (0, b)], [(0, 0), (1, 0)])):
        _, got, ch, flag = run_plan(emul, fr, row_bytes, 128, pairs)
        assert flag and got == [] and ch == []


# ---- the entry points ----------------------------------------------------------------------------------------------------

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
    for name in NAMES:
        assert re.search(r"STENOS_EXPORT[^;(]*\b" + name + r"\s*\(", text), name
        assert name in exported and name in lib._stenos_symbols, name
    from stenos_amd.api import Stenos

    assert callable(Stenos.gather_rows_batch) and callable(Stenos.frames_index)
    # the header says what is not checked, how an empty array differs from the single call, and who is served by what
    comment = text[:text.index("STENOS_EXPORT size_t " + NAMES[0])].rsplit("/*", 1)[1]
    assert "WHAT IS CHECKED" in comment and "NOT detected" in comment and "EMPTY array" in comment and "WHO IS SERVED BY WHAT" in comment
    assert "stenos_hip_gather_rows" in comment and "large frame" in comment


def _call(lib, ctx, n, m=3, T=4, row_bytes=16, stride=16, frames=True, sizes=True, ids=0x200000, rows=0x300000, dst=0x100000):
    """(the device pointers are made up: a call that went on would fault)"""
    P, Z = ctypes.c_void_p * 3, ctypes.c_size_t * 3
    return lib.stenos_hip_gather_rows_batch(ctx, m, T, P(0x1000, 0x2000, 0x3000) if frames else None, Z(4096, 4096, 4096) if sizes else None, row_bytes, n, ids, rows, dst,
                                            stride, None, None)


def test_no_rows_is_no_work(lib):
    ctx = lib.stenos_make_context()
    try:
        assert _call(lib, ctx, 0) == 0
        assert _call(lib, ctx, 0, m=0, row_bytes=0, frames=False, sizes=False) == 0
    finally:
        lib.stenos_destroy_context(ctx)


def test_refusals_that_need_no_device(lib):
    ctx = lib.stenos_make_context()
    try:
        bad = E(9)  # STENOS_ERROR_INVALID_PARAMETER
        assert _call(lib, ctx, 3, m=0) == bad
        assert _call(lib, ctx, 3, m=1 << 31) == bad
        assert _call(lib, ctx, 3, row_bytes=0) == bad
        assert _call(lib, ctx, 3, row_bytes=16, stride=15) == bad
        assert _call(lib, ctx, 3, T=0) == bad and _call(lib, ctx, 3, T=65) == bad
        assert _call(lib, ctx, 1 << 61, row_bytes=8, stride=8) == bad  # n * row_bytes
        assert _call(lib, ctx, 3, row_bytes=1 << 63, stride=1 << 63) == bad
        assert _call(lib, ctx, (1 << 40) + 1, row_bytes=1, stride=1 << 24) == bad  # (n - 1) * dst_stride + row_bytes
        assert _call(lib, ctx, 2, row_bytes=16, stride=(1 << 64) - 8) == bad
        for kw in (dict(frames=False), dict(sizes=False), dict(ids=None), dict(rows=None), dict(dst=None)):
            assert _call(lib, ctx, 3, **kw) == bad, kw
        n = ctypes.c_size_t(7)
        assert not lib.stenos_hip_frames_index(ctx, 0, 4, None, None, ctypes.byref(n), None) and n.value == 0
    finally:
        lib.stenos_destroy_context(ctx)


def test_no_gpu_means_loud_failure(lib):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    ctx = lib.stenos_make_context()
    try:
        assert _call(lib, ctx, 3) == E(5)  # STENOS_ERROR_INVALID_INSTRUCTION_SET
        P, Z = ctypes.c_void_p * 1, ctypes.c_size_t * 1
        n = ctypes.c_size_t(7)
        assert not lib.stenos_hip_frames_index(ctx, 1, 4, P(0x1000), Z(4096), ctypes.byref(n), None) and n.value == 0
    finally:
        lib.stenos_destroy_context(ctx)


# ---- build properties of gather_batch_decode -----------------------------------------------------------------------------

KEYS = [f"gather_batch_decodeILj{T}E" for T in (2, 4, 8, 0)]


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_batch_decoder_has_no_divergent_branch():
    p = subprocess.run([os.path.join(ROOT, "tools", "divergent_branches.sh"), "gather_batch_kernels.hip"] + KEYS, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert [l for l in lines if l.startswith("== ")] == [f"== {k}" for k in KEYS], p.stdout[-1500:]
    assert [l for l in lines if not l.startswith("== ")] == [], "divergent branches:\n" + p.stdout[-1500:]


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_batch_kernel_resources():
    """no scratch memory, no spilled vector register, the occupancy of gather_decode; and the names the budget tests of the other
    decoders key on stay unique"""
    cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-c",
           os.path.join(ROOT, "stenos_amd", "csrc", "gather_batch_kernels.hip"), "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage", "-mllvm",
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
    for key in KEYS:
        hits = [v for k, v in res.items() if key in k]
        assert len(hits) == 1, (key, list(res))
        assert hits[0]["ScratchSize"] == 0 and hits[0]["VGPRs Spill"] == 0, (key, hits[0])
        assert hits[0]["Occupancy"] == (7 if key == "gather_batch_decodeILj4E" else 8), (key, hits[0])
    for name in res:
        assert ("decode_superblocksILj" not in name and "encode_superblocksILj" not in name and "decode_frames_batchILj" not in name
                and "decode_rangesILj" not in name and "gather_decodeILj" not in name), name
