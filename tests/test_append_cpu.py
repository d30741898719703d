"""CPU-side checks of stenos_hip_append (include/stenos_hip.h): what one thread or wavefront of append_plan, append_commit_plan
and append_commit does (csrc/append_codec.h) in the host emulation (tests/emul_append: plain and with the access audit) against a
Python model; refused indices; the prefix property of the format on the C oracle; declared, exported and bound; the refusals
that need no device; loud failure without one; the build properties of csrc/append_kernels.hip.

Every case runs in both builds.  The audited one checks every global access: reads against one arena that ENDS with the old
frame's last byte (words, index, the encoder's offsets and streams, the frame), writes against the words and the index during the
planning steps, then the 7 size bytes of the header, then [p, new total) of the frame's buffer.  The buffer stands between 64
guard bytes of 0xA5, is pre-filled with 0xA5 behind the frame and shifted off its alignment, and is compared WHOLE: after a
refusal it must be what it was.  The frames are made of stored superblocks (code 6), so that "decoding" is slicing, the test hands
in the encoded streams itself, and the expected result is simply the stored frame of A||B."""
import ctypes
import os
import re
import shutil
import subprocess
from ctypes import c_char_p, c_int, c_size_t, c_uint32, c_uint64, c_void_p

import numpy as np
import pytest

from _libs import ROOT, has_error, load_oracle, np_ptr
from stenos_amd.api import load_library
from test_update_cpu import stored_frame

NAME = "stenos_hip_append"
E = lambda k: (1 << 64) - k  # noqa: E731
W_STATUS, W_P, W_TOTAL, W_LEN0, W_LEN1 = 0, 2, 4, 6, 8
ST_TRUNCATED, ST_INVALID, ST_HOST_CODES = 1, 2, 4
GUARD = 64
MIS = [(0, 0), (1, 5), (15, 3), (7, 15)]  # (frame's buffer, encoded streams)


def _load(name):
    d = os.path.join(ROOT, "tests", "emul_append")
    subprocess.check_call(["make", "-C", d], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    lib = ctypes.CDLL(os.path.join(d, name))
    vp, u32, sz, u64 = c_void_p, c_uint32, c_size_t, c_uint64
    lib.emul_append.restype = sz
    lib.emul_append.argtypes = [vp, sz, sz, vp, sz, u32, u32, u32, u32, u32, u64, vp, sz, u64, vp, sz, c_int, c_int, vp, vp, vp, vp]
    lib.emul_audit_first_name.restype = c_char_p
    lib.emul_append_audited.restype = c_int
    lib.emul_append_plan_threads.restype = u32
    lib.emul_append_commit_chunk.restype = u32
    return lib


@pytest.fixture(scope="module")
def builds():
    plain, audit = _load("libstenos_emul_append.so"), _load("libstenos_emul_append_audit.so")
    assert plain.emul_append_audited() == 0 and audit.emul_append_audited() == 1
    return plain, audit


def _clean(lib, rep, what):
    off = int(rep[3]) - (1 << 64) if int(rep[3]) >> 63 else int(rep[3])
    assert rep[0] == 0, (f"{what}: {rep[0]} accesses outside their arena, first: {lib.emul_audit_first_name().decode()} kind {rep[2]} "
                         f"(1 global read, 2 global write) at arena offset {off}, {rep[4]} bytes")
    if lib.emul_append_audited():
        assert rep[1] > 0, what


def word64(words, w):
    return int(words[w]) | (int(words[w + 1]) << 32)


def stored_stream(raw, sb):
    """the bytes as independent stored superblocks without a frame header: (stream, its offsets from 0)"""
    parts = [bytes([6]) + len(raw[o:o + sb]).to_bytes(3, "little") + bytes(raw[o:o + sb]) for o in range(0, len(raw), sb)]
    return b"".join(parts), np.cumsum([0] + [len(p) for p in parts]).astype(np.uint64)


def encoder_output(tail, B, sb, gap):
    """what the host hands append_commit_plan: the stitched superblock (r > 0) and the rest of B as two streams, `gap` bytes apart,
    and the encoder's offsets, the first stream's entries in front.  Returns (enc, enc_off, enc_base1, k, k0)."""
    r = len(tail)
    n0 = min(len(B), sb - r) if r else 0
    streams = []
    if r:
        streams.append(stored_stream(np.concatenate([tail, B[:n0]]), sb))
    if len(B) > n0:
        streams.append(stored_stream(B[n0:], sb))
    k0 = 1 if r else 0
    k = sum(len(o) - 1 for _, o in streams)
    enc_base1 = len(streams[0][0]) + gap if len(streams) == 2 else 0
    enc = bytearray(streams[0][0])
    if len(streams) == 2:
        enc += bytes([0x5A]) * gap + streams[1][0]
    enc_off = np.concatenate([o for _, o in streams])
    return np.frombuffer(bytes(enc), dtype=np.uint8).copy(), enc_off, enc_base1, k, k0


def call(lib, frame, cap, idx, keep, r, k, k0, header, new_bytes, enc, enc_off, enc_base1, mis):
    new_idx = np.zeros(keep + k + 1, dtype=np.uint64)
    words = np.zeros(16, dtype=np.uint32)
    buf = np.zeros(cap + 2 * GUARD, dtype=np.uint8)
    rep = np.zeros(5, dtype=np.uint64)
    enc_off = np.ascontiguousarray(enc_off, dtype=np.uint64)
    res = lib.emul_append(np_ptr(frame), frame.size, cap, np_ptr(idx), idx.size, keep, r, k, k0, header, new_bytes, np_ptr(enc), enc.size, enc_base1, np_ptr(enc_off),
                          enc_off.size, mis[0], mis[1], np_ptr(new_idx), np_ptr(words), np_ptr(buf), np_ptr(rep))
    assert res != E(3)
    _clean(lib, rep, "append_plan / append_commit_plan / append_commit")
    return res, new_idx, words, buf


def untouched(frame, cap):
    return np.concatenate([np.full(GUARD, 0xA5, np.uint8), frame, np.full(cap - frame.size + GUARD, 0xA5, np.uint8)])


def run_case(builds, rng, sb, header, keep, r, nbytes, turn, codes=None):
    total = keep * sb + r
    data = rng.integers(0, 256, total, dtype=np.uint8)
    B = rng.integers(0, 256, nbytes, dtype=np.uint8)
    frame, idx = stored_frame(data, sb, header, codes)
    want, want_idx = stored_frame(np.concatenate([data, B]), sb, header, {s: c for s, c in (codes or {}).items() if s < keep})
    enc, enc_off, enc_base1, k, k0 = encoder_output(data[keep * sb:], B, sb, 5 + turn % 29)
    assert keep + k == want_idx.size - 1
    p = int(idx[keep])
    assert np.array_equal(want[header:p], frame[header:p]) and np.array_equal(want_idx[:keep + 1], idx[:keep + 1])
    cap = want.size + 40
    got = []
    for lib in builds:
        mis = MIS[(turn + (lib is builds[1])) % len(MIS)]
        res, new_idx, words, buf = call(lib, frame, cap, idx, keep, r, k, k0, header, total + nbytes, enc, enc_off, enc_base1, mis)
        assert res == want.size, (hex(res), want.size)
        assert np.array_equal(new_idx, want_idx)
        assert word64(words, W_P) == p and word64(words, W_TOTAL) == want.size and word64(words, W_LEN0) + word64(words, W_LEN1) == want.size - p
        assert not words[W_STATUS] & (ST_TRUNCATED | ST_INVALID)
        assert bool(words[W_STATUS] & ST_HOST_CODES) == bool(r and (codes or {}).get(keep, 6) in (2, 3, 4, 5))
        assert np.array_equal(buf, untouched(want, cap)), "the buffer is not guard | frame of A||B | 0xA5 | guard"
        # one byte short: refused, the whole buffer as it was
        res2, _, _, buf2 = call(lib, frame, want.size - 1, idx, keep, r, k, k0, header, total + nbytes, enc, enc_off, enc_base1, mis)
        assert res2 == E(6)
        assert np.array_equal(buf2, untouched(frame, want.size - 1)), "a refused append wrote to the buffer"
        got.append(bytes(buf))
    assert got[0] == got[1], "the result depends on the build"
    return k


# ---- the planning and commit steps ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sb", [64, 256, 1024])
def test_plan_and_commit_against_the_model(builds, sb):
    rng = np.random.default_rng([61, sb])
    turn = 0
    seen = set()
    for header in (8, 12):
        for keep in (0, 1, 3):
            for r in (0, 1, sb - 1):
                if keep == 0 and r == 0:
                    continue  # (the frame of an empty array: stenos_hip_compress, not these kernels)
                for k in (1, 2, 5):
                    for last in (1, sb // 2, sb):  # bytes of the new last superblock
                        nbytes = (k - 1) * sb + last - r
                        if nbytes <= 0:
                            continue
                        assert run_case(builds, rng, sb, header, keep, r, nbytes, turn) == k
                        seen.add((r > 0, k > 1))
                        turn += 1
    assert len(seen) == 4 and turn > 100


def test_long_frames_and_more_new_superblocks_than_planning_threads(builds):
    rng = np.random.default_rng(62)
    threads, chunk = builds[0].emul_append_plan_threads(), builds[0].emul_append_commit_chunk()
    # a frame of 2 500 superblocks, the last one partial
    assert run_case(builds, rng, 64, 8, 2499, 33, 5 * 64, 1) == 6
    assert run_case(builds, rng, 64, 12, 2500, 0, 3 * 64 + 1, 2) == 4
    # more new superblocks than one workgroup of append_commit_plan has threads, in a stream of several copy chunks
    k = 2 * threads + 3
    assert k * 68 > 2 * chunk
    assert run_case(builds, rng, 64, 8, 3, 40, (k - 1) * 64 - 40 + 7, 3) == k
    assert run_case(builds, rng, 64, 8, 2, 0, threads * 64 + 1, 4) == threads + 1
    # both streams longer than a chunk cannot be (the first is one superblock); a second stream that ends on a chunk boundary
    sb = 1024
    per = chunk // (sb + 4)
    assert run_case(builds, rng, sb, 8, 1, 100, (sb - 100) + per * sb, 5) == per + 1


def test_a_zstd_based_code_of_the_last_superblock_is_flagged(builds):
    rng = np.random.default_rng(63)
    for code in (2, 3, 4, 5):
        run_case(builds, rng, 256, 8, 2, 100, 300, code, codes={2: code})
    run_case(builds, rng, 256, 8, 2, 0, 300, 9, codes={1: 3})  # (a whole superblock in front: not looked at)


def test_bad_index_entries_are_refused_with_nothing_written(builds):
    rng = np.random.default_rng(64)
    sb, header = 512, 8
    for keep, r in ((3, 9), (3, 0)):
        total = keep * sb + r
        data = rng.integers(0, 256, total, dtype=np.uint8)
        B = rng.integers(0, 256, 1300, dtype=np.uint8)
        frame, idx = stored_frame(data, sb, header)
        enc, enc_off, enc_base1, k, k0 = encoder_output(data[keep * sb:], B, sb, 11)
        cap = 4 * frame.size
        cases = []

        def bad(at, value, code):
            x = idx.copy()
            x[at] = value
            cases.append((x, code))

        bad(keep, header - 1, E(4))  # in front of the first superblock
        bad(keep, 0, E(4))
        if r:
            bad(keep + 1, int(idx[keep]) + 3, E(4))  # a superblock under 4 bytes
            bad(keep + 1, int(idx[keep]) - 1, E(4))  # decreasing
            bad(keep + 1, frame.size + 1, E(2))  # the end beyond the frame
            bad(keep + 1, 1 << 63, E(2))
            # garbage in idx[keep]: the code byte is read inside the frame only (the audit's read arena ends with the frame)
            for at in (frame.size - 3, frame.size, frame.size + 1000, (1 << 64) - 2):
                bad(keep, at, E(4))
            x = idx.copy()
            x[keep], x[keep + 1] = (1 << 64) - 8, (1 << 64) - 2  # both far beyond, four bytes apart
            cases.append((x, E(2)))
        else:
            bad(keep, frame.size + 1, E(2))
            bad(keep, (1 << 64) - 2, E(2))
        for lib in builds:
            ok, _, _, _ = call(lib, frame, cap, idx, keep, r, k, k0, header, total + B.size, enc, enc_off, enc_base1, MIS[1])
            assert not has_error(ok)
            for x, code in cases:
                res, _, words, buf = call(lib, frame, cap, x, keep, r, k, k0, header, total + B.size, enc, enc_off, enc_base1, MIS[2])
                assert res == code, (x.tolist(), hex(res))
                assert words[W_STATUS] & (ST_INVALID | ST_TRUNCATED)
                assert np.array_equal(buf, untouched(frame, cap)), "a refused append wrote to the buffer"
            # offsets the encoder never writes: decreasing, a superblock under 4 bytes, one longer than a header can announce, a
            # stream that does not start at 0
            for at, value in ((enc_off.size - 1, int(enc_off[-2]) + 3), (enc_off.size - 1, int(enc_off[-2]) - 1), (enc_off.size - 1, int(enc_off[-2]) + (1 << 24) + 4), (0, 1)):
                y = enc_off.copy()
                y[at] = value
                res, _, _, buf = call(lib, frame, cap, idx, keep, r, k, k0, header, total + B.size, enc, y, enc_base1, MIS[3])
                assert res == E(4), (at, value, hex(res))
                assert np.array_equal(buf, untouched(frame, cap))


# ---- the prefix property of the format, on the oracle ------------------------------------------------------------------------

def _chain(frame, header):
    idx, p = [], header
    while p < len(frame):
        idx.append(p)
        p += 4 + int.from_bytes(bytes(frame[p + 1:p + 4]), "little")
    assert p == len(frame)
    return idx + [p]


def _data(kind, n, rng):
    if kind == "random":
        return rng.integers(0, 256, n, dtype=np.uint8)
    if kind == "periodic":
        return np.resize(rng.integers(0, 256, 24, dtype=np.uint8), n)
    return (np.arange(n, dtype=np.uint64) // 5 % 251).astype(np.uint8)  # slowly rising


def test_the_frame_of_a_concatenation_starts_with_the_frame_of_its_head():
    """oracle compress(A||B)[8 : p] == oracle compress(A)[8 : p] with an equal index[keep]: what append relies on"""
    oracle = load_oracle()
    rng = np.random.default_rng(65)
    cases = 0
    for level in (0, 1):
        for T in (2, 4, 8, 3, 12, 64):
            sb = oracle.so_superblock_size(T, 1, level)
            assert sb == oracle.so_superblock_size(T, 10 * sb, level)  # (levels 0 and 1 never shift)
            olds = [0, 127, 128, sb - 1, sb, sb + 1, 2 * sb + 256 * T + 3, 3 * sb - 5]
            news = [1, sb - 1, sb + 100, 2 * sb + 5]
            for i, old in enumerate(olds):
                for j, new in enumerate(news):
                    if (i + j + T + level) % 3:  # (the grid, thinned)
                        continue
                    kind = ("random", "periodic", "rising")[(i + j) % 3]
                    ab = _data(kind, old + new, rng)
                    fa = np.zeros(oracle.so_bound(old) + 64, dtype=np.uint8)
                    fab = np.zeros(oracle.so_bound(old + new) + 64, dtype=np.uint8)
                    ra = oracle.so_compress(np_ptr(ab), T, old, np_ptr(fa), oracle.so_bound(old), level)
                    rab = oracle.so_compress(np_ptr(ab), T, old + new, np_ptr(fab), oracle.so_bound(old + new), level)
                    assert not has_error(ra) and not has_error(rab)
                    keep = old // sb
                    ia, iab = _chain(fa[:ra], 8), _chain(fab[:rab], 8)
                    assert ia[keep] == iab[keep], (level, T, old, new)
                    assert np.array_equal(fa[8:ia[keep]], fab[8:ia[keep]]), (level, T, old, new)
                    assert fa[0] == fab[0]
                    cases += 1
    assert cases > 100


# ---- the entry point ----------------------------------------------------------------------------------------------------------

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
    assert re.search(r"STENOS_EXPORT[^;(]*\b" + NAME + r"\s*\(", text)
    assert NAME in exported
    assert NAME in lib._stenos_symbols
    from stenos_amd.api import Stenos

    assert callable(Stenos.append)
    # the header says what stays, what is written, what is not checked, what an empty frame means and where the figures are
    comment = text[:text.index("STENOS_EXPORT size_t " + NAME)].rsplit("/*", 1)[1]
    for phrase in ("IN PLACE", "WRITES TO d_frame", "WHAT IS CHECKED", "NOT detected", "EMPTY array", "stenos_bound", "DEVICE MEMORY", "profiles/append_rate.txt",
                   "stenos_hip_last_index", "unfused"):
        assert phrase in comment, phrase


def _call(lib, ctx, T=4, bytes_=4096, capacity=1 << 20, src=0x300000, src_bytes=1000, frame=0x1000):
    return lib.stenos_hip_append(ctx, frame, T, bytes_, capacity, src, src_bytes, None, None)


def test_refusals_that_need_no_device(lib):
    """(the device pointers are made up: a call that went on would fault)"""
    ctx = lib.stenos_make_context()
    try:
        bad = E(9)  # STENOS_ERROR_INVALID_PARAMETER
        assert _call(lib, ctx, capacity=4095) == bad
        assert _call(lib, ctx, T=0) == bad and _call(lib, ctx, T=65) == bad
        assert _call(lib, ctx, src_bytes=1 << 56) == bad
        assert _call(lib, ctx, frame=None) == bad and _call(lib, ctx, src=None) == bad
        for level in (2, 5, 9):
            lib.stenos_set_level(ctx, level)
            assert _call(lib, ctx) == bad, level
        lib.stenos_set_level(ctx, 1)
        assert _call(lib, ctx, T=1) == bad  # bytesoftype 1 at level 1
        lib.stenos_set_max_nanoseconds(ctx, 1000)
        assert _call(lib, ctx) == bad
    finally:
        lib.stenos_destroy_context(ctx)


def test_no_gpu_means_loud_failure(lib):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    ctx = lib.stenos_make_context()
    try:
        assert _call(lib, ctx) == E(5)  # STENOS_ERROR_INVALID_INSTRUCTION_SET
        assert _call(lib, ctx, src_bytes=0, src=None) == E(5)
    finally:
        lib.stenos_destroy_context(ctx)


# ---- build properties of append_kernels.hip ------------------------------------------------------------------------------------

KEYS = [f"append_decodeILj{T}E" for T in (2, 4, 8, 0)]
OTHERS = ["append_planE", "append_commit_planE", "append_commitE"]


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_append_kernel_resources():
    """no scratch memory, no spilled vector register; the decoder at eight waves per SIMD; and the names the budget tests of the
    other decoders key on stay unique"""
    cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-c", os.path.join(ROOT, "stenos_amd", "csrc", "append_kernels.hip"),
           "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage", "-mllvm", "-structurizecfg-skip-uniform-regions=1"]
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
        if key in KEYS:
            assert hits[0]["Occupancy"] == 8, (key, hits[0])
    for name in res:
        assert ("decode_superblocksILj" not in name and "encode_superblocksILj" not in name and "decode_frames_batchILj" not in name
                and "decode_rangesILj" not in name and "gather_decodeILj" not in name and "update_decodeILj" not in name), name
