"""CPU-side checks of stenos_hip_decompress_ranges (include/stenos_hip.h): the window decoder of csrc/range_codec.h in the host
emulation (tests/emul_ranges: plain and with the access audit), against slices of the oracle's decode; declared, exported and
bound; loud failure without a device; the build properties of decode_ranges (csrc/range_decode_kernels.hip).

Every window is decoded twice: by the plain build (LDS filled with 0xCD) and by the audited one (LDS filled with 0x37; every LDS
and global access checked against the wave's LDS, the 16-byte hull of the payload and [dst, dst + hi - lo) exactly).  Both must
give the slice, and neither may change one of the 64 guard bytes on either side of the destination.  Source misalignments
0, 1, 15 and destination misalignments 0, 1, 3, 15 take turns from window to window."""
import ctypes
import itertools
import os
import re
import shutil
import subprocess
from ctypes import c_char_p, c_int, c_size_t, c_void_p

import numpy as np
import pytest

import streamgen as sg
from _libs import ROOT, has_error, np_ptr
from stenos_amd.api import load_library
from stenos_amd.datagen import generate

NAME = "stenos_hip_decompress_ranges"
E = lambda k: (1 << 64) - k  # noqa: E731
TS = [1, 2, 3, 4, 8, 12, 64]
KINDS = ["rand12", "walk", "dict16", "runs", "mixed", "rand", "lzmix"]
GUARD = 64
MISALIGN = list(itertools.product((0, 1, 15), (0, 1, 3, 15)))  # (source, destination)
DECODE_ERROR = E(4)
CHECKED = [0, 0]  # windows, accesses audited


def _load(name):
    d = os.path.join(ROOT, "tests", "emul_ranges")
    subprocess.check_call(["make", "-C", d], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    lib = ctypes.CDLL(os.path.join(d, name))
    lib.emul_window_decompress.restype = c_size_t
    lib.emul_window_decompress.argtypes = [c_void_p, c_size_t, c_size_t, c_size_t, c_size_t, c_size_t, c_void_p, c_int, c_int]
    lib.emul_set_lds_fill.restype = None
    lib.emul_set_lds_fill.argtypes = [c_int]
    return lib


@pytest.fixture(scope="module")
def plain():
    lib = _load("libstenos_emul_ranges.so")
    lib.emul_set_lds_fill(0xCD)
    return lib


@pytest.fixture(scope="module")
def audit():
    lib = _load("libstenos_emul_ranges_audit.so")
    lib.emul_audit_window_decompress.restype = c_size_t
    lib.emul_audit_window_decompress.argtypes = [c_void_p, c_size_t, c_size_t, c_size_t, c_size_t, c_size_t, c_void_p, c_int, c_int, ctypes.POINTER(ctypes.c_uint64)]
    lib.emul_audit_first_name.restype = c_char_p
    lib.emul_set_lds_fill(0x37)
    return lib


def padded(payload: bytes, slack: int = 64) -> np.ndarray:
    buf = np.zeros(len(payload) + slack, dtype=np.uint8)
    buf[:len(payload)] = np.frombuffer(payload, dtype=np.uint8)
    return buf


def window(plain, audit, buf, csize, T, dsize, lo, n, mis, dmis):
    """-> (result of the plain build, its bytes); the audited build must agree and stay inside its regions"""
    outs = []
    for lib in (plain, audit):
        out = np.full(n + 2 * GUARD + 16, 0xA5, dtype=np.uint8)
        at = GUARD + dmis
        if lib is plain:
            r = lib.emul_window_decompress(np_ptr(buf), csize, T, dsize, lo, lo + n, np_ptr(out) + at, mis, dmis)
        else:
            rep = (ctypes.c_uint64 * 5)()
            r = lib.emul_audit_window_decompress(np_ptr(buf), csize, T, dsize, lo, lo + n, np_ptr(out) + at, mis, dmis, rep)
            off = rep[3] - (1 << 64) if rep[3] >> 63 else rep[3]
            assert rep[0] == 0, (f"T={T} dsize={dsize} [{lo}, {lo + n}) mis={mis}/{dmis}: {rep[0]} accesses outside their region, first: "
                                 f"{lib.emul_audit_first_name().decode()} kind {rep[2]} (0 LDS, 1 global read, 2 global write) at region offset {off}, {rep[4]} bytes")
            CHECKED[1] += rep[1]
        assert r != E(7), f"T={T} dsize={dsize} [{lo}, {lo + n}) mis={mis}/{dmis}: a guard byte of the decoder's destination changed"
        assert (out[:at] == 0xA5).all() and (out[at + n:] == 0xA5).all()
        outs.append((r, out[at:at + n].copy()))
    assert outs[0][0] == outs[1][0] and np.array_equal(outs[0][1], outs[1][1]), (T, dsize, lo, n, "the result depends on the LDS contents or the build")
    CHECKED[0] += 1
    return outs[0]


def windows_of(T, dsize, rng, nrandom=50):
    """(lo, length): the whole superblock, its first and last byte, every block boundary +- 1, inside one row, into the raw
    remainder of the tail, random ones"""
    bs, row = 256 * T, 16 * T
    w = [(0, dsize), (0, 1), (dsize - 1, 1)]
    for b in range(bs, dsize + 1, bs):
        w.append((b - 1, 1))
        if b < dsize:
            w += [(b, 1), (b - 1, 2)]
    w.append((min(dsize - 1, row + 3), max(1, min(row - 5, dsize - 1 - min(dsize - 1, row + 3)))))  # inside one row
    tail = dsize % bs
    if tail:
        tb, raw = dsize - tail, (tail // row) * row  # the tail's rows end at tb + raw; behind them raw bytes
        if raw < tail:
            w += [(max(0, tb + raw - 3), tail - raw + min(3, tb + raw)), (tb + raw, tail - raw), (dsize - 1, 1)]
            if tail - raw > 2:
                w.append((tb + raw + 1, tail - raw - 2))
        w.append((max(0, tb - 5), min(dsize, tb + 7) - max(0, tb - 5)))
    for _ in range(nrandom):
        lo = int(rng.integers(0, dsize))
        w.append((lo, int(rng.integers(1, min(dsize - lo, 1 + int(rng.choice([7, 300, 4 * bs, dsize])))  + 1))))
    return [(lo, n) for lo, n in w if n > 0 and lo + n <= dsize]


def dsizes(T):
    bs = 256 * T
    return [bs, 4 * bs, 4 * bs + 15 * T + 7, max(1, 16 * T - 3), sg.base_superblock(T)]


def check_payload(plain, audit, payload, T, data, rng, turn, windows=None):
    buf = padded(payload)
    dsize = data.size
    for lo, n in windows if windows is not None else windows_of(T, dsize, rng):
        mis, dmis = MISALIGN[next(turn) % len(MISALIGN)]
        r, got = window(plain, audit, buf, len(payload), T, dsize, lo, n, mis, dmis)
        assert r == n, (T, dsize, lo, n, r)
        assert np.array_equal(got, data[lo:lo + n]), (T, dsize, lo, n, mis, dmis)


def oracle_payload(oracle, kind, T, nbytes, seed):
    data = generate(kind, T, (nbytes + T - 1) // T, seed)[:nbytes].copy()
    buf = np.zeros(nbytes * 2 + 4096, dtype=np.uint8)
    r = oracle.so_block_compress(np_ptr(data), T, nbytes, np_ptr(buf), buf.nbytes)
    assert not has_error(r)
    back = np.zeros(nbytes + 64, dtype=np.uint8)
    r2 = oracle.so_block_decompress(np_ptr(buf), r, T, nbytes, np_ptr(back))  # (the reference of every window: slices of this)
    assert not has_error(r2) and np.array_equal(back[:nbytes], data)
    return buf[:r].tobytes(), back[:nbytes].copy()


@pytest.mark.parametrize("T", TS)
def test_windows_of_oracle_payloads(oracle, plain, audit, T):
    """payloads the oracle's block encoder writes, over the data kinds (rand: copied blocks; lzmix: mini-LZ blocks)"""
    rng = np.random.default_rng([11, T])
    turn = itertools.count(T)
    before = CHECKED[0]
    for k, kind in enumerate(KINDS):
        if kind == "rand12" and T != 4:
            continue
        sizes = dsizes(T)
        for dsize in sizes:
            payload, data = oracle_payload(oracle, kind, T, dsize, 40 + k)
            check_payload(plain, audit, payload, T, data, rng, turn)
    assert CHECKED[0] - before > 1000


@pytest.mark.parametrize("T", TS)
def test_windows_of_free_choice_payloads(plain, audit, T):
    """legal streams no encoder writes (tests/streamgen.py): every block kind and plane form, oversize blocks, tails"""
    rng = np.random.default_rng([12, T])
    turn = itertools.count(3 * T)
    for name, ch in sg.VARIANTS.items():
        if name.startswith("lz") and not sg.lz_width(T):
            continue
        for dsize in (4 * 256 * T + 15 * T + 7, max(1, 16 * T - 3)) if name in ("legal", "oversize", "copy", "lz") else (2 * 256 * T + 37 * T + 5,):
            data = sg.make_data(rng, T, dsize, sg.DATA_STYLE.get(name))
            payload = sg.encode_payload(data, T, ch, rng)
            check_payload(plain, audit, payload, T, data, rng, turn, windows_of(T, dsize, rng, nrandom=12))


def _blocks(T, rng, kinds):
    """-> (data, the blocks' encodings): full blocks of the given kinds"""
    bs = 256 * T
    data = sg.make_data(rng, T, len(kinds) * bs, None)
    return data, [sg.encode_block(data[b * bs:(b + 1) * bs], T, sg.PLANES_ONLY, rng, kind) for b, kind in enumerate(kinds)]


@pytest.mark.parametrize("T", [2, 3, 4, 8, 12])
def test_truncated_in_front_is_an_error_and_damage_behind_is_not_seen(plain, audit, T):
    rng = np.random.default_rng([13, T])
    bs = 256 * T
    for kinds in (("planes", "planes", "planes", "planes"), ("planes", "copy", "planes", "planes"), ("copy", "copy", "copy", "copy")):
        data, enc = _blocks(T, rng, kinds)
        payload = b"".join(enc)
        buf = padded(payload)
        lo, n = 3 * bs + 11, 40  # inside the last block
        r, got = window(plain, audit, buf, len(payload), T, data.size, lo, n, 1, 3)
        assert r == n and np.array_equal(got, data[lo:lo + n])
        # the payload ends inside block 1, in front of the window: the chain cannot be followed
        cut = len(enc[0]) + len(enc[1]) // 2
        r, _ = window(plain, audit, buf, cut, T, data.size, lo, n, 0, 1)
        assert r == DECODE_ERROR, (T, kinds, r)
        # ... or inside block 2, right behind a block that is stepped over
        cut = len(enc[0]) + len(enc[1]) + 1
        r, _ = window(plain, audit, buf, cut, T, data.size, lo, n, 15, 0)
        assert r == DECODE_ERROR, (T, kinds, r)
        # damage behind the block that holds the window's last byte is not looked at
        bad = buf.copy()
        start = len(enc[0]) + len(enc[1])
        bad[start:len(payload)] = 0xFF
        lo1, n1 = bs - 7, 7 + bs  # blocks 0 and 1, to the last byte of block 1
        r, got = window(plain, audit, bad, len(payload), T, data.size, lo1, n1, 1, 15)
        assert r == n1 and np.array_equal(got, data[lo1:lo1 + n1]), (T, kinds, r)
        # ... while a window that reaches into it sees it
        r, _ = window(plain, audit, bad, len(payload), T, data.size, lo1, n1 + 1, 0, 0)
        assert r == DECODE_ERROR, (T, kinds, r)


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
    assert re.search(r"STENOS_EXPORT[^;(]*\b" + NAME + r"\s*\(", text)
    assert NAME in exported
    assert NAME in lib._stenos_symbols
    from stenos_amd.api import Stenos

    assert callable(Stenos.decompress_ranges) and callable(Stenos.decompress_range)
    # the two index functions say that a ranges call leaves their buffer alone
    for fn in ("stenos_hip_last_index", "stenos_hip_frame_index"):
        comment = text[:text.index("STENOS_EXPORT const uint64_t* " + fn)].rsplit("/*", 1)[1]
        assert NAME in comment, fn


def _call(lib, ctx, n):
    U, P = ctypes.c_uint64 * max(n, 1), ctypes.c_void_p * max(n, 1)
    return lib.stenos_hip_decompress_ranges(ctx, 0x1000, 4, 4096, n, U(*[0] * max(n, 1)), U(*[16] * max(n, 1)), P(*[0x100000] * max(n, 1)), None, None)


def test_no_ranges_is_no_work(lib):
    ctx = lib.stenos_make_context()
    try:
        assert _call(lib, ctx, 0) == 0  # (the device pointers are made up: a call that went on would fault)
    finally:
        lib.stenos_destroy_context(ctx)


def test_no_gpu_means_loud_failure(lib):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    ctx = lib.stenos_make_context()
    try:
        assert _call(lib, ctx, 3) == E(5)  # STENOS_ERROR_INVALID_INSTRUCTION_SET
    finally:
        lib.stenos_destroy_context(ctx)


# ---- build properties of decode_ranges ---------------------------------------------------------------------------------

KEYS = [f"decode_rangesILj{T}E" for T in (2, 4, 8, 0)]


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_range_decoder_has_no_divergent_branch():
    p = subprocess.run([os.path.join(ROOT, "tools", "divergent_branches.sh"), "range_decode_kernels.hip"] + KEYS, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert [l for l in lines if l.startswith("== ")] == [f"== {k}" for k in KEYS], p.stdout[-1500:]
    assert [l for l in lines if not l.startswith("== ")] == [], "divergent branches:\n" + p.stdout[-1500:]


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_range_kernel_resources():
    """no scratch memory, no spilled vector register; and the names the budget tests of the other decoders key on stay unique"""
    cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-c", os.path.join(ROOT, "stenos_amd", "csrc", "range_decode_kernels.hip"),
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
    for key in KEYS:
        hits = [v for k, v in res.items() if key in k]
        assert len(hits) == 1, (key, list(res))
        assert hits[0]["ScratchSize"] == 0 and hits[0]["VGPRs Spill"] == 0, (key, hits[0])
    for name in res:
        assert "decode_superblocksILj" not in name and "encode_superblocksILj" not in name and "decode_frames_batchILj" not in name, name
