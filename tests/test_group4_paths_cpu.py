"""The groups of four int32 blocks of the fused encoder (superblock_codec.h: group4) and the straight-line emission of a second
pass made of packed rows of values (slot_codec.h: slot_rows_emit_rows_packed; the key counts of the four blocks taken at once,
lz_distinct_keys_group4), in the host emulation against the oracle, bytes equal.  Inputs: tests/group4_inputs.py -- a kind for
every precondition a fast path tests and one that breaks it in the second, third or fourth block of a group.  Shapes: one group
(4 blocks), a group and a remainder (5), groups on both sides of a changed block (9), a superblock and three blocks (131).
No GPU: it proves the kernel logic, not the shipped binary (tests/test_gpu_group4_paths.py does that)."""
import ctypes
import os
import subprocess
from ctypes import c_int, c_size_t, c_void_p

import numpy as np
import pytest

import group4_inputs as g4in
from _libs import ROOT, np_ptr, oracle_compress

RUNS = [(kind, n, pos) for kind in g4in.KINDS for n in (4, 5, 9) for pos in (1, 2, 3)]
RUNS_THRESHOLD = [("low_count", n, pos, d) for d in g4in.THRESHOLD_COUNTS for n, pos in ((4, 1), (9, 3))]


@pytest.fixture(scope="module")
def emul():
    d = os.path.join(ROOT, "tests", "emul")
    subprocess.check_call(["make", "-C", d], stdout=subprocess.DEVNULL)
    lib = ctypes.CDLL(os.path.join(d, "libstenos_emul_enc.so"))
    lib.emul_run_compress.restype = c_size_t
    lib.emul_run_compress.argtypes = [c_void_p, c_size_t, c_size_t, c_void_p]
    lib.emul_compress_frame.restype = c_size_t
    lib.emul_compress_frame.argtypes = [c_void_p, c_size_t, c_size_t, c_void_p, c_size_t, c_int]
    lib.emul_group4_count.restype = c_size_t
    lib.emul_set_fused.argtypes = [c_int]
    lib.emul_set_slots.argtypes = [c_int]
    lib.emul_set_fused(1)
    lib.emul_set_slots(1)
    return lib


def _oracle_blocks(oracle, data):
    ref = np.zeros(data.nbytes * 2 + 4096, dtype=np.uint8)
    r = oracle.so_block_compress(np_ptr(data), 4, data.nbytes, np_ptr(ref), ref.nbytes)
    return ref[:r]


@pytest.mark.parametrize("kind,n,pos", RUNS, ids=[f"{k}-{n}-{p}" for k, n, p in RUNS])
def test_a_run_of_blocks_matches_the_oracle(oracle, emul, kind, n, pos):
    data = g4in.make(kind, n, pos)
    ref = _oracle_blocks(oracle, data)
    out = np.zeros(data.nbytes * 2 + 4096, dtype=np.uint8)
    before = emul.emul_group4_count()
    r = emul.emul_run_compress(np_ptr(data), 4, n, np_ptr(out))
    took = emul.emul_group4_count() - before
    assert r == ref.size and np.array_equal(out[:r], ref), (kind, n, pos)
    if g4in.KINDS[kind][0]:
        assert took == n // 4, (kind, n, pos, took)
    elif n < 8:
        assert took == 0, (kind, n, pos, took)
    else:
        assert took < n // 4, (kind, n, pos, took)


@pytest.mark.parametrize("kind,n,pos,distinct", RUNS_THRESHOLD, ids=[f"{d}-{n}" for _, n, _, d in RUNS_THRESHOLD])
def test_key_counts_around_the_mini_lz_threshold(oracle, emul, kind, n, pos, distinct):
    data = g4in.make(kind, n, pos, distinct=distinct)
    ref = _oracle_blocks(oracle, data)
    out = np.zeros(data.nbytes * 2 + 4096, dtype=np.uint8)
    r = emul.emul_run_compress(np_ptr(data), 4, n, np_ptr(out))
    assert r == ref.size and np.array_equal(out[:r], ref), (n, distinct)


@pytest.mark.parametrize("kind", list(g4in.KINDS))
def test_a_superblock_and_three_blocks_match_the_oracle(oracle, emul, kind):
    """A frame: the runs of a superblock's waves, then a superblock of three blocks that no group takes."""
    n = 128 + 3
    data = g4in.make(kind, n, 2)
    cap = oracle.so_bound(data.nbytes) + 5000
    r1, f1 = oracle_compress(oracle, data, 4, 1, cap)
    out = np.zeros(cap, dtype=np.uint8)
    before = emul.emul_group4_count()
    r2 = emul.emul_compress_frame(np_ptr(data), 4, data.nbytes, np_ptr(out), cap, 1)
    took = emul.emul_group4_count() - before
    assert r2 == r1 and np.array_equal(out[:r2], f1), kind
    if g4in.KINDS[kind][0]:
        assert took >= 128 // 4 - 4, (kind, took)  # (a wave's run need not be a multiple of four blocks)
    else:
        assert took < 128 // 4, (kind, took)


@pytest.fixture(scope="module")
def programs():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "emul_group4")], stdout=subprocess.DEVNULL)
    return {name: os.path.join(ROOT, "build", name) for name in ("emul_group4", "emul_group4_san")}


def _all_runs():
    runs = [(g4in.make(kind, n, pos), kind, n) for kind, n, pos in RUNS if n != 5 or pos == 1]
    runs += [(g4in.make(kind, n, pos, distinct=d), kind, n) for kind, n, pos, d in RUNS_THRESHOLD]
    return runs


@pytest.mark.parametrize("name", ["emul_group4", "emul_group4_san"])
def test_the_runs_in_a_program_of_its_own_plain_and_sanitized(oracle, programs, tmp_path, name):
    """Every run above in one call of the stand-alone program (tests/emul_group4): streams equal the oracle's, the groups are
    taken where they are meant to be, and the straight-line emission exactly where its precondition holds.  The sanitized build
    (input, LDS and staging are mallocs of their exact sizes) has to come through without a report."""
    runs = _all_runs()
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(b"".join(d.tobytes() for d, _, _ in runs))
    p = subprocess.run([programs[name], str(src), str(dst)] + [str(n) for _, _, n in runs], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [tuple(int(x) for x in l.split()) for l in p.stdout.split("\n") if l.strip()]
    assert len(lines) == len(runs)
    streams = np.frombuffer(dst.read_bytes(), dtype=np.uint8)
    at = 0
    for (data, kind, n), (size, groups, packed) in zip(runs, lines):
        ref = _oracle_blocks(oracle, data)
        assert size == ref.size and np.array_equal(streams[at:at + size], ref), (kind, n)
        at += size
        if kind == "low_count":
            continue
        group, is_packed = g4in.KINDS[kind]
        if group:
            assert groups == n // 4, (kind, n, groups)
            assert packed == (groups if is_packed else 0), (kind, n, groups, packed)
        elif n < 8:
            assert groups == 0 and packed == 0, (kind, n, groups, packed)
    assert at == streams.size


def test_the_sanitized_build_is_one(programs):
    """(a build without the sanitizers' runtime would pass the test above for nothing)"""
    out = subprocess.run(["nm", programs["emul_group4_san"]], capture_output=True, text=True, check=True).stdout
    assert "__asan_init" in out and "__ubsan_handle" in out
    assert "__asan_init" not in subprocess.run(["nm", programs["emul_group4"]], capture_output=True, text=True, check=True).stdout
