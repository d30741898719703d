"""CPU-side checks of stenos_hip_gather_ranges (include/stenos_hip.h): the measuring and cutting rules of
csrc/gather_ranges_codec.h against a Python model that intersects intervals; the validity test, which forms no sum that may wrap;
the three scan passes run as block steps at a width of 4 (and 64) against numpy.cumsum, the overflow bit at exactly D[n] ==
dst_size + 1; the whole call in the host emulation (tests/emul_gather_ranges: measure -> scan -> count -> gather_scan's rule -> fill
-> decode_gather_chunk), plain and with the access audit, on a frame built by hand and on one the oracle wrote; declared, exported
and bound; no ranges is no work; loud failure without a device.

The packed output lies between 64 guard bytes of 0xA5 on both sides, behind it the superblocks' flag words and another guard.  With
the bad-range bit or the overflow bit set, the audited build is given NO region it may write: a single store of the decoder would
be counted."""
import ctypes
import itertools
import os
import re
import subprocess
from ctypes import c_char_p, c_int, c_size_t, c_uint32, c_uint64, c_void_p

import numpy as np
import pytest

import streamgen as sg
from _libs import ROOT, has_error, np_ptr, oracle_compress
from stenos_amd.api import load_library
from stenos_amd.datagen import generate
from test_ranges_cpu import MISALIGN, oracle_payload, padded, windows_of

NAME = "stenos_hip_gather_ranges"
E = lambda k: (1 << 64) - k  # noqa: E731
M64 = (1 << 64) - 1
BAD_RANGE, DST_OVERFLOW, HOST_CODES = 8, 16, 4  # DECODE_STATUS_* (csrc/kernels.h)
U64P, U32P = ctypes.POINTER(c_uint64), ctypes.POINTER(c_uint32)


def _load(name):
    d = os.path.join(ROOT, "tests", "emul_gather_ranges")
    subprocess.check_call(["make", "-C", d], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    lib = ctypes.CDLL(os.path.join(d, name))
    lib.emul_set_lds_fill.restype = None
    lib.emul_set_lds_fill.argtypes = [c_int]
    lib.emul_ranges_measure.restype = c_int
    lib.emul_ranges_measure.argtypes = [c_uint64] * 4 + [U64P]
    lib.emul_ranges_piece_bound.restype = c_uint64
    lib.emul_ranges_piece_bound.argtypes = [c_uint64] * 3
    lib.emul_ranges_cut.restype = None
    lib.emul_ranges_cut.argtypes = [c_uint64] * 5 + [U64P]
    lib.emul_ranges_offsets.restype = c_size_t
    lib.emul_ranges_offsets.argtypes = [c_uint64] * 4 + [c_void_p, c_void_p, c_uint32, c_void_p, c_void_p, U64P]
    lib.emul_gather_ranges.restype = c_size_t
    lib.emul_gather_ranges.argtypes = ([c_void_p, c_size_t, c_size_t, c_uint64, c_uint64, c_uint64, c_void_p, c_uint64, c_void_p, c_void_p, c_uint64, c_size_t, c_uint32,
                                        c_void_p, c_void_p, c_void_p, U64P, c_int, c_int])
    return lib


@pytest.fixture(scope="module")
def plain():
    lib = _load("libstenos_emul_gather_ranges.so")
    lib.emul_set_lds_fill(0xCD)
    return lib


@pytest.fixture(scope="module")
def audit():
    lib = _load("libstenos_emul_gather_ranges_audit.so")
    lib.emul_audit_gather_ranges.restype = c_size_t
    lib.emul_audit_gather_ranges.argtypes = lib.emul_gather_ranges.argtypes + [c_int, U64P]
    lib.emul_audit_first_name.restype = c_char_p
    lib.emul_set_lds_fill(0x37)
    return lib


# ---- the model -----------------------------------------------------------------------------------------------------------

def model_pieces(total, sb, off, length, d=0):
    """the intersections of [off, off + length) with the superblocks it touches, in order: (superblock, lo, hi, destination)"""
    out = []
    if length == 0:
        return out
    for s in range(off // sb, (off + length - 1) // sb + 1):
        a, b = max(off, s * sb), min(off + length, (s + 1) * sb, total)
        assert a < b
        out.append((s, a - s * sb, b - s * sb, d + (a - off)))
    return out


def model_valid(total, off, length):
    return off + length <= total  # (Python integers: nothing wraps)


def boundary_ranges(total, sb):
    """offsets and lengths on, one byte before and one byte behind every superblock boundary; length 0 at 0, in the middle and at
    the end; the whole array; ranges that end at `total` (in a partial last superblock where there is one)"""
    r = {(0, 0), (total // 2, 0), (total, 0), (0, total), (0, 1), (total - 1, 1), (max(0, total - 7), min(7, total))}
    edges = sorted({b + e for b in range(0, total + sb, sb) for e in (-1, 0, 1) if 0 <= b + e <= total})
    for a in edges:
        for b in edges:
            if a <= b and (b - a <= 2 * sb + 2):
                r.add((a, b - a))
    last = (total - 1) // sb * sb
    r |= {(last, total - last), (max(0, last - 1), total - max(0, last - 1)), (last + (total - last) // 2, total - last - (total - last) // 2)}
    return sorted(r)


# ---- the cutting rule ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T", [2, 4, 3, 64])
def test_cutting_against_the_model(plain, T):
    bs, n = 256 * T, 0
    two, four = (c_uint64 * 2)(), (c_uint64 * 4)()
    for sb in (sg.base_superblock(T), bs):  # the default size, and a custom one of a single block
        for total in (sb, 2 * sb + 300, 3 * sb + 37 * T + 5, 2 * sb):
            for i, (off, length) in enumerate(boundary_ranges(total, sb)):
                want = model_pieces(total, sb, off, length, d := (1 << 40) * (i % 3) + 1000 * i)
                assert plain.emul_ranges_measure(total, sb, off, length, two) == 1, (total, sb, off, length)
                # piece counts equal the measure rule
                rule = (off + length - 1) // sb - off // sb + 1 if length else 0
                assert (two[0], two[1]) == (length, len(want)) and len(want) == rule, (total, sb, off, length, tuple(two))
                assert rule <= (length - 1) // sb + 2 if length else rule == 0  # (what the piece bound rests on)
                covered = 0
                for j, w in enumerate(want):
                    plain.emul_ranges_cut(sb, off, length, d, j, four)
                    assert tuple(four) == w, (total, sb, off, length, j)
                    s, lo, hi, dst = w
                    assert lo < hi <= min(sb, total - s * sb) and dst == d + covered  # non-empty, inside the superblock, contiguous from D[i]
                    covered += hi - lo
                    n += 1
                assert covered == length, "the pieces of a range are the range"
    assert n > 300  # (pieces compared: the loops above did run)


def test_cutting_at_large_values(plain):
    """where a 32-bit temporary would show: an array beyond 2^40, ranges across multiples of 2^32, destinations beyond 2^40"""
    sb, total = 131072, (1 << 40) + 5 * 131072 + 1003
    two, four = (c_uint64 * 2)(), (c_uint64 * 4)()
    for off, length in (((1 << 32) - 3, 7), ((1 << 40) - 1, sb + 2), (total - 1003 - sb - 1, sb + 1004), ((1 << 33) + sb - 1, 2)):
        want = model_pieces(total, sb, off, length, d := (1 << 41) + 17)
        assert plain.emul_ranges_measure(total, sb, off, length, two) == 1 and (two[0], two[1]) == (length, len(want))
        for j, w in enumerate(want):
            plain.emul_ranges_cut(sb, off, length, d, j, four)
            assert tuple(four) == w


def test_validity_forms_no_sum_that_wraps(plain):
    two = (c_uint64 * 2)()
    total, sb = 3 * 4096 + 77, 4096
    for off, length, valid in ((M64, 2, False), (total, 1, False), (0, M64, False), (total, 0, True), (total + 1, 0, False), (M64, 0, False), (1, M64, False),
                               (total - 1, 1, True), (total - 1, 2, False), (0, total, True), (0, total + 1, False), (1 << 63, 1 << 63, False)):
        got = plain.emul_ranges_measure(total, sb, off, length, two)
        assert bool(got) == valid == model_valid(total, off, length), (off, length)
        if not valid:
            assert (two[0], two[1]) == (0, 0), "an invalid range counts as 0 bytes and 0 pieces"
    # the empty array: only length 0 at offset 0
    for off, length, valid in ((0, 0, True), (0, 1, False), (1, 0, False)):
        assert bool(plain.emul_ranges_measure(0, 1, off, length, two)) == valid


def test_piece_bound(plain):
    """2 n + floor(dst_size / sb), 0 where that passes 2^31 - 1; reached by ranges that straddle a boundary with two bytes"""
    lim = (1 << 31) - 1
    assert plain.emul_ranges_piece_bound(3, 10 * 4096 + 5, 4096) == 16
    assert plain.emul_ranges_piece_bound(1, 0, 4096) == 2
    assert plain.emul_ranges_piece_bound(lim // 2, 4096, 4096) == lim and plain.emul_ranges_piece_bound(lim // 2, 2 * 4096, 4096) == 0
    assert plain.emul_ranges_piece_bound(lim // 2 + 1, 0, 4096) == 0 and plain.emul_ranges_piece_bound(1 << 62, 0, 4096) == 0
    assert plain.emul_ranges_piece_bound(1, (lim - 2) * 4096, 4096) == lim and plain.emul_ranges_piece_bound(1, (lim - 1) * 4096, 4096) == 0
    assert plain.emul_ranges_piece_bound(1, M64, 1) == 0
    # the bound is met: n = sb / 2 - 1 ranges of sb + 2 bytes that start on the last byte of a superblock have 3 n pieces, and
    # 2 n + floor(n (sb + 2) / sb) = 2 n + n + floor(2 n / sb) = 3 n
    sb = 4096
    n = sb // 2 - 1
    assert n * 3 == plain.emul_ranges_piece_bound(n, n * (sb + 2), sb)
    assert len(model_pieces(10 * sb, sb, sb - 1, sb + 2)) == 3


# ---- the scan passes -----------------------------------------------------------------------------------------------------

def offsets_of(lib, total, sb, dst_size, offs, lens, width):
    n = len(offs)
    o, l = np.asarray(offs, dtype=np.uint64), np.asarray(lens, dtype=np.uint64)
    D, P = np.zeros(n + 1, dtype=np.uint64), np.zeros(n + 1, dtype=np.uint32)
    words = (c_uint64 * 3)()
    assert lib.emul_ranges_offsets(total, sb, dst_size, n, np_ptr(o) if n else None, np_ptr(l) if n else None, width, np_ptr(D), np_ptr(P), words) == 0
    return D, P, tuple(words)


@pytest.mark.parametrize("width", [4, 64])
@pytest.mark.parametrize("n", [0, 1, 4, 5, 16, 17, 64, 65, 1000])
def test_scan_steps_against_cumsum(plain, n, width):
    """every level boundary of the three passes is crossed at width 4: one block, one block and one range, one run per thread of
    the middle pass, runs of two, ...; lengths up to 2^31 on an array of 2^40, so the byte sums pass 2^32"""
    rng = np.random.default_rng([51, n, width])
    sb, total = 131072, (1 << 40) + 12345
    offs = [int(x) for x in rng.integers(0, total - (1 << 31), n)]
    lens = [int(x) for x in rng.integers(0, 1 << 31, n)]
    for k in range(0, n, 7):
        lens[k] = 0  # (empty ranges span nothing)
    want_D = np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.uint64), dtype=np.uint64)]).astype(np.uint64)
    pieces = [len(model_pieces(total, sb, o, l)) for o, l in zip(offs, lens)]
    want_P = np.concatenate([[0], np.cumsum(np.asarray(pieces, dtype=np.uint64))]).astype(np.uint64)
    if n >= 16:
        assert int(want_D[-1]) > 1 << 32
    total_bytes = int(want_D[-1])
    # the overflow bit: not at D[n] == dst_size, set at exactly D[n] == dst_size + 1
    for dst_size, over in ((total_bytes, False), (total_bytes + 1, False), (M64, False)) + (((total_bytes - 1, True), (0, True)) if total_bytes else ()):
        D, P, (status, npieces, tot) = offsets_of(plain, total, sb, dst_size, offs, lens, width)
        assert np.array_equal(D, want_D), (n, width, dst_size)
        assert np.array_equal(P.astype(np.uint64), want_P & np.uint64(0xFFFFFFFF)), (n, width)
        assert tot == total_bytes and npieces == int(want_P[-1]) & 0xFFFFFFFF
        assert status == (DST_OVERFLOW if over else 0), (n, width, dst_size, status)
    if n == 0:
        return
    # one invalid range in the middle: the bit, and the range counts for nothing in either sum
    k = n // 2
    for bad in ((total, 1), (M64, 2), (0, M64), (total - 5, 6)):
        o2, l2 = list(offs), list(lens)
        o2[k], l2[k] = bad
        eff = list(l2)
        eff[k] = 0
        wD = np.concatenate([[0], np.cumsum(np.asarray(eff, dtype=np.uint64), dtype=np.uint64)]).astype(np.uint64)
        D, P, (status, npieces, tot) = offsets_of(plain, total, sb, int(wD[-1]), o2, l2, width)
        assert status == BAD_RANGE and np.array_equal(D, wD) and tot == int(wD[-1]), (n, width, bad)
        # ... together with a too-small dst_size: both bits
        if int(wD[-1]):
            assert offsets_of(plain, total, sb, int(wD[-1]) - 1, o2, l2, width)[2][0] == BAD_RANGE | DST_OVERFLOW


def test_sums_of_lengths_do_not_wrap(plain):
    """lengths that pass 2^64 together: the sum stops at 2^64 - 1 and counts as beyond every dst_size"""
    total = M64
    for width in (4, 64):
        D, _, (status, _, tot) = offsets_of(plain, total, 1 << 20, M64, [0, 0, 0, 5, 0], [1 << 63, 1 << 62, 1 << 62, 5, 1], width)
        assert status == DST_OVERFLOW and tot == M64 and list(D[:3]) == [0, 1 << 63, (1 << 63) + (1 << 62)] and int(D[3]) == M64


# ---- the call in the emulation -------------------------------------------------------------------------------------------

def run_call(lib, frame, size, T, total, sb, index, ranges, dst_size, out_bytes, width, mis, dmis, audited=False, no_write=False):
    n, nsb = len(ranges), len(index) - 1
    o, l = np.asarray([r[0] for r in ranges], dtype=np.uint64), np.asarray([r[1] for r in ranges], dtype=np.uint64)
    idx = np.asarray(index, dtype=np.uint64)
    out, D, flags = np.zeros(out_bytes + 16, dtype=np.uint8), np.zeros(n + 1, dtype=np.uint64), np.zeros(nsb + 1, dtype=np.uint32)
    words = (c_uint64 * 3)()
    args = [np_ptr(frame), size, T, total, sb, nsb, np_ptr(idx), n, np_ptr(o), np_ptr(l), dst_size, out_bytes, width, np_ptr(out), np_ptr(D), np_ptr(flags), words, mis, dmis]
    rep = None
    if audited:
        rep = (c_uint64 * 5)()
        r = lib.emul_audit_gather_ranges(*args, 1 if no_write else 0, rep)
    else:
        r = lib.emul_gather_ranges(*args)
    assert r != E(7), "a byte outside the packed output and the flag words changed"
    assert r != E(3)
    return r, out[:out_bytes].copy(), D, flags[:nsb].copy(), tuple(words), rep


def _audit_clean(audit, rep, what):
    off = rep[3] - (1 << 64) if rep[3] >> 63 else rep[3]
    assert rep[0] == 0, (f"{what}: {rep[0]} accesses outside their arena, first: {audit.emul_audit_first_name().decode()} kind {rep[2]} (0 LDS, 1 global read, "
                         f"2 global write) at arena offset {off}, {rep[4]} bytes")


def check_call(plain, audit, frame, size, T, array, sb, index, ranges, turn):
    """plain and audited: the packed output equals the source slices, D the cumulative sum, every guard byte is intact"""
    total = array.size
    want = np.concatenate([array[o:o + n] for o, n in ranges] + [np.zeros(0, dtype=np.uint8)])
    want_D = np.concatenate([[0], np.cumsum(np.asarray([n for _, n in ranges], dtype=np.uint64), dtype=np.uint64)]).astype(np.uint64)
    for lib in (plain, audit):
        k = next(turn)
        mis, dmis = MISALIGN[k % len(MISALIGN)]
        r, out, D, flags, (status, npieces, tot), rep = run_call(lib, frame, size, T, total, sb, index, ranges, want.size + (k % 2) * 1000, want.size, 4 if k % 3 else 64, mis, dmis,
                                                                 audited=lib is audit)
        assert r == 0 and status == 0, (r, status, ranges[:4])
        assert tot == want.size and np.array_equal(D, want_D)
        assert npieces == sum(len(model_pieces(total, sb, o, n)) for o, n in ranges)
        assert not flags.any()
        if not np.array_equal(out, want):
            bad = int(np.flatnonzero(out != want)[0])
            i = int(np.searchsorted(want_D, bad, side="right")) - 1
            raise AssertionError(f"byte {bad} of the packed output differs (got {out[bad]}, want {want[bad]}): range {i} = {ranges[i]}")
        if rep is not None:
            _audit_clean(audit, rep, f"{len(ranges)} ranges")
            assert rep[1] > 0 or want.size == 0


def check_gated(plain, audit, frame, size, T, array, sb, index, ranges, dst_size, bits, turn):
    """an invalid range or lengths beyond dst_size: the bit is set, no piece is made, and the audited build -- given no region it
    may write -- records no store at all; the output arena is as it was"""
    total = array.size
    room = sum(n for o, n in ranges if model_valid(total, o, n))
    for lib in (plain, audit):
        mis, dmis = MISALIGN[next(turn) % len(MISALIGN)]
        r, out, _, flags, (status, _, _), rep = run_call(lib, frame, size, T, total, sb, index, ranges, dst_size, room, 4, mis, dmis, audited=lib is audit, no_write=True)
        assert r == status == bits, (r, status, bits)
        assert (out == 0xA5).all() and not flags.any()
        if rep is not None:
            _audit_clean(audit, rep, "gated call")
            assert rep[1] == 0, "the decoder ran"


def call_sets(total, sb, T, rng, inside_sb):
    """ranges out of windows_of per superblock, ranges across the boundaries, empty ones, the whole array, duplicates, a permutation;
    then 64 and 65 ranges of 7 bytes inside superblock `inside_sb` among a few others"""
    nsb = (total + sb - 1) // sb
    base = [(0, 0), (total, 0), (total // 2, 0), (0, total)]
    for s in range(nsb):
        d = min(sb, total - s * sb)
        base += [(s * sb + lo, n) for lo, n in windows_of(T, d, rng, 6)[:40]]
    for b in range(sb, total, sb):
        base += [(b - 1, 2), (b - 1, 1), (b, 1), (b - 5, min(sb + 9, total - b + 5))]
    base += [base[5], base[len(base) // 2]]
    base = [base[int(k)] for k in rng.permutation(len(base))]
    sets = [base]
    lo, hi = inside_sb * sb, min(total, (inside_sb + 1) * sb)
    for count in (64, 65):
        inside = [(int(x), 7) for x in rng.integers(lo, hi - 7, count)]
        sets.append(inside)
        sets.append([(1, 3)] + inside + [(total - 2, 2)] if inside_sb else inside + [(total - 2, 2)])
    return sets


def _hand_frame(oracle):
    """32-bit elements, two superblocks of four blocks and a tail: a block stream, a stored superblock, a block stream with a partial block"""
    T, sb, tail = 4, 4096, 1500
    total = 2 * sb + tail
    pay0, data0 = oracle_payload(oracle, "walk", T, sb, 81)
    data1 = np.random.default_rng(82).integers(0, 256, sb, dtype=np.uint8)
    pay2, data2 = oracle_payload(oracle, "dict16", T, tail, 83)
    array = np.concatenate([data0, data1, data2])
    head = lambda code, n: bytes([code]) + n.to_bytes(3, "little")  # noqa: E731
    parts = [b"\xff" + total.to_bytes(7, "little") + sb.to_bytes(4, "little"), head(1, len(pay0)) + pay0, head(6, sb) + data1.tobytes(), head(1, len(pay2)) + pay2]
    index = list(itertools.accumulate(len(x) for x in parts))
    return T, sb, array, padded(b"".join(parts)), index[3], index


def _oracle_frame(oracle):
    """three superblocks of the default size written by the oracle's level 1: 2 sb + 5000 bytes of 16-bit elements"""
    T = 2
    sb = sg.base_superblock(T)
    total = 2 * sb + 5000
    array = np.concatenate([np.ascontiguousarray(generate(k, T, (n + T - 1) // T, 90 + i)).view(np.uint8).ravel()[:n]
                            for i, (k, n) in enumerate((("walk", sb), ("dict16", sb), ("runs", 5000)))])
    size, frame = oracle_compress(oracle, array, T, 1)
    assert not has_error(size) and frame[0] != 255
    index, p = [], 8
    for _ in range(3):
        index.append(p)
        assert frame[p] in (1, 6), "level 1 writes block streams and copies"
        p += 4 + int.from_bytes(frame[p + 1:p + 4].tobytes(), "little")
    assert p == size
    return T, sb, array, padded(frame.tobytes()), size, index + [p]


@pytest.mark.parametrize("which", ["hand_built", "oracle_built"])
def test_the_call_in_the_emulation(oracle, plain, audit, which):
    T, sb, array, frame, size, index = _hand_frame(oracle) if which == "hand_built" else _oracle_frame(oracle)
    total = array.size
    rng = np.random.default_rng([52, T])
    turn = itertools.count(T)
    for inside_sb in (1, 0) if which == "hand_built" else (1,):  # (the stored superblock and a block stream; a block stream)
        for ranges in call_sets(total, sb, T, rng, inside_sb):
            check_call(plain, audit, frame, size, T, array, sb, index, ranges, turn)
    # gating: each invalid range alone in the middle of a valid set, a dst_size one byte short, both
    good = call_sets(total, sb, T, rng, inside_sb=0)[1][:20] + [(sb - 3, 10)]
    room = sum(n for _, n in good)
    for bad in ((total, 1), (M64, 2), (0, M64), (total - 1, 2)):
        ranges = good[:10] + [bad] + good[10:]
        check_gated(plain, audit, frame, size, T, array, sb, index, ranges, room, BAD_RANGE, turn)
        check_gated(plain, audit, frame, size, T, array, sb, index, ranges, room - 1, BAD_RANGE | DST_OVERFLOW, turn)
    check_gated(plain, audit, frame, size, T, array, sb, index, good, room - 1, DST_OVERFLOW, turn)
    check_gated(plain, audit, frame, size, T, array, sb, index, good, 0, DST_OVERFLOW, turn)
    check_call(plain, audit, frame, size, T, array, sb, index, good, turn)  # (dst_size == the sum: it fits)


def test_zstd_codes_are_flagged_for_the_host(oracle, plain, audit):
    """a superblock with a zstd-based code: its flag word is set and DECODE_STATUS_HOST_CODES comes back; the other superblocks' pieces arrive"""
    T, sb, array, frame, size, index = _hand_frame(oracle)
    bad = frame.copy()
    bad[index[1]] = 2
    ranges = [(5, 100), (sb + 7, 50), (2 * sb + 3, 40), (sb - 2, 4)]
    want_D = [0, 100, 150, 190, 194]
    for lib in (plain, audit):
        r, out, D, flags, (status, _, tot), rep = run_call(lib, bad, size, T, array.size, sb, index, ranges, 194, 194, 4, 1, 3, audited=lib is audit)
        assert r == status == HOST_CODES and list(flags) == [0, 1, 0] and list(D) == want_D and tot == 194
        assert np.array_equal(out[:100], array[5:105]) and np.array_equal(out[150:190], array[2 * sb + 3:2 * sb + 43]) and np.array_equal(out[190:192], array[sb - 2:sb])
        assert (out[100:150] == 0xA5).all() and (out[192:194] == 0xA5).all()  # (left to the host)
        if rep is not None:
            _audit_clean(audit, rep, "host codes")


def test_stand_alone_program_under_the_sanitizers():
    """tests/emul_gather_ranges/sanitized_main.cpp: the rules and the call as a program of its own, built with
    -fsanitize=address,undefined (host code only; nothing of it is loaded into this process)"""
    d = os.path.join(ROOT, "tests", "emul_gather_ranges")
    subprocess.check_call(["make", "-C", d, "sanitized"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    p = subprocess.run([os.path.join(d, "gather_ranges_sanitized")], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip() == "ok", (p.returncode, p.stdout[-500:], p.stderr[-2000:])


# ---- the entry point -----------------------------------------------------------------------------------------------------

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

    assert callable(Stenos.gather_ranges)
    # the header says what is not checked, what memory the context keeps, what dst_size is, and who is served by what
    comment = text[:text.index("STENOS_EXPORT size_t " + NAME)].rsplit("/*", 1)[1]
    for phrase in ("WHAT IS CHECKED", "NOT detected", "DEVICE MEMORY", "WHO IS SERVED BY WHAT", "REAL capacity", "stenos_hip_decompress_ranges", "Pmax"):
        assert phrase in comment, phrase


def _call(lib, ctx, n, T=4, dst_size=1 << 20, offsets=0x200000, lengths=0x300000, dst=0x100000):
    return lib.stenos_hip_gather_ranges(ctx, 0x1000, T, 4096, n, offsets, lengths, dst, dst_size, None, None, None)


def test_no_ranges_is_no_work(lib):
    ctx = lib.stenos_make_context()
    try:
        assert _call(lib, ctx, 0) == 0  # (the device pointers are made up: a call that went on would fault)
        assert _call(lib, ctx, 0, T=0) == 0
    finally:
        lib.stenos_destroy_context(ctx)


def test_refusals_that_need_no_device(lib):
    """(the device pointers are made up: a call that went on would fault)"""
    ctx = lib.stenos_make_context()
    try:
        bad = E(9)  # STENOS_ERROR_INVALID_PARAMETER
        assert _call(lib, ctx, 3, T=0) == bad and _call(lib, ctx, 3, T=65) == bad
        assert _call(lib, ctx, 1 << 30) == bad  # 2 n alone passes 2^31 - 1
        assert _call(lib, ctx, 3, offsets=None) == bad and _call(lib, ctx, 3, lengths=None) == bad and _call(lib, ctx, 3, dst=None) == bad
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
