"""CPU-side checks of stenos_hip_gather_rows (include/stenos_hip.h): the cutting function of csrc/gather_codec.h against a Python
model; decode_superblock_pieces in the host emulation (tests/emul_gather: plain and with the access audit) against slices of the
oracle's decode; the chunk rule of the gather kernels, decode_gather_chunk, in the same emulation on a frame built by hand;
declared, exported and bound; the refusals that need no device; loud failure without one; the build properties of
gather_decode (csrc/gather_kernels.hip).

Every chunk of pieces is decoded twice: by the plain build (LDS filled with 0xCD) and by the audited one (LDS filled with 0x37;
every LDS and global access checked against the wave's LDS, the read arena -- the piece table and the payload's 16-byte hull -- and
the write arena).  The write arena holds all slots with 64 guard bytes of 0xA5 between them and at both ends; both builds must give
the slices and leave every guard byte as it is.  Source misalignments 0, 1, 15 and arena misalignments 0, 1, 3, 15 take turns."""
import ctypes
import itertools
import os
import re
import shutil
import subprocess
from ctypes import c_char_p, c_int, c_size_t, c_uint64, c_void_p

import numpy as np
import pytest

import streamgen as sg
from _libs import ROOT, np_ptr
from stenos_amd.api import load_library
from test_ranges_cpu import KINDS, MISALIGN, TS, _blocks, dsizes, oracle_payload, padded, windows_of

NAME = "stenos_hip_gather_rows"
E = lambda k: (1 << 64) - k  # noqa: E731
DECODE_ERROR = E(4)
CHECKED = [0, 0]  # chunks, accesses audited


def _load(name):
    d = os.path.join(ROOT, "tests", "emul_gather")
    subprocess.check_call(["make", "-C", d], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    lib = ctypes.CDLL(os.path.join(d, name))
    U32P = ctypes.POINTER(ctypes.c_uint32)
    lib.emul_gather_pieces.restype = c_size_t
    lib.emul_gather_pieces.argtypes = [c_void_p, c_size_t, c_size_t, c_size_t, U32P, U32P, c_size_t, c_void_p, c_int, c_int]
    lib.emul_gather_chunk.restype = c_size_t
    lib.emul_gather_chunk.argtypes = [c_void_p, c_size_t, c_size_t] + [c_uint64] * 4 + [U32P, U32P, c_size_t, c_void_p, U32P, c_int, c_int]
    lib.emul_set_lds_fill.restype = None
    lib.emul_set_lds_fill.argtypes = [c_int]
    lib.emul_gather_pieces_per_row.restype = c_uint64
    lib.emul_gather_pieces_per_row.argtypes = [c_uint64, c_uint64]
    lib.emul_gather_valid_rows.restype = c_uint64
    lib.emul_gather_valid_rows.argtypes = [c_uint64, c_uint64]
    lib.emul_gather_cut.restype = c_int
    lib.emul_gather_cut.argtypes = [c_uint64] * 7 + [ctypes.POINTER(c_uint64)]
    return lib


@pytest.fixture(scope="module")
def plain():
    lib = _load("libstenos_emul_gather.so")
    lib.emul_set_lds_fill(0xCD)
    return lib


@pytest.fixture(scope="module")
def audit():
    lib = _load("libstenos_emul_gather_audit.so")
    lib.emul_audit_gather_pieces.restype = c_size_t
    lib.emul_audit_gather_pieces.argtypes = lib.emul_gather_pieces.argtypes + [ctypes.POINTER(c_uint64)]
    lib.emul_audit_gather_chunk.restype = c_size_t
    lib.emul_audit_gather_chunk.argtypes = lib.emul_gather_chunk.argtypes + [ctypes.POINTER(c_uint64)]
    lib.emul_audit_first_name.restype = c_char_p
    lib.emul_set_lds_fill(0x37)
    return lib


# ---- the cutting function ----------------------------------------------------------------------------------------------

def model_pieces_per_row(row_bytes, sb):
    """1 when no row can straddle a superblock boundary, else the most superblocks a row can touch"""
    if sb % row_bytes == 0:
        return 1
    return -(-(row_bytes - 1) // sb) + 1


def model_cut(row_bytes, stride, total, sb, row, i, j):
    """the bytes of row `row` inside superblock off // sb + j, by intersecting intervals: (superblock, lo, hi, dst) or None"""
    off = row * row_bytes
    s = off // sb + j
    a, b = max(off, s * sb), min(off + row_bytes, (s + 1) * sb, total)
    if a >= b:
        return None
    return (s, a - s * sb, b - s * sb, i * stride + (a - off))


def _totals(T, sb):
    bs = 256 * T
    return [sb, 2 * sb + 300, 2 * sb + 100, 3 * sb + (bs if sb > bs else 0) + 37 * T + 5, 2 * sb]


@pytest.mark.parametrize("T", [1, 2, 4, 12])
def test_cutting_against_the_model(plain, T):
    bs, n = 256 * T, 0
    out = (c_uint64 * 4)()
    for sb in (sg.base_superblock(T), 3 * bs):
        for row_bytes in (1, 7, bs - 1, bs, bs + 1, sb - 1, sb, sb + 1, 2 * sb + 5):
            P = plain.emul_gather_pieces_per_row(row_bytes, sb)
            assert P == model_pieces_per_row(row_bytes, sb), (row_bytes, sb)
            if row_bytes in (1, bs, sb, sb - 1, sb + 1, 2 * sb + 5):  # (bs divides sb; sb - 1 does not for sb > 2)
                assert P == {1: 1, bs: 1, sb: 1, sb - 1: 2, sb + 1: 2, 2 * sb + 5: 4}[row_bytes], (row_bytes, sb, P)
            for total in _totals(T, sb):
                nrows = plain.emul_gather_valid_rows(total, row_bytes)
                assert nrows == total // row_bytes
                if nrows == 0:
                    continue
                # first and last valid row; around every superblock boundary: the rows that straddle it or end exactly on it;
                # the rows of the last, partial superblock
                rows = {0, nrows - 1}
                for b in range(sb, total + 1, sb):
                    rows |= {r for r in ((b - 1) // row_bytes, b // row_bytes, b // row_bytes - 1, b // row_bytes + 1) if 0 <= r < nrows}
                rows |= {r for r in range(max(0, nrows - 3), nrows)}
                straddles = ends_on = 0
                for i, row in enumerate(sorted(rows)):
                    stride = row_bytes + (i % 3) * 67
                    covered = 0
                    for j in range(P):
                        want = model_cut(row_bytes, stride, total, sb, row, i, j)
                        got = plain.emul_gather_cut(row_bytes, stride, total, sb, row, i, j, out)
                        assert (tuple(out) if got else None) == want, (row_bytes, sb, total, row, j)
                        if want:
                            s, lo, hi, dst = want
                            assert lo < hi <= min(sb, total - s * sb) and dst == i * stride + covered
                            covered += hi - lo
                            n += 1
                    assert covered == row_bytes, "the pieces of a row are the row"
                    # (no piece beyond P: the row has ended)
                    assert model_cut(row_bytes, stride, total, sb, row, i, P) is None
                    off = row * row_bytes
                    straddles += off // sb != (off + row_bytes - 1) // sb
                    ends_on += (off + row_bytes) % sb == 0
                if P > 1 and total > sb:
                    assert straddles, (row_bytes, sb, total)
                if total > sb and row_bytes <= sb:
                    assert ends_on or sb % row_bytes, (row_bytes, sb, total)
    assert n > 300  # (pieces compared)


SB32 = 131072  # the default superblock of 32-bit elements: the geometry of the arrays beyond 4 GiB
LARGE_TOTALS = [(1 << 31) + a * SB32 + b for a in (-1, 1) for b in (-1, 1)] + [(1 << 32) + 5 * SB32 + 1003, (1 << 40) + 77]


@pytest.mark.parametrize("total", LARGE_TOTALS, ids=lambda t: f"total{t:#x}")
def test_cutting_against_the_model_at_large_values(plain, total):
    """The same comparison where a 32-bit temporary in gather_cut would show: arrays around 2^31 bytes, beyond 2^32 and 2^40; rows
    that end just below, start on and straddle every multiple of 2^31 (every multiple of 2^32 is one), and the last valid row; slot
    numbers and strides whose product passes 2^32 and 2^40.  Python integers are the model: nothing wraps there, and every
    expected value is asserted to fit the 64 bits (the 32 bits of lo and hi) the structure gives it."""
    sb, n = SB32, 0
    out = (c_uint64 * 4)()
    # (slot i, stride as a function of row_bytes): i * stride below 2^32, just above it, above 2^40, and the products the device
    # tests form -- three slots 2^31 + 8 apart, 2^20 + 3 slots of 4 KiB
    slots = [(0, lambda rb: rb), (1, lambda rb: (1 << 32) + rb), (2, lambda rb: (1 << 31) + 8), (3, lambda rb: (1 << 31) + 8),
             ((1 << 20) + 2, lambda rb: max(rb, 4096)), ((1 << 32) + 1, lambda rb: rb + 67), ((1 << 31) - 1, lambda rb: max(rb, 513)),
             ((1 << 40) // 4101 + 1, lambda rb: rb + 4101), (5, lambda rb: (1 << 40) + rb)]
    boundaries = list(range(1 << 31, total + 1, 1 << 31))  # (none for the two totals just below 2^31: their last rows end there)
    assert len(boundaries) == total >> 31
    passed32 = passed40 = 0
    for row_bytes in (1, 7, 4101, sb + 5):
        P = plain.emul_gather_pieces_per_row(row_bytes, sb)
        assert P == model_pieces_per_row(row_bytes, sb) == {1: 1, 7: 2, 4101: 2, sb + 5: 3}[row_bytes]
        nrows = plain.emul_gather_valid_rows(total, row_bytes)
        assert nrows == total // row_bytes and nrows * row_bytes <= total < (nrows + 1) * row_bytes
        rows = {0, nrows - 1, nrows - 2}
        for b in boundaries:
            rows |= {r for r in ((b - 1) // row_bytes - 1, (b - 1) // row_bytes, b // row_bytes, b // row_bytes + 1) if 0 <= r < nrows}
        # (the superblock boundaries next to the array's end: the last whole superblock and the partial one)
        for b in (total // sb * sb, total // sb * sb - sb):
            rows |= {r for r in ((b - 1) // row_bytes, b // row_bytes) if 0 <= r < nrows}
        straddles = 0
        for row in sorted(rows):
            for i, f in slots:
                stride = f(row_bytes)
                covered = 0
                for j in range(P + 1):
                    want = model_cut(row_bytes, stride, total, sb, row, i, j)
                    got = plain.emul_gather_cut(row_bytes, stride, total, sb, row, i, j, out)
                    assert (tuple(out) if got else None) == want, (row_bytes, total, row, i, stride, j)
                    if want:
                        s, lo, hi, dst = want
                        assert j < P and lo < hi <= min(sb, total - s * sb) and hi < (1 << 32) and s < (1 << 32) and dst < (1 << 64)
                        assert dst == i * stride + covered
                        covered += hi - lo
                        passed32 += dst >= (1 << 32)
                        passed40 += dst >= (1 << 40)
                        n += 1
                assert covered == row_bytes, "the pieces of a row are the row"
            off = row * row_bytes
            straddles += any(off < b < off + row_bytes for b in boundaries)
        # (a valid row straddles the boundary b when b is no multiple of row_bytes and the row that holds b - 1 is whole)
        assert bool(straddles) == any(b % row_bytes and (b - 1) // row_bytes < nrows for b in boundaries), (row_bytes, total)
    assert n > 100 and passed32 > 50 and passed40 > 20, (n, passed32, passed40)  # (pieces compared; destinations beyond 2^32 and 2^40)


# ---- the decoder -------------------------------------------------------------------------------------------------------

def gather(plain, audit, buf, csize, T, dsize, pieces, mis, dmis):
    """pieces: (lo, length) -> (result of the plain build, its slots' bytes back to back); the audited build must agree"""
    count = len(pieces)
    U = ctypes.c_uint32 * count
    lo, hi = U(*[p[0] for p in pieces]), U(*[p[0] + p[1] for p in pieces])
    nbytes = sum(p[1] for p in pieces)
    outs = []
    for lib in (plain, audit):
        out = np.zeros(nbytes + 16, dtype=np.uint8)
        if lib is plain:
            r = lib.emul_gather_pieces(np_ptr(buf), csize, T, dsize, lo, hi, count, np_ptr(out), mis, dmis)
        else:
            rep = (c_uint64 * 5)()
            r = lib.emul_audit_gather_pieces(np_ptr(buf), csize, T, dsize, lo, hi, count, np_ptr(out), mis, dmis, rep)
            off = rep[3] - (1 << 64) if rep[3] >> 63 else rep[3]
            assert rep[0] == 0, (f"T={T} dsize={dsize} {count} pieces mis={mis}/{dmis}: {rep[0]} accesses outside their arena, first: "
                                 f"{lib.emul_audit_first_name().decode()} kind {rep[2]} (0 LDS, 1 global read, 2 global write) at arena offset {off}, {rep[4]} bytes")
            CHECKED[1] += rep[1]
        assert r != E(7), f"T={T} dsize={dsize} {count} pieces mis={mis}/{dmis}: a byte outside the slots changed"
        assert r != E(3)
        outs.append((r, out[:nbytes].copy()))
    assert outs[0][0] == outs[1][0] and (outs[0][0] != 0 or np.array_equal(outs[0][1], outs[1][1])), (T, dsize, count, "the result depends on the LDS contents or the build")
    CHECKED[0] += 1
    return outs[0]


def chunks_of(T, dsize, rng, nrandom=12):
    """chunks of 1, 2, 63 and 64 pieces out of the windows of test_ranges_cpu.py: with duplicates; all inside block 0 (the walk
    stops early); one piece that reaches the last byte (the tail, where there is one) among pieces of block 0"""
    bs = 256 * T
    w = windows_of(T, dsize, rng, nrandom)
    pick = lambda k: [w[int(x)] for x in rng.integers(0, len(w), k)]  # noqa: E731
    first = [(lo, n) for lo, n in w if lo + n <= min(bs, dsize)] or [(0, 1)]
    in_first = lambda k: [first[int(x)] for x in rng.integers(0, len(first), k)]  # noqa: E731
    out = [[w[0]], [w[2]], pick(2), [w[1], w[1]], pick(63), pick(64), pick(31) * 2, in_first(1), in_first(2), in_first(63), in_first(64),
           in_first(62) + [(max(0, dsize - 9), min(9, dsize))], [(dsize - 1, 1)] + in_first(63)]
    out += [[x] for x in w[3:3 + nrandom]]  # single pieces: every edge of windows_of once
    out.append(w[:64])
    return out


def check_payload(plain, audit, payload, T, data, rng, turn, nrandom=12):
    buf = padded(payload)
    for pieces in chunks_of(T, data.size, rng, nrandom):
        mis, dmis = MISALIGN[next(turn) % len(MISALIGN)]
        r, got = gather(plain, audit, buf, len(payload), T, data.size, pieces, mis, dmis)
        assert r == 0, (T, data.size, pieces[:4], r)
        want = np.concatenate([data[lo:lo + n] for lo, n in pieces])
        assert np.array_equal(got, want), (T, data.size, pieces[:4], mis, dmis)


@pytest.mark.parametrize("T", TS)
def test_pieces_of_oracle_payloads(oracle, plain, audit, T):
    """payloads the oracle's block encoder writes, over the data kinds (rand: copied blocks; lzmix: mini-LZ blocks)"""
    rng = np.random.default_rng([31, T])
    turn = itertools.count(T)
    before = CHECKED[0]
    for k, kind in enumerate(KINDS):
        if kind == "rand12" and T != 4:
            continue
        for dsize in dsizes(T):
            payload, data = oracle_payload(oracle, kind, T, dsize, 40 + k)
            check_payload(plain, audit, payload, T, data, rng, turn)
    assert CHECKED[0] - before > 400


@pytest.mark.parametrize("T", TS)
def test_pieces_of_free_choice_payloads(plain, audit, T):
    """legal streams no encoder writes (tests/streamgen.py): every block kind and plane form, oversize blocks, tails"""
    rng = np.random.default_rng([32, T])
    turn = itertools.count(3 * T)
    for name, ch in sg.VARIANTS.items():
        if name.startswith("lz") and not sg.lz_width(T):
            continue
        for dsize in (4 * 256 * T + 15 * T + 7, max(1, 16 * T - 3)) if name in ("legal", "oversize", "copy", "lz") else (2 * 256 * T + 37 * T + 5,):
            data = sg.make_data(rng, T, dsize, sg.DATA_STYLE.get(name))
            payload = sg.encode_payload(data, T, ch, rng)
            check_payload(plain, audit, payload, T, data, rng, turn, nrandom=6)


@pytest.mark.parametrize("T", [2, 3, 4, 8, 12])
def test_truncated_in_front_is_an_error_and_damage_behind_is_not_seen(plain, audit, T):
    rng = np.random.default_rng([33, T])
    bs = 256 * T
    for kinds in (("planes", "planes", "planes", "planes"), ("planes", "copy", "planes", "planes"), ("copy", "copy", "copy", "copy")):
        data, enc = _blocks(T, rng, kinds)
        payload = b"".join(enc)
        buf = padded(payload)
        want = lambda ps: np.concatenate([data[lo:lo + n] for lo, n in ps])  # noqa: E731
        far = [(5, 3), (3 * bs + 11, 40)]  # block 0 and the last block: blocks 1 and 2 are parsed for nobody
        r, got = gather(plain, audit, buf, len(payload), T, data.size, far, 1, 3)
        assert r == 0 and np.array_equal(got, want(far))
        # the payload ends inside block 1, in front of the last block needed: the chain cannot be followed
        cut = len(enc[0]) + len(enc[1]) // 2
        r, _ = gather(plain, audit, buf, cut, T, data.size, far, 0, 1)
        assert r == DECODE_ERROR, (T, kinds, r)
        # ... or inside block 2, right behind a block that is stepped over
        cut = len(enc[0]) + len(enc[1]) + 1
        r, _ = gather(plain, audit, buf, cut, T, data.size, far, 15, 0)
        assert r == DECODE_ERROR, (T, kinds, r)
        # damage behind the block that holds the chunk's last byte is not looked at
        bad = buf.copy()
        start = len(enc[0]) + len(enc[1])
        bad[start:len(payload)] = 0xFF
        near = [(bs - 7, 7 + bs), (0, 1), (bs + 3, 2)]  # blocks 0 and 1, to the last byte of block 1
        r, got = gather(plain, audit, bad, len(payload), T, data.size, near, 1, 15)
        assert r == 0 and np.array_equal(got, want(near)), (T, kinds, r)
        # ... while a chunk with one piece that reaches into it sees it
        r, _ = gather(plain, audit, bad, len(payload), T, data.size, near + [(2 * bs, 1)], 0, 0)
        assert r == DECODE_ERROR, (T, kinds, r)


# ---- the chunk rule ------------------------------------------------------------------------------------------------------

TRUNCATED, INVALID, HOST_CODES = 1, 2, 4  # DECODE_STATUS_* (csrc/kernels.h)
UNTOUCHED = 0xA5A5A5A5  # the flag word as the arena is filled


def chunk(plain, audit, frame, size, T, total, sb, s, p, pieces, mis, dmis):
    """decode_gather_chunk on superblock s of frame[:size] with the index entry p -> (status, flag word, the slots' bytes) of the
    plain build; the audited build must agree, and neither may touch a byte outside the slots and the flag word"""
    count = len(pieces)
    U = ctypes.c_uint32 * count
    lo, hi = U(*[q[0] for q in pieces]), U(*[q[0] + q[1] for q in pieces])
    nbytes = sum(q[1] for q in pieces)
    outs = []
    for lib in (plain, audit):
        out = np.zeros(nbytes + 16, dtype=np.uint8)
        flag = ctypes.c_uint32(0)
        args = [np_ptr(frame), size, T, total, sb, s, p, lo, hi, count, np_ptr(out), ctypes.byref(flag), mis, dmis]
        if lib is plain:
            r = lib.emul_gather_chunk(*args)
        else:
            rep = (c_uint64 * 5)()
            r = lib.emul_audit_gather_chunk(*args, rep)
            off = rep[3] - (1 << 64) if rep[3] >> 63 else rep[3]
            assert rep[0] == 0, (f"s={s} p={p:#x} size={size} mis={mis}/{dmis}: {rep[0]} accesses outside their arena, first: "
                                 f"{lib.emul_audit_first_name().decode()} kind {rep[2]} (0 LDS, 1 global read, 2 global write) at arena offset {off}, {rep[4]} bytes")
        assert r != E(7), f"s={s} p={p:#x} size={size} mis={mis}/{dmis}: a byte outside the slots and the flag word changed"
        assert r != E(3)
        outs.append((r, flag.value, out[:nbytes].copy()))
    assert outs[0][:2] == outs[1][:2] and np.array_equal(outs[0][2], outs[1][2]), (s, p, "the result depends on the LDS contents or the build")
    return outs[0]


def test_chunk_rule_on_a_frame(oracle, plain, audit):
    """What a gather wavefront does with its superblock (csrc/gather_codec.h, decode_gather_chunk: the one copy gather_decode and
    gather_batch_decode call), on a frame of 32-bit elements with two superblocks of four blocks and a tail: the index entry and
    the header checked against the frame, the pieces against the superblock, the dispatch on the code."""
    T, sb, tail = 4, 4096, 1500
    total = 2 * sb + tail
    # superblock 0: a block stream (code 1), superblock 1: stored as it is (code 6), the tail: a block stream with a partial block
    pay0, data0 = oracle_payload(oracle, "walk", T, sb, 71)
    data1 = np.random.default_rng(72).integers(0, 256, sb, dtype=np.uint8)
    pay2, data2 = oracle_payload(oracle, "dict16", T, tail, 73)
    array = np.concatenate([data0, data1, data2])
    head = lambda code, n: bytes([code]) + n.to_bytes(3, "little")  # noqa: E731
    parts = [b"\xff" + total.to_bytes(7, "little") + sb.to_bytes(4, "little"), head(1, len(pay0)) + pay0, head(6, sb) + data1.tobytes(), head(1, len(pay2)) + pay2]
    index = list(itertools.accumulate(len(x) for x in parts))  # index[s]: the header of superblock s; index[3]: the frame's end
    size = index[3]
    frame = padded(b"".join(parts))
    turn = itertools.count(5)
    mis = lambda: MISALIGN[next(turn) % len(MISALIGN)]  # noqa: E731
    pieces = [[(0, 1), (5, 300), (1020, 2100), (sb - 1, 1), (0, sb)], [(0, sb), (17, 4000), (sb - 1, 1), (3, 1)], [(0, tail), (tail - 1, 1), (1000, 500), (7, 9)]]
    want = lambda s, ps: np.concatenate([array[s * sb + lo:s * sb + lo + n] for lo, n in ps])  # noqa: E731

    def run(s, p, ps=None, fr=frame, sz=size):
        return chunk(plain, audit, fr, sz, T, total, sb, s, p, ps or pieces[s], *mis())

    def refused(got, status, ps):  # nothing delivered, no flag set
        assert got[0] == status and got[1] == UNTOUCHED and (got[2] == 0xA5).all(), (got[0], hex(got[1]), ps[:2])

    # code 1 and code 6 delivered, the tail too
    for s in range(3):
        st, flag, got = run(s, index[s])
        assert st == 0 and flag == UNTOUCHED and np.array_equal(got, want(s, pieces[s])), (s, st, hex(flag))
    # an index entry equal to the frame size, three bytes in front of its end, and 2^63: no header is read
    for p in (size, size - 3, 1 << 63):
        refused(run(2, p), TRUNCATED, pieces[2])
    # (four bytes in front of the end a header is read: whatever stands there, its payload cannot fit or its code is refused)
    assert run(2, size - 4)[0] in (TRUNCATED, INVALID)
    # a csize that runs one byte past the frame
    refused(run(2, index[2], sz=size - 1), TRUNCATED, pieces[2])
    # code 6 with csize != dsize
    bad = frame.copy()
    bad[index[1] + 1:index[1] + 4] = np.frombuffer((sb - 1).to_bytes(3, "little"), dtype=np.uint8)
    refused(run(1, index[1], fr=bad), INVALID, pieces[1])
    # codes 2-5 are the host's: the flag word is set, nothing is delivered
    for code in (2, 3, 4, 5):
        bad = frame.copy()
        bad[index[0]] = code
        st, flag, got = run(0, index[0], fr=bad)
        assert st == HOST_CODES and flag == 1 and (got == 0xA5).all(), (code, st, hex(flag))
    # codes 0 and 7 are none
    for code in (0, 7, 255):
        bad = frame.copy()
        bad[index[1]] = code
        refused(run(1, index[1], fr=bad), INVALID, pieces[1])
    # a superblock number whose begin is at or past the array's end (3 sb > total; the largest number a table can hold)
    for s in (3, (1 << 32) - 1):
        refused(run(s, index[2], ps=pieces[2]), INVALID, pieces[2])
    # a piece with hi > dsize, among good ones; and one with lo > hi cannot be built here (its slot would be negative)
    for s, dsize in ((0, sb), (1, sb), (2, tail)):
        ps = pieces[s][:2] + [(dsize - 10, 11)]
        refused(run(s, index[s], ps=ps), INVALID, ps)


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

    assert callable(Stenos.gather_rows)
    # the header says what is not checked, that a single row is slower than the ranges call, and who serves long rows better
    comment = text[:text.index("STENOS_EXPORT size_t " + NAME)].rsplit("/*", 1)[1]
    assert "WHAT IS CHECKED" in comment and "NOT detected" in comment and "stenos_hip_decompress_ranges" in comment


def _call(lib, ctx, n, T=4, row_bytes=16, stride=16):
    return lib.stenos_hip_gather_rows(ctx, 0x1000, T, 4096, row_bytes, n, 0x200000, 0x100000, stride, None, None)


def test_no_rows_is_no_work(lib):
    ctx = lib.stenos_make_context()
    try:
        assert _call(lib, ctx, 0) == 0  # (the device pointers are made up: a call that went on would fault)
        assert _call(lib, ctx, 0, row_bytes=0) == 0
    finally:
        lib.stenos_destroy_context(ctx)


def test_refusals_that_need_no_device(lib):
    """(the device pointers are made up: a call that went on would fault)"""
    ctx = lib.stenos_make_context()
    try:
        bad = E(9)  # STENOS_ERROR_INVALID_PARAMETER
        assert _call(lib, ctx, 3, row_bytes=0) == bad
        assert _call(lib, ctx, 3, row_bytes=16, stride=15) == bad
        assert _call(lib, ctx, 3, T=0) == bad and _call(lib, ctx, 3, T=65) == bad
        assert _call(lib, ctx, 1 << 61, row_bytes=8, stride=8) == bad  # n * row_bytes
        assert _call(lib, ctx, 3, row_bytes=1 << 63, stride=1 << 63) == bad  # n * row_bytes
        assert _call(lib, ctx, (1 << 40) + 1, row_bytes=1, stride=1 << 24) == bad  # (n - 1) * dst_stride + row_bytes
        assert _call(lib, ctx, 2, row_bytes=16, stride=(1 << 64) - 8) == bad  # ... which 2^64 - 8 + 16 is too
        assert lib.stenos_hip_gather_rows(ctx, 0x1000, 4, 4096, 16, 3, None, 0x100000, 16, None, None) == bad
        assert lib.stenos_hip_gather_rows(ctx, 0x1000, 4, 4096, 16, 3, 0x200000, None, 16, None, None) == bad
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


# ---- build properties of gather_decode ----------------------------------------------------------------------------------

KEYS = [f"gather_decodeILj{T}E" for T in (2, 4, 8, 0)]


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_gather_decoder_has_no_divergent_branch():
    p = subprocess.run([os.path.join(ROOT, "tools", "divergent_branches.sh"), "gather_kernels.hip"] + KEYS, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert [l for l in lines if l.startswith("== ")] == [f"== {k}" for k in KEYS], p.stdout[-1500:]
    assert [l for l in lines if not l.startswith("== ")] == [], "divergent branches:\n" + p.stdout[-1500:]


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_gather_kernel_resources():
    """no scratch memory, no spilled vector register; and the names the budget tests of the other decoders key on stay unique"""
    cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-c", os.path.join(ROOT, "stenos_amd", "csrc", "gather_kernels.hip"),
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
        assert hits[0]["Occupancy"] == (7 if key == "gather_decodeILj4E" else 8), (key, hits[0])
    for name in res:
        assert ("decode_superblocksILj" not in name and "encode_superblocksILj" not in name and "decode_frames_batchILj" not in name
                and "decode_rangesILj" not in name), name
