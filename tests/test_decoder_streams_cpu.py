"""The decoders on streams no encoder writes, and on damaged ones (no GPU: the host emulation of the kernel source).

tests/streamgen.py writes legal block streams with free choices; the truth is the data a stream was built from.  Every
stream goes through the oracle (pins the writer), the compiled reference where it was built (pins "the reference accepts
this"), every path of the emulation (both builds, register and image path, source misalignment 0 and 7) and the access
audit (tests/emul, -DWV_AUDIT: every LDS and global access of the kernel source checked against the wave's LDS, the 16-byte
hull of the payload and the destination).  Mutants of oracle-made and writer-made payloads are decoded by the oracle and
the emulation: same verdict, same bytes, no access outside the regions.

Runtime: the mutant test is sized by STENOS_STREAM_FUZZ_SECONDS (default 20; at least 2 000 mutants whatever it says)."""
import ctypes
import os
import subprocess
import time
from ctypes import c_char_p, c_int, c_size_t, c_void_p
from dataclasses import replace

import numpy as np
import pytest

import streamgen as sg
from _libs import ROOT, STAT_COPY_BLOCKS, STAT_LZ, STAT_PARTIAL, STAT_PLANE_TYPE, STAT_ROW_HDR, frame_stats, has_error, np_ptr
from stenos_amd.datagen import generate

TS = [2, 3, 4, 5, 8, 12, 16, 33, 64]
WIDE_TS = [65, 132, 516]
FORMS = ["packed_plain", "packed_raw", "packed_rle6", "packed_rle7", "runs", "slopes", "generic", "lz256", "lz256_exact", "planes_to"]
FUZZ_SECONDS = float(os.environ.get("STENOS_STREAM_FUZZ_SECONDS", "20"))
MIN_MUTANTS = 2000


def _load(name):
    d = os.path.join(ROOT, "tests", "emul")
    subprocess.check_call(["make", "-C", d], stdout=subprocess.DEVNULL)
    lib = ctypes.CDLL(os.path.join(d, name))
    lib.emul_block_decompress.restype = c_size_t
    lib.emul_block_decompress.argtypes = [c_void_p, c_size_t, c_size_t, c_size_t, c_void_p, c_int]
    lib.emul_set_dec_regs.restype = None
    lib.emul_set_dec_regs.argtypes = [c_int]
    lib.emul_set_lds_fill.restype = None
    lib.emul_set_lds_fill.argtypes = [c_int]
    lib.emul_dec_form_count.restype = c_size_t
    lib.emul_dec_form_count.argtypes = [c_int]
    lib.emul_lz_serial_count.restype = c_size_t
    lib.emul_dec_limits.restype = None
    lib.emul_dec_limits.argtypes = [c_size_t, ctypes.POINTER(ctypes.c_uint32)]
    lib.emul_dec_layout.restype = None
    lib.emul_dec_layout.argtypes = [c_size_t, ctypes.POINTER(ctypes.c_uint32)]
    return lib


@pytest.fixture(scope="module")
def emuls():
    """the two builds of the codec (copy helpers as the decode kernels / as the encoders compile them)"""
    return {"dec": _load("libstenos_emul.so"), "enc": _load("libstenos_emul_enc.so")}


@pytest.fixture(scope="module")
def audit():
    lib = _load("libstenos_emul_audit.so")
    lib.emul_audit_block_decompress.restype = c_size_t
    lib.emul_audit_block_decompress.argtypes = [c_void_p, c_size_t, c_size_t, c_size_t, c_void_p, c_int, ctypes.POINTER(ctypes.c_uint64)]
    lib.emul_audit_first_name.restype = c_char_p
    return lib


def padded(payload: bytes, slack: int = 64) -> np.ndarray:
    """the payload inside a larger buffer: a decoder that reads a byte too far reads zeros, not another allocation"""
    buf = np.zeros(len(payload) + slack, dtype=np.uint8)
    buf[:len(payload)] = np.frombuffer(payload, dtype=np.uint8)
    return buf


def oracle_decode(oracle, payload: bytes, T: int, dsize: int):
    buf = padded(payload)
    out = np.zeros(dsize + 64, dtype=np.uint8)
    r = oracle.so_block_decompress(np_ptr(buf), len(payload), T, dsize, np_ptr(out))
    return r, out[:dsize]


def prefix_bytes(T: int, dsize: int, hi: int) -> int:
    """what a decoder asked for bytes up to hi (exclusive) of a superblock of dsize bytes must look at: the blocks up to the one
    that holds byte hi - 1, which is the whole superblock when that byte lies in the tail"""
    assert 0 < hi <= dsize
    bs = 256 * T
    last = (hi - 1) // bs
    return (last + 1) * bs if last < dsize // bs else dsize


def prefix_decode(oracle, payload: bytes, T: int, dsize: int, hi: int):
    """The verdict and the bytes a partial decoder owes for any window that ends at hi: so_block_decompress decodes the prefix's
    blocks in order, returns at the first error and never looks at payload behind them -> (result, the prefix's bytes)"""
    return oracle_decode(oracle, payload, T, prefix_bytes(T, dsize, hi))


def paths(T: int):
    """(build, register path, source misalignment)"""
    return [(b, regs, mis) for b in ("dec", "enc") for regs in ((1, 0) if T in (2, 4, 8) else (0,)) for mis in (0, 7)]


def audit_paths(T: int):
    return [(regs, mis) for regs in ((1, 0) if T in (2, 4, 8) else (0,)) for mis in (0, 7)]


def emul_decode(lib, payload: bytes, T: int, dsize: int, regs: int, mis: int):
    buf = padded(payload)
    out = np.zeros(dsize + 64, dtype=np.uint8)
    lib.emul_set_dec_regs(regs)
    r = lib.emul_block_decompress(np_ptr(buf), len(payload), T, dsize, np_ptr(out), mis)
    lib.emul_set_dec_regs(1)
    assert not out[dsize:].any()
    return r, out[:dsize]


AUDITED = [0, 0]  # decodes, accesses checked


def audit_decode(lib, payload: bytes, T: int, dsize: int, regs: int, mis: int, fill: int = 0xCD):
    """-> (result, bytes); fails on any access outside the wave's LDS, the payload's 16-byte hull or the destination"""
    buf = padded(payload)
    out = np.zeros(dsize + 64, dtype=np.uint8)
    rep = (ctypes.c_uint64 * 5)()
    lib.emul_set_dec_regs(regs)
    lib.emul_set_lds_fill(fill)
    r = lib.emul_audit_block_decompress(np_ptr(buf), len(payload), T, dsize, np_ptr(out), mis, rep)
    lib.emul_set_lds_fill(0xCD)
    lib.emul_set_dec_regs(1)
    AUDITED[0] += 1
    off = rep[3] - (1 << 64) if rep[3] >> 63 else rep[3]
    assert rep[0] == 0, (f"T={T} regs={regs} mis={mis} fill={fill:#x}: {rep[0]} accesses outside their region, first: {lib.emul_audit_first_name().decode()} "
                         f"kind {rep[2]} (0 LDS, 1 global read, 2 global write) at region offset {off}, {rep[4]} bytes")
    AUDITED[1] += rep[1]
    return r, out[:dsize]


def forms(lib):
    return np.array([lib.emul_dec_form_count(i) for i in range(len(FORMS))], dtype=np.int64)


VARIANTS, DATA_STYLE = sg.VARIANTS, sg.DATA_STYLE


def streams_for(T: int, seed: int, names=None, blocks=None, nbytes=None):
    """(name, data, payload, choices) for every variant that applies to T; nbytes: the decoded size of every one (default: one or
    two blocks and a tail of any length)"""
    rng = np.random.default_rng([seed, T])
    for name, ch in VARIANTS.items():
        if names is not None and name not in names:
            continue
        if name.startswith("lz") and not sg.lz_width(T):
            continue
        nblocks = blocks if blocks is not None else (2 if T <= 16 else 1)
        tail = int(rng.integers(0, 256 * T))
        data = sg.make_data(rng, T, nblocks * 256 * T + tail if nbytes is None else nbytes, DATA_STYLE.get(name))
        yield name, data, sg.encode_payload(data, T, ch, rng), ch


def test_writer_reaches_the_whole_format(oracle):
    """so_frame_stats over the writer's frames: all four plane types, all sixteen row headers, mini-LZ, partial and copy blocks"""
    total = np.zeros(32, dtype=np.uint64)
    nframes = 0
    for T in (2, 4, 8, 3):
        rng = np.random.default_rng([11, T])
        for ch in (sg.LEGAL, sg.OVERSIZE):
            data = sg.make_data(rng, T, 14 * 256 * T + 100 * T + 3)
            frame, offs = sg.make_frame(data, T, ch, rng, sb_bytes=4 * 256 * T, p_copy=0.2)
            out = np.zeros(data.size + 64, dtype=np.uint8)
            assert oracle.so_decompress(np_ptr(frame), T, frame.size, np_ptr(out), data.size, 1) == data.size
            assert np.array_equal(out[:data.size], data)
            total += frame_stats(oracle, frame, T)
            nframes += 1
    print(f"writer self-test: {nframes} frames, plane types {total[STAT_PLANE_TYPE:STAT_PLANE_TYPE + 4].tolist()}, "
          f"row headers {total[STAT_ROW_HDR:STAT_ROW_HDR + 16].tolist()}, lz {total[STAT_LZ]}, partial {total[STAT_PARTIAL]}, copy {total[STAT_COPY_BLOCKS]}")
    assert (total[STAT_PLANE_TYPE:STAT_PLANE_TYPE + 4] > 0).all(), total
    assert (total[STAT_ROW_HDR:STAT_ROW_HDR + 16] > 0).all(), total
    assert total[STAT_LZ] > 0 and total[STAT_PARTIAL] > 0 and total[STAT_COPY_BLOCKS] > 0
    assert total[22 + 1] > 0 and total[22 + 6] > 0  # superblock codes 1 and 6


def test_oversize_limits(emuls):
    """The decoder takes the longest block the FORMAT allows, not the longest an encoder writes, and its window can hold it."""
    lib = emuls["dec"]
    for T in list(range(2, 65)) + WIDE_TS:
        lim = (ctypes.c_uint32 * 3)()
        lay = (ctypes.c_uint32 * 5)()
        lib.emul_dec_limits(T, lim)
        lib.emul_dec_layout(T, lay)
        hs = (T + 1) // 2
        assert lim[0] == sg.max_block_bytes(T)
        assert lim[1] >= hs + T * (8 + 18 + 16 * 18) == sg.max_format_block_bytes(T)
        if sg.lz_width(T):  # a mini-LZ block of literals only: [253], the items, a flags byte per eight of them
            assert lim[1] >= 1 + 256 * T + 256 * T // sg.lz_width(T) // 8
        assert lim[2] >= 1 + hs + T * (8 + 15 + 15 * 18) + (16 * T - 1)
        wcap = lay[3]
        assert wcap >= lim[1] + 15 and wcap >= lim[2] + 15, T  # (the window starts at the 16-byte boundary below the block)


@pytest.mark.parametrize("T", TS)
def test_legal_streams_decode_to_what_they_were_built_from(oracle, emuls, audit, T, request):
    ref = None
    try:
        ref = request.getfixturevalue("ref_det")
    except pytest.skip.Exception:
        pass
    before = {b: forms(lib) for b, lib in emuls.items()}
    serial_before = emuls["dec"].emul_lz_serial_count()
    nstreams = ndec = 0
    longest = 0
    checked_before = AUDITED[1]
    for name, data, payload, ch in streams_for(T, 1):
        r, got = oracle_decode(oracle, payload, T, data.size)
        assert r == len(payload) and np.array_equal(got, data), (name, "oracle", hex(r))
        if not ch.oversize:
            full = data.size // (256 * T)
            assert len(payload) <= full * sg.max_block_bytes(T) + (280 * T + sg.header_bytes(T) + 2), name
        longest = max(longest, len(payload))
        if ref is not None:
            frame = sg.frame_of_payload(payload, T, data.size)
            out = np.zeros(data.size + 64, dtype=np.uint8)
            fbuf = padded(frame.tobytes())
            rr = ref.stenos_decompress(np_ptr(fbuf), T, frame.size, np_ptr(out), data.size)
            assert rr == data.size and np.array_equal(out[:data.size], data), (name, "reference", hex(rr))
        for b, regs, mis in paths(T):
            r, got = emul_decode(emuls[b], payload, T, data.size, regs, mis)
            assert r == data.size and np.array_equal(got, data), (name, b, regs, mis, hex(r))
            ndec += 1
        for regs, mis in audit_paths(T):
            for fill in (0x00, 0xCD, 0xFF):  # no dependence on what the LDS held
                r, got = audit_decode(audit, payload, T, data.size, regs, mis, fill)
                assert r == data.size and np.array_equal(got, data), (name, "audit", regs, mis, fill, hex(r))
        nstreams += 1
    assert AUDITED[1] - checked_before > 1000 * nstreams  # (the audit did look at the accesses)
    took = {b: dict(zip(FORMS, (forms(lib) - before[b]).tolist())) for b, lib in emuls.items()}
    print(f"T={T}: {nstreams} streams (longest {longest} bytes), {ndec} emulated decodes, {AUDITED[0]} audited decodes so far, forms {took['dec']}")
    for b in emuls:
        t = took[b]
        for f in ("packed_plain", "packed_raw", "packed_rle6", "packed_rle7", "runs", "slopes", "generic"):
            assert t[f] > 0, (b, f, t)  # (generic: the rows of the tails)
        if T in (4, 8):
            assert t["lz256"] > 0 and t["lz256_exact"] > 0 and t["planes_to"] > 0, (b, t)
        if T == 2:
            assert t["planes_to"] > 0
        if T in (12, 16, 64):
            assert t["lz256"] == 0
    if T in (12, 16, 64):
        assert emuls["dec"].emul_lz_serial_count() > serial_before
    if T in (4, 8):  # no legal stream makes lz_decode_256 give up
        assert emuls["dec"].emul_lz_serial_count() == serial_before


@pytest.mark.parametrize("T", WIDE_TS)
def test_legal_streams_of_wide_types(oracle, emuls, audit, T):
    """bytesoftype above 64 (the device keeps the scratch in global memory there) through the block decoder"""
    n = 0
    for name, data, payload, ch in streams_for(T, 2, names=("legal", "oversize", "mix6715", "lz"), blocks=1):
        r, got = oracle_decode(oracle, payload, T, data.size)
        assert r == len(payload) and np.array_equal(got, data), (name, "oracle")
        for mis in (0, 7):
            r, got = emul_decode(emuls["dec"], payload, T, data.size, 0, mis)
            assert r == data.size and np.array_equal(got, data), (name, mis, hex(r))
        r, got = audit_decode(audit, payload, T, data.size, 0, 7)
        assert r == data.size and np.array_equal(got, data), name
        n += 1
    print(f"T={T}: {n} streams")


# ---- mutants ---------------------------------------------------------------------------------------------------------

ORACLE_KINDS = ["rand", "walk", "dict16", "runs", "burst", "mixed", "lzmix", "slopes"]


def mutate(rng, payload: bytes) -> bytes:
    b = bytearray(payload)
    kind = rng.choice(5, p=[0.35, 0.3, 0.1, 0.1, 0.15])
    if kind == 0:  # overwrites
        for _ in range(int(rng.integers(1, 4))):
            b[int(rng.integers(len(b)))] = int(rng.integers(256))
    elif kind == 1:  # bit flips
        for _ in range(int(rng.integers(1, 4))):
            b[int(rng.integers(len(b)))] ^= 1 << int(rng.integers(8))
    elif kind == 2:  # deletion
        at, n = int(rng.integers(len(b))), int(rng.integers(1, 5))
        del b[at:at + n]
    elif kind == 3:  # insertion
        at = int(rng.integers(len(b) + 1))
        b[at:at] = rng.integers(0, 256, int(rng.integers(1, 5))).astype(np.uint8).tobytes()
    else:  # truncation + garbage tail
        at = int(rng.integers(1, len(b)))
        b = b[:at] + bytearray(rng.integers(0, 256, int(rng.integers(0, 40))).astype(np.uint8).tobytes())
    return bytes(b) if b else b"\x00"


def mutation_bases(oracle, T: int, dsize: int | None = None):
    """(payload, decoded size): oracle-made payloads of the fuzz kinds and writer-made ones.  dsize: every base decodes to exactly
    that many bytes (default: about 600 elements, 300 above bytesoftype 16)"""
    rng = np.random.default_rng([5, T])
    bases = []
    n = 600 if T <= 16 else 300
    for k, kind in enumerate(ORACLE_KINDS):
        data = generate(kind, T, n + 13 * k, 100 + k) if dsize is None else generate(kind, T, -(-dsize // T), 100 + k)[:dsize].copy()
        buf = np.zeros(data.nbytes * 2 + 4096, dtype=np.uint8)
        r = oracle.so_block_compress(np_ptr(data), T, data.nbytes, np_ptr(buf), buf.nbytes)
        assert not has_error(r)
        bases.append((buf[:r].tobytes(), data.nbytes))
    for name, data, payload, ch in streams_for(T, 3, names=("legal", "oversize", "mix6715", "lz", "packed+6+7", "copy"), nbytes=dsize):
        bases.append((payload, data.size))
    return bases


def test_mutants_same_verdict_same_bytes_no_stray_access(oracle, emuls, audit):
    t0 = time.time()
    bases = {T: mutation_bases(oracle, T) for T in TS}
    rng = np.random.default_rng(2024)
    per_T = {T: [0, 0] for T in TS}
    total = accepted = ndec = 0
    audited_before = AUDITED[0]
    chunk = MIN_MUTANTS
    while total < MIN_MUTANTS or time.time() - t0 < FUZZ_SECONDS:
        # the oracle alone first: the differential must not be empty on either side
        mutants = []
        for i in range(total, total + chunk):
            T = TS[i % len(TS)]
            payload, dsize = bases[T][(i // len(TS)) % len(bases[T])]
            m = mutate(rng, payload)
            r, got = oracle_decode(oracle, m, T, dsize)
            mutants.append((i, T, m, dsize, r, got.copy()))
        acc = sum(1 for m in mutants if not has_error(m[4]))
        assert acc >= 0.3 * chunk and chunk - acc >= 0.1 * chunk, (acc, chunk)
        for i, T, m, dsize, r, want in mutants:
            ok = not has_error(r)
            per_T[T][0 if ok else 1] += 1
            ps = paths(T)
            chosen = ps if i % 16 == 0 else [ps[(i // len(TS)) % len(ps)]]  # one path by the index, a sample through all of them
            for b, regs, mis in chosen:
                r2, got = emul_decode(emuls[b], m, T, dsize, regs, mis)
                ndec += 1
                if ok:
                    assert r2 == dsize and np.array_equal(got, want), (i, T, b, regs, mis, hex(r2), m.hex()[:120])
                else:
                    assert has_error(r2), (i, T, b, regs, mis, "accepted what the oracle rejects", hex(r), m.hex()[:120])
            for regs, mis in audit_paths(T):
                r3, got = audit_decode(audit, m, T, dsize, regs, mis)
                if ok:
                    assert r3 == dsize and np.array_equal(got, want), (i, T, "audit", regs, mis)
                else:
                    assert has_error(r3), (i, T, "audit", regs, mis)
        total += chunk
        accepted += acc
        chunk = 450
    for T in TS:
        assert per_T[T][0] > 0 and per_T[T][1] > 0, (T, per_T)
    assert total >= MIN_MUTANTS
    print(f"{total} mutants: the oracle accepts {accepted} ({100 * accepted / total:.0f} %), rejects {total - accepted}; {ndec} emulated decodes, "
          f"{AUDITED[0] - audited_before} audited decodes; per bytesoftype [accepted, rejected]: {per_T}; {time.time() - t0:.1f} s")


# ---- streams that aim at the bound -----------------------------------------------------------------------------------------


def zero_plane(size: int) -> bytes:
    """a NORMAL plane of `size` bytes (24 .. 296) that decodes to 256 zeros: rows of header 0 (a minimum, no payload) or header 7
    with as many literals as it takes"""
    assert 24 <= size <= 296
    extra = size - 24
    hdr, rows, nmins = [], [], 0
    for r in range(16):
        if extra == 0:
            hdr.append(0)
            nmins += 1
            continue
        n = min(extra - 1, 16)  # literals of this row: it takes 2 + n bytes instead of 1
        extra -= 1 + n
        hdr.append(7)
        rows.append(((0xFFFF << n) & 0xFFFF).to_bytes(2, "little") + bytes(n))
    nib = bytearray(8)
    for r, h in enumerate(hdr):
        nib[r >> 1] |= h << (4 * (r & 1))
    return bytes(nib) + bytes(nmins) + b"".join(rows)


def zero_blocks(T: int, total: int):
    """full blocks of zeros whose encodings add up to exactly `total` bytes -> (payload, number of blocks)"""
    hs = sg.header_bytes(T)
    nb = max(1, -(-total // (hs + 296 * T)))
    while nb * (hs + T) > total:
        nb -= 1
    assert nb >= 1 and nb * (hs + T) <= total <= nb * (hs + 296 * T), (T, total)
    extra = total - nb * (hs + T)  # over planes of one byte (SAME) each
    sizes = [1] * (nb * T)
    k = 0
    while extra:
        take = min(extra, 295)
        if 0 < extra - take < 23:
            take = extra - 23
        if take < 23:  # (only when the whole extra is below 23: not reachable with one plane)
            raise AssertionError((T, total))
        sizes[k] += take
        extra -= take
        k += 1
    out = bytearray()
    for b in range(nb):
        head = bytearray(hs)
        body = bytearray()
        for j in range(T):
            s = sizes[b * T + j]
            if s == 1:
                body += b"\x00"
            else:
                head[j >> 1] |= sg.NORMAL << (4 * (j & 1))
                body += zero_plane(s)
        out += head + body
    assert len(out) == total
    return bytes(out), nb


WORST = replace(sg.LEGAL, block_kinds=("planes",), plane_types=(sg.NORMAL_RLE,), p_same=0.0, headers=(7,), p_plane_one_header=0.0, row_rle="none",
                mins_rle="none", oversize=True)


@pytest.mark.parametrize("T", [2, 4, 8, 5, 16, 64])
def test_the_longest_block_of_the_format(oracle, emuls, audit, T):
    """Every plane NORMAL_RLE with sixteen header-7 rows of sixteen literals (hs + 314 T bytes, the case of the comment above
    max_block_reach): alone, behind a stream that puts its first byte on the last bytes the window can hold, and each cut one byte short."""
    rng = np.random.default_rng([7, T])
    hs = sg.header_bytes(T)
    lay = (ctypes.c_uint32 * 5)()
    emuls["dec"].emul_dec_layout(T, lay)
    wcap = lay[3]
    data = sg.make_data(rng, T, 256 * T, "noise")
    worst = sg.encode_payload(data, T, WORST, rng)
    assert len(worst) == sg.max_format_block_bytes(T)
    cases = [("alone", worst, data)]
    for back in (1, hs + 1, 16, 17):  # the block starts `back` bytes in front of the end of the first window fill
        for mis in (0, 7):
            front, nb = zero_blocks(T, wcap - mis - back)
            cases.append((f"window-{back}-mis{mis}", front + worst, np.concatenate([np.zeros(nb * 256 * T, dtype=np.uint8), data])))
    n = 0
    for name, payload, want in cases:
        r, got = oracle_decode(oracle, payload, T, want.size)
        assert r == len(payload) and np.array_equal(got, want), name
        for regs, mis in audit_paths(T):
            for fill in (0x00, 0x77, 0xFF):
                r, got = audit_decode(audit, payload, T, want.size, regs, mis, fill)
                assert r == want.size and np.array_equal(got, want), (name, regs, mis, fill, hex(r))
                # one byte short, and cut where only the type nibbles and one byte of the block are left: what the block then reads
                # behind its bytes is whatever the LDS held (0x00: sixteen literals a row, the longest walk; 0x77, 0xFF: other shapes)
                for cut in (len(payload) - 1, len(payload) - len(worst) + hs + 1):
                    r, _ = audit_decode(audit, payload[:cut], T, want.size, regs, mis, fill)
                    assert has_error(r), (name, regs, mis, fill, cut)
                    n += 2
        for b, regs, mis in paths(T):
            r, got = emul_decode(emuls[b], payload, T, want.size, regs, mis)
            assert r == want.size and np.array_equal(got, want), (name, b, regs, mis)
            assert has_error(emul_decode(emuls[b], payload[:-1], T, want.size, regs, mis)[0])
        assert has_error(oracle_decode(oracle, payload[:-1], T, want.size)[0])
    print(f"T={T}: {len(cases)} streams around a block of {len(worst)} bytes (an encoder's longest: {sg.max_block_bytes(T)}), window {wcap}")


@pytest.mark.parametrize("T", [4, 8, 12, 16])
def test_mini_lz_block_of_literals_only(oracle, emuls, audit, T):
    """[253] and groups of eight literals throughout (flags 0x00): 1 + 256 T + a byte per group, longer than any block an encoder
    writes; for 4 and 8 it is the longest walk of lds_lz_walk32.  Complete, one byte short, and at the end of the window."""
    rng = np.random.default_rng([9, T])
    B = sg.lz_width(T)
    data = sg.make_data(rng, T, 256 * T, "noise")
    lz = sg.encode_payload(data, T, VARIANTS["lz_literals"], rng)
    assert len(lz) == 1 + 256 * T + 256 * T // B // 8 and lz[0] == 253
    lay = (ctypes.c_uint32 * 5)()
    emuls["dec"].emul_dec_layout(T, lay)
    cases = [(lz, data)]
    for back in (1, 3, 16):
        front, nb = zero_blocks(T, lay[3] - back)
        cases.append((front + lz, np.concatenate([np.zeros(nb * 256 * T, dtype=np.uint8), data])))
    for payload, want in cases:
        r, got = oracle_decode(oracle, payload, T, want.size)
        assert r == len(payload) and np.array_equal(got, want)
        for regs, mis in audit_paths(T):
            for fill in (0x00, 0xFF):
                r, got = audit_decode(audit, payload, T, want.size, regs, mis, fill)
                assert r == want.size and np.array_equal(got, want), (regs, mis, fill, hex(r))
                for cut in (len(payload) - 1, len(payload) - len(lz) + sg.header_bytes(T) + 1):
                    assert has_error(audit_decode(audit, payload[:cut], T, want.size, regs, mis, fill)[0])
        for b, regs, mis in paths(T):
            r, got = emul_decode(emuls[b], payload, T, want.size, regs, mis)
            assert r == want.size and np.array_equal(got, want), (b, regs, mis)


def test_oracle_mini_lz_does_not_read_a_distance_behind_the_payload(oracle):
    """a [253] block whose last item is a match, cut in front of the distance: an error, whatever stands behind the payload"""
    T = 4
    rng = np.random.default_rng(3)
    data = sg.make_data(rng, T, 256 * T, "dict8")
    lz = sg.encode_payload(data, T, VARIANTS["lz_matches"], rng)
    assert lz[-9] == 0xFF  # (the last group: eight one-byte distances)
    for behind in (0x00, 0x01, 0xFF):
        buf = np.full(len(lz) + 64, behind, dtype=np.uint8)
        buf[:len(lz) - 1] = np.frombuffer(lz[:-1], dtype=np.uint8)
        out = np.zeros(256 * T, dtype=np.uint8)
        assert has_error(oracle.so_block_decompress(np_ptr(buf), len(lz) - 1, T, 256 * T, np_ptr(out)))


def test_truncated_streams_under_the_audit(oracle, audit):
    """the truncation cases of test_emulation_vs_oracle.py: every prefix is an error, and no access leaves its region"""
    n = 0
    for kind, T in (("burst", 4), ("dict16", 4), ("walk", 2), ("runs", 8), ("mixed", 3), ("lzmix", 12)):
        data = generate(kind, T, 700, 3)
        buf = np.zeros(data.nbytes * 2 + 4096, dtype=np.uint8)
        r1 = oracle.so_block_compress(np_ptr(data), T, data.nbytes, np_ptr(buf), buf.nbytes)
        payload = buf[:r1].tobytes()
        for cut in list(range(1, min(r1, 80))) + list(range(max(1, r1 - 40), r1)):
            for regs, mis in audit_paths(T):
                r, _ = audit_decode(audit, payload[:cut], T, data.nbytes, regs, mis)
                assert has_error(r), (kind, cut, regs, mis)
                n += 1
    print(f"{n} audited decodes of truncated streams")
