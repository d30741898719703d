"""Damaged streams through the partial decoders (no GPU: the host emulations of csrc/range_codec.h and csrc/gather_codec.h, plain
and with the access audit).  The mutants of tests/test_decoder_streams_cpu.py -- overwritten bytes, flipped bits, deleted and
inserted bytes, a cut with a garbage tail -- reach decode_superblock_window and decode_superblock_pieces here.

The reference is the PREFIX ORACLE (prefix_decode): a decoder asked for bytes up to `hi` owes the oracle's verdict and bytes for
the blocks up to the one that holds byte hi - 1, and nothing else -- the oracle decodes those blocks in order, returns at the
first error and never looks behind them.  For a chunk of pieces hi is the chunk's largest.  The class that tells a partial decoder
from a whole one is "prefix accepted, whole payload rejected".

window() and gather() (tests/test_ranges_cpu.py, tests/test_gather_cpu.py) run both builds and assert on their own: the builds
agree, the guard bytes are intact, the audit saw no access outside the wave's LDS, the payload's 16-byte hull and the
destination / the slots.  The shares of the verdicts are conditions on the oracle alone, asserted before any emulated decode."""
import ctypes
import itertools
import time
from ctypes import c_char_p, c_size_t, c_uint64

import numpy as np
import pytest

import test_gather_cpu as tg
import test_ranges_cpu as tr
from _libs import has_error
from test_decoder_streams_cpu import mutate, mutation_bases, oracle_decode, prefix_bytes, prefix_decode
from test_gather_cpu import chunks_of, gather
from test_ranges_cpu import DECODE_ERROR, MISALIGN, _blocks, padded, window, windows_of

TS = [2, 3, 4, 8, 12, 64]
MUTANTS_PER_T = 120
WINDOWS_PER_MUTANT, CHUNKS_PER_MUTANT = 6, 3
MIN_WINDOWS, MIN_CHUNKS = 3000, 1500


@pytest.fixture(scope="module")
def wplain():
    lib = tr._load("libstenos_emul_ranges.so")
    lib.emul_set_lds_fill(0xCD)
    return lib


@pytest.fixture(scope="module")
def waudit():
    lib = tr._load("libstenos_emul_ranges_audit.so")
    lib.emul_audit_window_decompress.restype = c_size_t
    lib.emul_audit_window_decompress.argtypes = lib.emul_window_decompress.argtypes + [ctypes.POINTER(c_uint64)]
    lib.emul_audit_first_name.restype = c_char_p
    lib.emul_set_lds_fill(0x37)
    return lib


@pytest.fixture(scope="module")
def gplain():
    lib = tg._load("libstenos_emul_gather.so")
    lib.emul_set_lds_fill(0xCD)
    return lib


@pytest.fixture(scope="module")
def gaudit():
    lib = tg._load("libstenos_emul_gather_audit.so")
    lib.emul_audit_gather_pieces.restype = c_size_t
    lib.emul_audit_gather_pieces.argtypes = lib.emul_gather_pieces.argtypes + [ctypes.POINTER(c_uint64)]
    lib.emul_audit_first_name.restype = c_char_p
    lib.emul_set_lds_fill(0x37)
    return lib


class Prefixes:
    """the prefix oracle's answers for one payload, each prefix decoded once"""

    def __init__(self, oracle, payload: bytes, T: int, dsize: int):
        self.oracle, self.payload, self.T, self.dsize = oracle, payload, T, dsize
        self.known = {}

    def upto(self, hi: int):
        """-> (accepted, the prefix's bytes)"""
        p = prefix_bytes(self.T, self.dsize, hi)
        if p not in self.known:
            r, got = prefix_decode(self.oracle, self.payload, self.T, self.dsize, hi)
            self.known[p] = (not has_error(r), got.copy())
        return self.known[p]

    def whole(self) -> bool:
        return self.upto(self.dsize)[0]


def mutants_of(oracle, T: int, rng, count: int):
    """(mutant, decoded size, its Prefixes): the bases in turn"""
    bases = mutation_bases(oracle, T)
    for i in range(count):
        payload, dsize = bases[i % len(bases)]
        m = mutate(rng, payload)
        yield m, dsize, Prefixes(oracle, m, T, dsize)


def shares(per_T, what: str, total_min: int, under_min: float | None):
    """asserts the conditions on the oracle's verdicts, prints them; per_T: T -> [cases, accepted, rejected, accepted under a rejected whole]"""
    total = sum(v[0] for v in per_T.values())
    assert total >= total_min, (what, total)
    for T, (n, acc, rej, under) in per_T.items():
        print(f"{what} T={T}: {n} cases, the prefix oracle accepts {100 * acc / n:.1f} %, rejects {100 * rej / n:.1f} %, "
              f"accepts under a rejected whole payload {100 * under / n:.1f} %")
        assert acc >= 0.3 * n and rej >= 0.1 * n, (what, T, n, acc, rej)
        assert under > 0, (what, T)
    under = sum(v[3] for v in per_T.values())
    print(f"{what}: {total} cases in all, {100 * under / total:.1f} % with an accepted prefix under a rejected whole payload")
    if under_min is not None:
        assert under >= under_min * total, (what, under, total)


def test_prefix_oracle_is_monotone(oracle):
    """the verdict does not get better with a longer prefix, and a longer accepted prefix begins with the bytes of a shorter one"""
    rng = np.random.default_rng(2027)
    n = 0
    for T in TS:
        for m, dsize, pre in mutants_of(oracle, T, rng, 40):
            his = sorted({min(dsize, b) for b in range(256 * T, dsize + 256 * T, 256 * T)})
            ok_before, bytes_before = True, np.zeros(0, dtype=np.uint8)
            for hi in his:
                ok, got = pre.upto(hi)
                assert ok_before or not ok, (T, hi, m.hex()[:80])
                if ok:
                    assert np.array_equal(got[:bytes_before.size], bytes_before), (T, hi)
                    bytes_before = got
                ok_before = ok
                n += 1
    assert n > 400


def test_window_mutants_against_the_prefix_oracle(oracle, wplain, waudit):
    t0 = time.time()
    rng = np.random.default_rng(2025)
    cases = []
    per_T = {T: [0, 0, 0, 0] for T in TS}
    for T in TS:
        for m, dsize, pre in mutants_of(oracle, T, rng, MUTANTS_PER_T):
            w = windows_of(T, dsize, rng, nrandom=10)
            for k in rng.choice(len(w), WINDOWS_PER_MUTANT, replace=False):
                lo, n = w[int(k)]
                ok, want = pre.upto(lo + n)
                c = per_T[T]
                c[0] += 1
                c[1 if ok else 2] += 1
                c[3] += ok and not pre.whole()
                cases.append((T, m, dsize, lo, n, ok, want))
    shares(per_T, "windows", MIN_WINDOWS, 0.04)  # (the oracle alone, before any emulated decode)
    before = list(tr.CHECKED)
    bufs = {}
    for i, (T, m, dsize, lo, n, ok, want) in enumerate(cases):
        mis, dmis = MISALIGN[i % len(MISALIGN)]
        buf = bufs.setdefault(id(m), padded(m))
        r, got = window(wplain, waudit, buf, len(m), T, dsize, lo, n, mis, dmis)
        if ok:
            assert r == n, (i, T, dsize, lo, n, mis, dmis, "rejected what the prefix oracle accepts", hex(r), m.hex()[:120])
            assert np.array_equal(got, want[lo:lo + n]), (i, T, dsize, lo, n, mis, dmis, m.hex()[:120])
        else:
            assert r == DECODE_ERROR, (i, T, dsize, lo, n, mis, dmis, "accepted what the prefix oracle rejects", hex(r), m.hex()[:120])
    print(f"{tr.CHECKED[0] - before[0]} windows of {len(TS) * MUTANTS_PER_T} mutants through both builds, {tr.CHECKED[1] - before[1]} audited accesses, "
          f"{time.time() - t0:.1f} s")
    assert tr.CHECKED[0] - before[0] == len(cases) and tr.CHECKED[1] - before[1] > 1000 * len(cases)


def check_chunk(gplain, gaudit, buf, csize, T, dsize, pieces, ok, want, mis, dmis, note):
    r, got = gather(gplain, gaudit, buf, csize, T, dsize, pieces, mis, dmis)
    if ok:
        assert r == 0, (note, T, dsize, pieces[:4], mis, dmis, "rejected what the prefix oracle accepts", hex(r))
        assert np.array_equal(got, np.concatenate([want[lo:lo + n] for lo, n in pieces])), (note, T, dsize, pieces[:4], mis, dmis)
    else:  # (the slots may be partly written; gather() has checked that nothing else was)
        assert r == DECODE_ERROR, (note, T, dsize, pieces[:4], mis, dmis, "accepted what the prefix oracle rejects", hex(r))


def test_piece_mutants_against_the_prefix_oracle(oracle, gplain, gaudit):
    t0 = time.time()
    rng = np.random.default_rng(2026)
    cases = []
    per_T = {T: [0, 0, 0, 0] for T in TS}
    sizes = set()
    for T in TS:
        for m, dsize, pre in mutants_of(oracle, T, rng, MUTANTS_PER_T):
            chunks = chunks_of(T, dsize, rng, nrandom=6)
            for k in rng.choice(len(chunks), CHUNKS_PER_MUTANT, replace=False):
                pieces = chunks[int(k)]
                ok, want = pre.upto(max(lo + n for lo, n in pieces))
                c = per_T[T]
                c[0] += 1
                c[1 if ok else 2] += 1
                c[3] += ok and not pre.whole()
                sizes.add(len(pieces))
                cases.append((T, m, dsize, pieces, ok, want))
    shares(per_T, "chunks", MIN_CHUNKS, None)
    assert {1, 2, 63, 64} <= sizes
    before = list(tg.CHECKED)
    for i, (T, m, dsize, pieces, ok, want) in enumerate(cases):
        mis, dmis = MISALIGN[i % len(MISALIGN)]
        check_chunk(gplain, gaudit, padded(m), len(m), T, dsize, pieces, ok, want, mis, dmis, (i, m.hex()[:120]))
    print(f"{tg.CHECKED[0] - before[0]} chunks of {len(TS) * MUTANTS_PER_T} mutants through both builds, {tg.CHECKED[1] - before[1]} audited accesses, "
          f"{time.time() - t0:.1f} s")
    assert tg.CHECKED[0] - before[0] == len(cases) and tg.CHECKED[1] - before[1] > 1000 * len(cases)


# ---- the first byte of a block that is stepped over, every value ---------------------------------------------------------------

ANCHOR_KINDS = (("planes", "copy", "planes", "planes"), ("copy",) * 4)


def anchor_cases(oracle, T: int):
    """(kinds, block whose first byte is overwritten, value, the byte's own value, payload, the oracle's verdict for the whole payload, its
    bytes, the data): the
    byte is the one the step-over test reads; 252 turns a block into a copied one of another length, so that the walk lands mid-stream"""
    rng = np.random.default_rng([14, T])
    for kinds in ANCHOR_KINDS:
        data, enc = _blocks(T, rng, kinds)
        payload = b"".join(enc)
        r, got = oracle_decode(oracle, payload, T, data.size)
        assert not has_error(r) and np.array_equal(got, data)
        for block in (1, 2):
            at = sum(len(e) for e in enc[:block])
            for value in range(256):
                bad = bytearray(payload)
                bad[at] = value
                r, got = oracle_decode(oracle, bytes(bad), T, data.size)
                yield kinds, block, value, payload[at], bytes(bad), not has_error(r), got.copy(), data


@pytest.mark.parametrize("T", TS)
def test_anchor_of_a_stepped_over_block_every_value(oracle, wplain, waudit, gplain, gaudit, T):
    """the window lies in block 3, the pieces in blocks 0 and 3: blocks 1 and 2 are parsed for nobody, and the verdict is the
    oracle's for the whole payload (the prefix up to block 3)"""
    bs = 256 * T
    lo, n = 3 * bs + 11, 40
    far = [(5, 3), (lo, n)]
    turn = itertools.count(T)
    seen = {True: 0, False: 0}
    for kinds, block, value, own, bad, ok, want, data in anchor_cases(oracle, T):
        assert prefix_bytes(T, data.size, lo + n) == data.size
        if value == own:
            assert ok and np.array_equal(want, data)
        seen[ok] += 1
        buf = padded(bad)
        mis, dmis = MISALIGN[next(turn) % len(MISALIGN)]
        r, got = window(wplain, waudit, buf, len(bad), T, data.size, lo, n, mis, dmis)
        if ok:
            assert r == n and np.array_equal(got, want[lo:lo + n]), (T, kinds, block, value, hex(r))
        else:
            assert r == DECODE_ERROR, (T, kinds, block, value, hex(r))
        check_chunk(gplain, gaudit, buf, len(bad), T, data.size, far, ok, want, mis, dmis, (kinds, block, value))
    assert seen[True] >= 4 and seen[False] >= 4, seen  # (every case has the value that leaves the stream as it was, and [254])
