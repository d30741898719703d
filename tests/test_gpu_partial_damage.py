"""stenos_hip_decompress_ranges, stenos_hip_gather_rows and stenos_hip_update_rows on frames that hold damaged superblocks
(include/stenos_hip.h, "WHAT IS CHECKED"; the CPU side: tests/test_partial_damage_cpu.py).  One frame per bytesoftype: 24 superblocks
of four blocks around payloads of four classes -- (a) intact, (b) a mutant the oracle accepts whole, (c) a mutant rejected at
block 0, (d) a mutant rejected first at a block k >= 1 -- and a last superblock of two blocks and a [254] tail, intact in one
variant of the frame and rejected only in the tail in the other.  The model keeps per superblock the number of good leading blocks
and the oracle's bytes of the longest accepted prefix (the prefix oracle of tests/test_decoder_streams_cpu.py); every expectation
comes from it:

  ranges, gather   a call fails exactly when, for some superblock, the blocks up to the highest byte asked for include a bad one;
  update           a call fails exactly when a touched superblock has a bad block anywhere, and then writes nothing.

THE RULE OF tests/test_gpu_decoder_streams.py HOLDS HERE WITHOUT EXCEPTION: a damaged payload reaches the device only after the
audited emulations have decoded it on the CPU with exactly the windows, the pieces (each alone, and a call's pieces of a superblock
in groups of up to 64) and the whole-superblock decodes the calls below ask for, at the alignment it will have in device memory,
without an access outside the wave's LDS, the payload's 16-byte hull and the destination.  An audit report ends the test on the CPU."""
import ctypes
import functools
from collections import defaultdict

import numpy as np
import pytest

import streamgen as sg
import test_decoder_streams_cpu as td
import test_gather_cpu as tg
import test_ranges_cpu as tr
from _libs import has_error, load_oracle
from stenos_amd.api import Stenos, StenosError
from test_decoder_streams_cpu import audit_decode, audit_paths, mutate, mutation_bases, oracle_decode, prefix_decode
from test_gather_cpu import gather
from test_gpu_decoder_streams import _dev
from test_gpu_gather import Slots, _rows_tensor
from test_gpu_ranges import Carved
from test_gpu_update import Out, _download
from test_ranges_cpu import DECODE_ERROR, padded, window

pytestmark = pytest.mark.gpu

E = lambda k: (1 << 64) - k  # noqa: E731
SRC_OVERFLOW, INVALID_INPUT = E(2), E(4)
DAMAGE = (SRC_OVERFLOW, INVALID_INPUT)
TS = [2, 4, 8, 3, 12, 64]  # the register variants, then the LDS-image variants
NSB, PER_CLASS = 24, 6
FRAME_OFFSETS = (0, 1, 7, 16)
AUDITED = {"windows": 0, "chunks": 0, "whole": 0}  # decodes by the audited emulations in front of the device
CALLS = {"ranges": [0, 0], "gather": [0, 0], "update": [0, 0]}  # device calls: [succeeded, failed]


def _counted(what, r):
    CALLS[what][r >= E(100)] += 1
    return r


def _cuda():
    import torch

    assert torch.cuda.is_available()
    return torch


def _code(call):
    try:
        return call()
    except StenosError as err:
        return err.code


@functools.lru_cache(maxsize=None)
def _emuls():
    wp, wa = tr._load("libstenos_emul_ranges.so"), tr._load("libstenos_emul_ranges_audit.so")
    wa.emul_audit_window_decompress.restype = ctypes.c_size_t
    wa.emul_audit_window_decompress.argtypes = wp.emul_window_decompress.argtypes + [ctypes.POINTER(ctypes.c_uint64)]
    gp, ga = tg._load("libstenos_emul_gather.so"), tg._load("libstenos_emul_gather_audit.so")
    ga.emul_audit_gather_pieces.restype = ctypes.c_size_t
    ga.emul_audit_gather_pieces.argtypes = gp.emul_gather_pieces.argtypes + [ctypes.POINTER(ctypes.c_uint64)]
    whole = td._load("libstenos_emul_audit.so")
    whole.emul_audit_block_decompress.restype = ctypes.c_size_t
    whole.emul_audit_block_decompress.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int,
                                                  ctypes.POINTER(ctypes.c_uint64)]
    for lib, fill in ((wp, 0xCD), (gp, 0xCD), (wa, 0x37), (ga, 0x37)):
        lib.emul_set_lds_fill(fill)
    for lib in (wa, ga, whole):
        lib.emul_audit_first_name.restype = ctypes.c_char_p
    return wp, wa, gp, ga, whole


def good_blocks(oracle, payload: bytes, T: int, dsize: int):
    """-> (the number of good leading blocks, or None when the oracle accepts the whole payload; the oracle's bytes of the longest
    accepted prefix).  The [254] tail counts as a block."""
    bs = 256 * T
    good, got = 0, np.zeros(0, dtype=np.uint8)
    for hi in list(range(bs, dsize + 1, bs)) + ([dsize] if dsize % bs else []):
        r, out = prefix_decode(oracle, payload, T, dsize, hi)
        if has_error(r):
            return good, got
        good, got = good + 1, out.copy()
    return None, got


class Frame:
    """one variant of the frame of a bytesoftype, with its model"""

    def __init__(self, T, payloads, classes, first_bad, accepted, foff):
        self.T, self.bs, self.sb = T, 256 * T, 4 * 256 * T
        self.tail = 2 * self.bs + 37 * T + 5
        self.total = NSB * self.sb + self.tail
        self.payloads, self.cls, self.first_bad, self.foff = payloads, classes, first_bad, foff
        self.np, self.offs = sg.frame_of_payloads(payloads, T, self.sb, self.total)
        self.full = np.zeros(self.total, dtype=np.uint8)  # the model's bytes; zeros where no decoder owes any
        for s, got in enumerate(accepted):
            self.full[s * self.sb:s * self.sb + got.size] = got
        self.padded = [padded(p) for p in payloads]

    def dsize(self, s):
        return min(self.sb, self.total - s * self.sb)

    def mis(self, s):
        """the payload's offset from a 16-byte boundary in device memory (allocations are 256-byte aligned)"""
        return (self.foff + self.offs[s] + 4) % 16

    def good_bytes(self, s):
        fb = self.first_bad[s]
        return self.dsize(s) if fb is None else fb * self.bs

    def units(self, off, n):
        """the parts of bytes [off, off + n) of the array, superblock by superblock: (s, lo, hi)"""
        out = []
        for s in range(off // self.sb, (off + n - 1) // self.sb + 1):
            b = s * self.sb
            out.append((s, max(off, b) - b, min(off + n, b + self.sb, self.total) - b))
        return out

    def unit_ok(self, s, hi):
        return self.first_bad[s] is None or (hi - 1) // self.bs < self.first_bad[s]

    def ok(self, spans):
        """the call-level model of ranges and gather over (off, n) spans of the array"""
        top = defaultdict(int)
        for off, n in spans:
            for s, lo, hi in self.units(off, n):
                top[s] = max(top[s], hi)
        return all(self.unit_ok(s, hi) for s, hi in top.items())

    def of_class(self, c):
        return [s for s in range(NSB) if self.cls[s] == c]


@functools.lru_cache(maxsize=None)
def frames_of(T):
    """-> {"tail_bad": Frame, "intact_tail": Frame}; classified by the oracle alone, then every damaged payload through the audited
    whole-superblock decoder (the path of update, and of a range that is a whole superblock)"""
    oracle = load_oracle()
    bs, sb = 256 * T, 4 * 256 * T
    tail = 2 * bs + 37 * T + 5
    rng = np.random.default_rng([41, T])
    bases = mutation_bases(oracle, T, sb)
    base_bytes = []
    for payload, dsize in bases:
        fb, got = good_blocks(oracle, payload, T, sb)
        assert dsize == sb and fb is None
        base_bytes.append(got)
    found = {"a": [], "b": [], "c": [], "d": []}
    for i in rng.permutation(len(bases))[:PER_CLASS]:
        found["a"].append((bases[int(i)][0], None, base_bytes[int(i)]))
    per_k, same, differs = defaultdict(int), 0, 0
    for i in range(6000):
        if all(len(v) == PER_CLASS for v in found.values()):
            break
        payload = bases[i % len(bases)][0]
        m = mutate(rng, payload)
        if m == payload:
            continue
        fb, got = good_blocks(oracle, m, T, sb)
        c = "b" if fb is None else "c" if fb == 0 else "d"
        if len(found[c]) == PER_CLASS:
            continue
        if c == "b":
            diff = not np.array_equal(got, base_bytes[i % len(bases)])
            if not diff and same >= PER_CLASS // 2:
                continue
            same, differs = same + (not diff), differs + diff
        if c == "d":
            if per_k[fb] >= 2 and i < 1500:  # (a spread over k = 1, 2, 3 while mutants are cheap to come by)
                continue
            per_k[fb] += 1
        found[c].append((m, fb, got))
    assert all(len(v) == PER_CLASS for v in found.values()), {c: len(v) for c, v in found.items()}
    assert differs >= 1 and all(fb >= 1 for _, fb, _ in found["d"]) and all(got.size == fb * bs for _, fb, got in found["d"])
    order = [found[c][i] + (c,) for i in range(PER_CLASS) for c in "adbc"]  # an intact superblock in front of every class (d) one
    # the last superblock: a base, and a mutant of it that the oracle rejects only in the tail
    tbases = mutation_bases(oracle, T, tail)
    tbad = None
    for i in range(6000):
        tb = tbases[i % len(tbases)]
        m = mutate(rng, tb[0])
        fb, got = good_blocks(oracle, m, T, tail)
        if fb == 2:
            tbad = (m, 2, got, "t")
            break
    assert tbad is not None and tb[1] == tail
    fb, got = good_blocks(oracle, tb[0], T, tail)
    assert fb is None and got.size == tail
    tgood = (tb[0], None, got, "a")
    k = TS.index(T)
    out = {}
    for v, (name, last) in enumerate((("tail_bad", tbad), ("intact_tail", tgood))):
        sbs = order + [last]
        out[name] = Frame(T, [x[0] for x in sbs], [x[3] for x in sbs], [x[1] for x in sbs], [x[2] for x in sbs], FRAME_OFFSETS[(k + v) % 4])
    whole = _emuls()[4]
    for fr in out.values():
        for s, c in enumerate(fr.cls):
            if c == "a":
                continue
            for regs in sorted({r for r, _ in audit_paths(T)}):
                r, got = audit_decode(whole, fr.payloads[s], T, fr.dsize(s), regs, fr.mis(s))
                if fr.first_bad[s] is None:
                    assert r == fr.dsize(s) and np.array_equal(got, fr.full[s * sb:s * sb + fr.dsize(s)]), (T, s, c, regs)
                else:
                    assert has_error(r), (T, s, c, regs, "the whole-superblock decoder accepts what the oracle rejects")
                AUDITED["whole"] += 1
    return out


# ---- the audit in front of the device ------------------------------------------------------------------------------------------

def audit_ranges(fr, ranges):
    """every unit of the call that lies in a superblock with a mutated payload, through both builds of the window decoder, at the
    misalignments of the device call (Carved puts range i at i % 16 behind a 16-byte boundary)"""
    wp, wa = _emuls()[:2]
    for i, (off, n) in enumerate(ranges):
        done = 0
        for s, lo, hi in fr.units(off, n):
            if fr.cls[s] != "a":
                r, got = window(wp, wa, fr.padded[s], len(fr.payloads[s]), fr.T, fr.dsize(s), lo, hi - lo, fr.mis(s), (i + done) % 16)
                if fr.unit_ok(s, hi):
                    assert r == hi - lo and np.array_equal(got, fr.full[s * fr.sb + lo:s * fr.sb + hi]), (fr.T, s, lo, hi, hex(r))
                else:
                    assert r == DECODE_ERROR, (fr.T, s, lo, hi, hex(r))
                AUDITED["windows"] += 1
            done += hi - lo


def audit_gather(fr, rb, rows, dmis):
    """the pieces of the call in every superblock with a mutated payload: each alone, and in groups of up to 64 in the call's order"""
    gp, ga = _emuls()[2:4]
    per_sb = defaultdict(list)
    for row in rows:
        for s, lo, hi in fr.units(row * rb, rb):
            if fr.cls[s] != "a":
                per_sb[s].append((lo, hi - lo))
    for s, pieces in per_sb.items():
        groups = [[p] for p in sorted(set(pieces))] + ([pieces[g:g + 64] for g in range(0, len(pieces), 64)] if len(pieces) > 1 else [])
        for group in groups:
            top = max(lo + n for lo, n in group)
            r, got = gather(gp, ga, fr.padded[s], len(fr.payloads[s]), fr.T, fr.dsize(s), group, fr.mis(s), dmis)
            if fr.unit_ok(s, top):
                want = np.concatenate([fr.full[s * fr.sb + lo:s * fr.sb + lo + n] for lo, n in group])
                assert r == 0 and np.array_equal(got, want), (fr.T, s, group[:4], hex(r))
            else:
                assert r == DECODE_ERROR, (fr.T, s, group[:4], hex(r))
            AUDITED["chunks"] += 1


class Device:
    """a frame in device memory at its byte offset, its index as frame_index gives it (in a tensor of the test's own: the calls
    overwrite the context's), a context"""

    def __init__(self, torch, fr, level=1):
        self.torch, self.fr = torch, fr
        self.st = Stenos(level=level)
        self.buf, self.view = _dev(torch, fr.np, fr.foff, 0xEE)
        assert self.buf.data_ptr() % 256 == 0
        self.size = fr.np.size
        assert self.st.frame_index(self.view, fr.T, self.size) == fr.offs
        self.index = torch.tensor(fr.offs, dtype=torch.int64, device="cuda")

    def idx(self, given):
        return self.index.data_ptr() if given else None

    def close(self):
        self.st.close()


def _ranges_call(dev, ranges, given, frame=None, size=None):
    c = Carved(dev.torch, ranges)
    f = dev.view if frame is None else frame
    r = _counted("ranges", _code(lambda: dev.st.decompress_ranges(f, dev.fr.T, dev.size if size is None else size, ranges, c.ptrs, dev.idx(given))))
    return r, c


def boundary_cases(fr):
    """per class (c) / (d) superblock, and the bad tail: (s, k, the first byte of block k in the array)"""
    return [(s, fr.first_bad[s], s * fr.sb + fr.first_bad[s] * fr.bs) for s in range(NSB + 1) if fr.first_bad[s] is not None]


# ---- ranges --------------------------------------------------------------------------------------------------------------------

def clean_ranges(fr, rng):
    sb, bs = fr.sb, fr.bs
    r = []
    for s in fr.of_class("d"):
        k = fr.first_bad[s]
        assert fr.cls[s - 1] == "a"
        r += [(s * sb + 3, 50), (s * sb + k * bs - 7, 7), (s * sb, k * bs), (s * sb - 100, 160), (s * sb - 1, 2), (s * sb + (k - 1) * bs, bs)]
    for s in fr.of_class("b"):
        r += [(s * sb, sb), (s * sb + bs - 5, bs + 10), (s * sb + 3 * bs + 1, bs - 1), (s * sb + sb - 1, 1)]
    for s in fr.of_class("a")[:2]:
        r += [(s * sb, sb), (s * sb + 2 * bs - 1, 2)]
    r.append((NSB * sb + 5, 2 * bs - 5))  # to the last byte of the last whole block of the last superblock
    fine = [s for s in range(NSB + 1) if fr.good_bytes(s)]
    for _ in range(60):
        s = fine[int(rng.integers(len(fine)))]
        lo = int(rng.integers(0, fr.good_bytes(s)))
        r.append((s * sb + lo, int(rng.integers(1, min(300, fr.good_bytes(s) - lo) + 1))))
    assert fr.ok(r)
    return r


@pytest.mark.parametrize("T", TS)
def test_ranges(T):
    frames = frames_of(T)
    bad, intact = frames["tail_bad"], frames["intact_tail"]
    rng = np.random.default_rng([42, T])
    clean = clean_ranges(bad, rng)
    fails, passes = [], []
    for s, k, at in boundary_cases(bad):
        fails.append([(at - 3, 4) if k else (at, 1)])  # the last byte is the first byte of block k
        if k:
            passes.append([(at - 9, 9)])  # the last byte is the last byte of block k - 1
    fails.append([(bad.total - 1, 1)])
    passes.append([(NSB * bad.sb, 2 * bad.bs)])
    assert not any(bad.ok(r) for r in fails) and all(bad.ok(r) for r in passes)
    assert len(fails) == 2 * PER_CLASS + 2 and len(passes) == PER_CLASS + 2
    for call in [clean] + fails + passes:  # in front of the device
        audit_ranges(bad, call)
    audit_ranges(intact, [(intact.total - 1, 1), (NSB * intact.sb, intact.tail)])
    print(f"T={T}: audited so far {AUDITED}")
    torch = _cuda()
    dev, dev2 = Device(torch, bad), Device(torch, intact)
    try:
        for given in (False, True):
            r, c = _ranges_call(dev, clean, given)
            assert r == sum(n for _, n in clean), (given, hex(r))
            c.check(bad.full)
            for call in fails:
                r, c = _ranges_call(dev, call, given)
                assert r in DAMAGE, (call, given, hex(r))
                assert c.guards_intact(), call
            for call in passes:
                r, c = _ranges_call(dev, call, given)
                assert r == call[0][1], (call, given, hex(r))
                c.check(bad.full)
            call = [(intact.total - 1, 1), (NSB * intact.sb, intact.tail)]  # the same tail, intact
            r, c = _ranges_call(dev2, call, given)
            assert r == 1 + intact.tail, hex(r)
            c.check(intact.full)
        print(f"T={T}: device calls so far [succeeded, failed] {CALLS}")
    finally:
        dev.close()
        dev2.close()


# ---- gather --------------------------------------------------------------------------------------------------------------------

def _row_ok(fr, rb, row):
    return fr.ok([(row * rb, rb)])


def clean_rows(fr, rb, rng):
    """at least 70 rows inside the accepted prefix of one class (d) superblock (more than one chunk of 64 for it), repeats among
    them, rows of every superblock that has accepted bytes, in a random order"""
    s = max(fr.of_class("d"), key=lambda x: fr.first_bad[x])
    lo, hi = s * fr.sb, s * fr.sb + fr.first_bad[s] * fr.bs
    inside = [row for row in range(-(-lo // rb), hi // rb)]
    assert inside and all(_row_ok(fr, rb, row) for row in inside)
    rows = [inside[int(x)] for x in rng.integers(0, len(inside), 75)]
    nrows = fr.total // rb
    while len(rows) < 75 + 120:
        row = int(rng.integers(0, nrows))
        if _row_ok(fr, rb, row):
            rows += [row, row] if len(rows) % 7 == 0 else [row]
    rows = [rows[int(x)] for x in rng.permutation(len(rows))]
    assert fr.ok([(row * rb, rb) for row in rows])
    return rows


def _gather_call(dev, rb, rows, given, frame=None):
    sl = Slots(dev.torch, len(rows), rb, rb + 64 + 3, 5)
    f, rt = dev.view if frame is None else frame, _rows_tensor(dev.torch, rows)
    r = _counted("gather", _code(lambda: dev.st.gather_rows(f, dev.fr.T, dev.size, rb, rt, sl.ptr, dev.idx(given), sl.stride)))
    return r, sl


@pytest.mark.parametrize("T", TS)
def test_gather(T):
    fr = frames_of(T)["tail_bad"]
    rng = np.random.default_rng([43, T])
    plan = []  # (row bytes, rows, the model's verdict)
    for rb in (256 * T, 100, 1):
        plan.append((rb, clean_rows(fr, rb, rng), True))
        for s, k, at in boundary_cases(fr):
            if at // rb < fr.total // rb:
                plan.append((rb, [at // rb], False))  # the row that holds the first byte of block k
            if k:
                plan.append((rb, [at // rb - 1], True))  # the last row that ends in front of it
    plan.append((1, [NSB * fr.sb + 2 * fr.bs - 1, 5], True))
    for rb, rows, ok in plan:
        assert fr.ok([(row * rb, rb) for row in rows]) == ok, (rb, rows[:4], ok)
        audit_gather(fr, rb, rows, 5)
    print(f"T={T}: audited so far {AUDITED}")
    torch = _cuda()
    dev = Device(torch, fr)
    try:
        for n, (rb, rows, ok) in enumerate(plan):
            for given in ((False, True) if len(rows) > 2 else (bool(n % 2),)):
                r, sl = _gather_call(dev, rb, rows, given)
                if ok:
                    assert r == len(rows) * rb, (rb, rows[:4], given, hex(r))
                    sl.check(fr.full, rows)  # (the whole buffer: the gaps and both ends too)
                else:  # the other slots are unspecified
                    assert r in DAMAGE, (rb, rows[:4], given, hex(r))
                    assert sl.gaps_intact(), (rb, rows[:4])
        print(f"T={T}: device calls so far [succeeded, failed] {CALLS}")
    finally:
        dev.close()


# ---- update --------------------------------------------------------------------------------------------------------------------

def _touched(fr, rb, rows):
    return sorted({s for row in rows for s, _, _ in fr.units(row * rb, rb)})


def _update_call(dev, rb, rows, src_rows, given, frame=None, cap=None):
    torch = dev.torch
    out = Out(torch, cap or dev.st.bound(dev.fr.total) + dev.size)  # (a mutant may be longer than anything an encoder writes)
    src = torch.from_numpy(np.ascontiguousarray(src_rows).reshape(-1)).cuda()
    f, rt = dev.view if frame is None else frame, _rows_tensor(torch, rows)
    r = _counted("update", _code(lambda: dev.st.update_rows(f, dev.fr.T, dev.size, rb, rt, src, out.view, dev.idx(given))))
    return r, out


def _superblock_bytes(oracle, T, part, dsize):
    """what one superblock of a frame decodes to: code 1 by the oracle's block decoder, code 6 as it stands"""
    code, csize = int(part[0]), int.from_bytes(part[1:4].tobytes(), "little")
    assert csize == part.size - 4
    if code == 6:
        assert csize == dsize
        return part[4:].copy()
    assert code == 1
    r, got = oracle_decode(oracle, part[4:].tobytes(), T, dsize)
    assert r == csize, hex(r)
    return got


def _check_updated(dev, ref, oracle, fr, rb, rows, src_rows, r, out):
    torch, T = dev.torch, fr.T
    got = out.frame(r)  # (asserts that nothing outside [d_out, d_out + r) changed)
    lp, ln = dev.st.last_index()
    assert lp and ln == NSB + 1
    new = _download(torch, lp, NSB + 2)
    assert new[0] == fr.offs[0] == 12 and new[-1] == r and np.array_equal(got[:12], fr.np[:12])
    touched = _touched(fr, rb, rows)
    want = np.zeros(fr.total, dtype=np.uint8)  # the model in the touched superblocks, zeros elsewhere
    for s in touched:
        want[s * fr.sb:s * fr.sb + fr.dsize(s)] = fr.full[s * fr.sb:s * fr.sb + fr.dsize(s)]
    col = np.arange(rb, dtype=np.int64)
    want[(np.asarray(rows, dtype=np.int64) * rb)[:, None] + col] = src_rows
    frame2 = torch.zeros(ref.bound(fr.total) + 8 * (NSB + 3), dtype=torch.uint8, device="cuda")
    size2 = ref.compress(torch.from_numpy(want).cuda(), T, frame2)
    offs2 = ref.frame_index(frame2, T, size2)
    assert len(offs2) == NSB + 2
    f2 = frame2[:size2].cpu().numpy()
    codes = set()
    for s in range(NSB + 1):
        part = got[new[s]:new[s + 1]]
        if s not in touched:  # the input's bytes, the damaged ones included
            assert np.array_equal(part, fr.np[fr.offs[s]:fr.offs[s + 1]]), (T, rb, s)
            continue
        codes.add(int(part[0]))
        assert np.array_equal(_superblock_bytes(oracle, T, part, fr.dsize(s)), want[s * fr.sb:s * fr.sb + fr.dsize(s)]), (T, rb, s)
        assert np.array_equal(part, f2[offs2[s]:offs2[s + 1]]), (T, rb, s, "not the bytes stenos_hip_compress makes of this superblock")
    return codes


@pytest.mark.parametrize("T", TS)
def test_update(oracle, T):
    frames = frames_of(T)
    bad, intact = frames["tail_bad"], frames["intact_tail"]
    rng = np.random.default_rng([44, T])
    bs, sb = bad.bs, bad.sb
    torch = _cuda()
    dev, dev2 = Device(torch, bad), Device(torch, intact)
    ref = Stenos(level=1)
    try:
        assert ref.lib.stenos_set_block_size(ref.ctx, 2) == 0
        # a touched superblock with a bad block anywhere: an error and not one byte written, even for a row of block 0 of a class
        # (d) superblock, which the gather call delivers
        sizes = (bs, 100, 1)
        for n, (s, k, at) in enumerate(boundary_cases(bad)):
            rb = sizes[n % 3]
            row = -(-(s * sb) // rb)  # the first row that begins in superblock s: in its block 0
            assert s * sb <= row * rb and (row + 1) * rb <= s * sb + bs
            clean = -(-(bad.of_class("a")[n % PER_CLASS] * sb) // rb)  # rows of an intact superblock beside it
            rows = [clean + 1, row, clean + 2]
            assert _touched(bad, rb, rows) == sorted({s, bad.of_class("a")[n % PER_CLASS]})
            assert s in _touched(bad, rb, rows) and (k == 0 or bad.ok([(row * rb, rb)]))
            r, out = _update_call(dev, rb, rows, rng.integers(0, 256, (3, rb), dtype=np.uint8), bool(n % 2))
            assert r in DAMAGE, (T, s, k, rb, hex(r))
            assert out.untouched(), (T, s, k, rb)
        # rows that touch only class (a) and (b) superblocks (and the intact tail)
        codes = set()
        for fr, d in ((bad, dev), (intact, dev2)):
            fine = [s for s in range(NSB + 1) if fr.first_bad[s] is None]
            for n, rb in enumerate(sizes):
                pick = [fine[int(x)] for x in rng.permutation(len(fine))[:5]]
                rows = []
                for s in pick:
                    first, end = -(-(s * sb) // rb), (s * sb + fr.dsize(s)) // rb
                    rows += [first + int(x) for x in rng.permutation(end - first)[:3]]
                if rb == bs:  # a whole superblock of noise: stored as it is (code 6)
                    s = fr.of_class("a")[0]
                    rows = sorted(set(rows) | set(range(4 * s, 4 * s + 4)))
                rows = sorted(set(rows))
                touched = _touched(fr, rb, rows)
                assert all(fr.first_bad[s] is None for s in touched) and 0 < len(touched) < NSB
                src_rows = rng.integers(0, 256, (len(rows), rb), dtype=np.uint8)
                r, out = _update_call(d, rb, rows, src_rows, bool(n % 2))
                assert r < E(100), (T, rb, hex(r))
                codes |= _check_updated(d, ref, oracle, fr, rb, rows, src_rows, r, out)
        assert codes == {1, 6}, codes
        print(f"T={T}: device calls so far [succeeded, failed] {CALLS}")
    finally:
        dev.close()
        dev2.close()
        ref.close()


# ---- size fields, with the index given: no walk repairs anything ---------------------------------------------------------------

@pytest.mark.parametrize("T", TS)
def test_size_fields(oracle, T):
    """csize of an intact superblock set to end the payload inside each of its blocks, and to reach into the next superblock's bytes:
    the verdict and the bytes are the oracle's for that csize over the same following bytes.  A csize beyond the frame's end is
    refused in front of the decoder by all three calls (range_decode_kernels.hip, gather_kernels.hip, decode_body.h:
    `a.size - p - 4 < csize`)."""
    fr = frames_of(T)["intact_tail"]
    bs, sb = fr.bs, fr.sb
    s = fr.of_class("a")[2]
    p = fr.offs[s] + 4
    ends = [0]
    for hi in range(bs, sb + 1, bs):  # where every block of the payload ends
        r, _ = prefix_decode(oracle, fr.payloads[s], T, sb, hi)
        assert not has_error(r)
        ends.append(int(r))
    assert ends[-1] == len(fr.payloads[s])
    csizes = [(ends[b] + ends[b + 1]) // 2 for b in range(4)] + [len(fr.payloads[s]) + 4 + 10]
    assert p + csizes[-1] <= fr.np.size
    windows = [(b * bs + 7, 20) for b in range(4)] + [(bs - 3, 2 * bs + 6), (0, sb)]
    wp, wa, gp, ga, whole = _emuls()
    plan = []
    for csize in csizes:
        payload = fr.np[p:p + csize].tobytes()
        fb, got = good_blocks(oracle, payload, T, sb)
        assert (fb is None) == (csize > ends[-1]) and (fb is None or fb == csizes.index(csize))
        good = sb if fb is None else fb * bs
        assert np.array_equal(got, fr.full[s * sb:s * sb + good])
        buf = padded(payload)
        for lo, n in windows:
            for dmis in (0, 1):  # (the range stands alone in its call, or second)
                r, out = window(wp, wa, buf, csize, T, sb, lo, n, fr.mis(s), dmis)
                assert (r == n and np.array_equal(out, got[lo:lo + n])) if lo + n <= good else r == DECODE_ERROR, (T, csize, lo, n, hex(r))
                AUDITED["windows"] += 1
        for b in range(4):
            r, out = gather(gp, ga, buf, csize, T, sb, [(b * bs, bs)], fr.mis(s), 5)
            assert (r == 0 and np.array_equal(out, got[b * bs:(b + 1) * bs])) if (b + 1) * bs <= good else r == DECODE_ERROR, (T, csize, b, hex(r))
            AUDITED["chunks"] += 1
        for regs in sorted({r for r, _ in audit_paths(T)}):
            r, out = audit_decode(whole, payload, T, sb, regs, fr.mis(s))
            assert has_error(r) == (fb is not None), (T, csize, regs)
            AUDITED["whole"] += 1
        plan.append((csize, good))
    print(f"T={T}: audited so far {AUDITED}")
    torch = _cuda()
    dev = Device(torch, fr)
    rng = np.random.default_rng([45, T])
    try:
        def with_csize(at, csize):
            f = dev.buf.clone()
            v = f[fr.foff:fr.foff + dev.size]
            v[at + 1:at + 4] = torch.tensor(list(csize.to_bytes(3, "little")), dtype=torch.uint8, device="cuda")
            return f, v

        for csize, good in plan:
            keep, f = with_csize(fr.offs[s], csize)
            for lo, n in windows:
                ok = lo + n <= good
                for call in ([(s * sb + lo, n)], [((s - 4) * sb + 5, 10), (s * sb + lo, n)]):  # alone, and beside a range of an intact superblock
                    r, c = _ranges_call(dev, call, True, frame=f)
                    if ok:
                        assert r == sum(x for _, x in call), (T, csize, lo, n, hex(r))
                        c.check(fr.full)
                    else:
                        assert r in DAMAGE, (T, csize, lo, n, hex(r))
                        assert c.guards_intact()
            for b in range(4):  # rows that are blocks
                ok = (b + 1) * bs <= good
                r, sl = _gather_call(dev, bs, [4 * s + b], True, frame=f)
                if ok:
                    assert r == bs, (T, csize, b, hex(r))
                    sl.check(fr.full, [4 * s + b])
                else:
                    assert r in DAMAGE, (T, csize, b, hex(r))
                    assert sl.gaps_intact()
            rows, src_rows = [4 * s + 1], rng.integers(0, 256, (1, bs), dtype=np.uint8)
            r, out = _update_call(dev, bs, rows, src_rows, True, frame=f)
            if good == sb:
                assert r < E(100), hex(r)
                got = out.frame(r)
                lp, ln = dev.st.last_index()
                new = _download(torch, lp, NSB + 2)
                want = fr.full[s * sb:(s + 1) * sb].copy()
                want[bs:2 * bs] = src_rows[0]
                assert np.array_equal(_superblock_bytes(oracle, T, got[new[s]:new[s + 1]], sb), want)
            else:
                assert r in DAMAGE, (T, csize, hex(r))
                assert out.untouched()
        # the last superblock announces one byte more than the frame holds
        keep, f = with_csize(fr.offs[NSB], len(fr.payloads[NSB]) + 1)
        r, c = _ranges_call(dev, [(NSB * sb + 3, 9)], True, frame=f)
        assert r in DAMAGE and c.untouched(), hex(r)
        r, sl = _gather_call(dev, 100, [NSB * sb // 100 + 1], True, frame=f)
        assert r in DAMAGE and sl.untouched(), hex(r)
        r, out = _update_call(dev, 100, [NSB * sb // 100 + 1], rng.integers(0, 256, (1, 100), dtype=np.uint8), True, frame=f)
        assert r in DAMAGE and out.untouched(), hex(r)
        print(f"T={T}: device calls so far [succeeded, failed] {CALLS}")
    finally:
        dev.close()
