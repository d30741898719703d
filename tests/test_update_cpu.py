"""CPU-side checks of stenos_hip_update_rows (include/stenos_hip.h): what one thread or wavefront of update_plan, update_apply,
update_splice_plan and update_splice does (csrc/update_codec.h) in the host emulation (tests/emul_update: plain and with the access
audit) against a Python model of the compact list, the overlaid slots, the new index and the spliced frame; refused indices;
declared, exported and bound; the refusals that need no device; loud failure without one; the build properties of
csrc/update_kernels.hip.

Every case runs in both builds.  The audited one checks every global access: reads against one arena that ENDS with the frame's last
byte (tables, encoded stream, old index, source rows, frame), writes against the tables of the planning steps, then the slots'
bytes, then [0, new total) of the output arena.  Slots and output stand between 64 guard bytes of 0xA5 and are shifted off their
alignment; after a refusal the whole output arena must still be 0xA5.  The frames are made of stored superblocks (code 6), so that
"decoding" is slicing and the test can hand the splice any new bytes it likes for the touched superblocks: the splice parses none."""
import ctypes
import os
import re
import shutil
import subprocess
from ctypes import c_char_p, c_int, c_size_t, c_uint32, c_uint64, c_void_p

import numpy as np
import pytest

from _libs import ROOT, np_ptr
from stenos_amd.api import load_library
from test_gather_cpu import model_cut, model_pieces_per_row

NAME = "stenos_hip_update_rows"
E = lambda k: (1 << 64) - k  # noqa: E731
NO_SLOT = 0xFFFFFFFF
W_STATUS, W_K, W_LAST, W_TOTAL = 0, 1, 2, 4
ST_TRUNCATED, ST_INVALID, ST_HOST_CODES = 1, 2, 4
PIECE = np.dtype([("lo", "<u4"), ("hi", "<u4"), ("dst", "<u8")])
MIS = [(0, 0), (1, 5), (15, 3), (7, 15)]


def _load(name):
    d = os.path.join(ROOT, "tests", "emul_update")
    subprocess.check_call(["make", "-C", d], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    lib = ctypes.CDLL(os.path.join(d, name))
    vp, u32, sz = c_void_p, c_uint32, c_size_t
    lib.emul_update_plan_apply.restype = sz
    lib.emul_update_plan_apply.argtypes = [vp, sz, vp, u32, u32, c_uint64, u32, vp, vp, sz, vp, sz, vp, c_int, c_int, vp, vp, vp, vp, vp, vp]
    lib.emul_update_splice.restype = sz
    lib.emul_update_splice.argtypes = [vp, sz, vp, u32, u32, vp, vp, sz, vp, u32, sz, c_int, c_int, vp, vp, vp, vp]
    lib.emul_audit_first_name.restype = c_char_p
    lib.emul_update_audited.restype = c_int
    return lib


@pytest.fixture(scope="module")
def builds():
    plain, audit = _load("libstenos_emul_update.so"), _load("libstenos_emul_update_audit.so")
    assert plain.emul_update_audited() == 0 and audit.emul_update_audited() == 1
    return plain, audit


def _clean(lib, rep, what):
    off = int(rep[3]) - (1 << 64) if int(rep[3]) >> 63 else int(rep[3])
    assert rep[0] == 0, (f"{what}: {rep[0]} accesses outside their arena, first: {lib.emul_audit_first_name().decode()} kind {rep[2]} "
                         f"(1 global read, 2 global write) at arena offset {off}, {rep[4]} bytes")
    if lib.emul_update_audited():
        assert rep[1] > 0, what


# ---- the model ----------------------------------------------------------------------------------------------------------

def stored_frame(data, sb, header=8, codes=None):
    """a frame of stored superblocks: (bytes, index); codes[s] replaces the code byte of superblock s (the payload stays)"""
    total = len(data)
    nsb = -(-total // sb)
    out = bytearray([0]) + total.to_bytes(7, "little")
    if header == 12:
        out = bytearray([255]) + total.to_bytes(7, "little") + sb.to_bytes(4, "little")
    idx = []
    for s in range(nsb):
        part = data[s * sb:(s + 1) * sb]
        idx.append(len(out))
        out += bytes([(codes or {}).get(s, 6)]) + len(part).to_bytes(3, "little") + bytes(part)
    idx.append(len(out))
    return np.frombuffer(bytes(out), dtype=np.uint8).copy(), np.array(idx, dtype=np.uint64)


def grouped_pieces(rows, row_bytes, stride, total, sb, nsb, rng):
    """what gather_count / gather_scan / gather_fill leave: (ppre, the table ordered by superblock, in some order inside one)"""
    P = model_pieces_per_row(row_bytes, sb)
    per = [[] for _ in range(nsb)]
    for i, row in enumerate(rows):
        for j in range(P):
            c = model_cut(row_bytes, stride, total, sb, int(row), i, j)
            if c:
                per[c[0]].append(c[1:])
    for lst in per:
        rng.shuffle(lst)
    ppre = np.zeros(nsb + 1, dtype=np.uint32)
    ppre[1:] = np.cumsum([len(x) for x in per])
    tab = np.zeros(int(ppre[-1]), dtype=PIECE)
    k = 0
    for lst in per:
        for lo, hi, dst in lst:
            tab[k] = (lo, hi, dst)
            k += 1
    return ppre, tab, per


def plan_apply(lib, frame, idx, nsb, sb, total, header, ppre, tab, src, decoded, mis):
    slot, touched, flags = (np.zeros(nsb, dtype=np.uint32) for _ in range(3))
    words = np.zeros(16, dtype=np.uint32)
    raw = np.zeros(nsb * sb + 16, dtype=np.uint8)
    rep = np.zeros(5, dtype=np.uint64)
    r = lib.emul_update_plan_apply(np_ptr(frame), frame.size, np_ptr(idx), nsb, sb, total, header, np_ptr(ppre), np_ptr(tab) if tab.size else None, tab.size,
                                   np_ptr(src) if src.size else None, src.size, np_ptr(decoded), mis[0], mis[1], np_ptr(slot), np_ptr(touched), np_ptr(flags),
                                   np_ptr(words), np_ptr(raw), np_ptr(rep))
    assert r != E(7), "a byte outside the slots changed"
    assert r == 0
    _clean(lib, rep, "update_plan / update_apply")
    return slot, touched, flags, words, raw


def splice(lib, frame, idx, nsb, header, slot, enc, enc_off, k, out_cap, mis):
    new_idx = np.zeros(nsb + 1, dtype=np.uint64)
    words = np.zeros(16, dtype=np.uint32)
    out = np.zeros(out_cap + 16, dtype=np.uint8)
    rep = np.zeros(5, dtype=np.uint64)
    enc_off = np.ascontiguousarray(enc_off, dtype=np.uint64)
    r = lib.emul_update_splice(np_ptr(frame), frame.size, np_ptr(idx), nsb, header, np_ptr(slot), np_ptr(enc) if enc.size else None, enc.size, np_ptr(enc_off), k,
                               out_cap, mis[0], mis[1], np_ptr(new_idx), np_ptr(words), np_ptr(out), np_ptr(rep))
    assert r != E(7), "a byte of the output arena outside [0, new total) changed"
    assert r != E(3)
    _clean(lib, rep, "update_splice_plan / update_splice")
    return r, new_idx, words, out


def encode_again(raw_slots, rng, how):
    """any bytes will do for the touched superblocks: the splice does not parse them.  how: 'same', 'grow', 'shrink', 'mixed'"""
    parts = []
    for c, part in enumerate(raw_slots):
        n = len(part)
        mode = how if how != "mixed" else ("grow", "shrink", "same")[c % 3]
        m = {"same": n, "grow": n + 1 + int(rng.integers(0, 40)), "shrink": max(0, n // 3 - int(rng.integers(0, 5)))}[mode]
        body = bytes(part[:m]) + bytes(rng.integers(0, 256, max(0, m - n), dtype=np.uint8))
        parts.append(bytes([6 if m == n else 1]) + m.to_bytes(3, "little") + body)
    off = np.zeros(len(parts) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(p) for p in parts])
    return np.frombuffer(b"".join(parts), dtype=np.uint8).copy(), off, parts


def run_case(builds, rng, total, sb, row_bytes, rows, how, header=8, codes=None, turn=0, dup_sources=False):
    nsb = -(-total // sb)
    data = rng.integers(0, 256, total, dtype=np.uint8)
    frame, idx = stored_frame(data, sb, header, codes)
    stride = row_bytes + (turn % 3) * 67
    n = len(rows)
    src = np.full(max(1, (n - 1) * stride + row_bytes) if n else 0, 0xEE, dtype=np.uint8)
    for i in range(n):
        src[i * stride:i * stride + row_bytes] = rng.integers(0, 256, row_bytes, dtype=np.uint8)
    ppre, tab, per = grouped_pieces(rows, row_bytes, stride, total, sb, nsb, rng)
    # the model: the compact list, the slots, the flags
    want_touched = [s for s in range(nsb) if per[s]]
    k = len(want_touched)
    want_slot = np.full(nsb, NO_SLOT, dtype=np.uint32)
    want_slot[want_touched] = np.arange(k, dtype=np.uint32)
    updated = data.copy()
    order = {}
    for s in range(nsb):
        for lo, hi, d in per[s]:
            order.setdefault((s, lo), []).append(src[d:d + hi - lo].copy())
    results = []
    for lib in builds:
        mis = MIS[(turn + (lib is builds[1])) % len(MIS)]
        slot, touched, flags, words, raw = plan_apply(lib, frame, idx, nsb, sb, total, header, ppre, tab, src, data, mis)
        assert words[W_K] == k and np.array_equal(slot, want_slot) and touched[:k].tolist() == want_touched
        if k:
            assert words[W_LAST] == want_touched[-1]
        want_flags = [1 if per[s] and (codes or {}).get(s, 6) in (2, 3, 4, 5) else 0 for s in range(nsb)]
        assert flags.tolist() == want_flags and bool(words[W_STATUS] & ST_HOST_CODES) == any(want_flags)
        assert not words[W_STATUS] & (ST_TRUNCATED | ST_INVALID)
        # the slots: the superblock's bytes with every piece replaced by (one of) its sources, whole
        slots = []
        for c, s in enumerate(want_touched):
            dsize = min(sb, total - s * sb)
            got = raw[c * sb:c * sb + dsize]
            covered = np.zeros(dsize, dtype=bool)
            for lo, hi, _ in per[s]:
                cands = order[(s, lo)]
                assert any(np.array_equal(got[lo:hi], x) for x in cands), (s, lo, hi, "a piece is not one of its sources, whole")
                if not dup_sources:
                    assert len(cands) == 1 or all(np.array_equal(cands[0], x) for x in cands)
                covered[lo:hi] = True
            assert np.array_equal(got[~covered], data[s * sb:s * sb + dsize][~covered]), "bytes no piece covers changed"
            slots.append(got.copy())
        # the splice: any new bytes for the touched superblocks
        enc, enc_off, parts = encode_again(slots, np.random.default_rng([7, turn]), how)
        pieces_of_frame = [parts[want_slot[s]] if want_slot[s] != NO_SLOT else bytes(frame[int(idx[s]):int(idx[s + 1])]) for s in range(nsb)]
        want = bytes(frame[:header]) + b"".join(pieces_of_frame)
        want_idx = np.cumsum([header] + [len(p) for p in pieces_of_frame]).astype(np.uint64)
        r, new_idx, words2, out = splice(lib, frame, idx, nsb, header, slot, enc, enc_off, k, len(want), mis)
        assert r == len(want) and np.array_equal(new_idx, want_idx)
        assert int(words2[W_TOTAL]) | (int(words2[W_TOTAL + 1]) << 32) == len(want)
        assert bytes(out[:r]) == want
        # one byte less: refused, the whole arena untouched (checked inside: -7 otherwise)
        r2, _, _, _ = splice(lib, frame, idx, nsb, header, slot, enc, enc_off, k, len(want) - 1, mis)
        assert r2 == E(6)
        results.append((bytes(raw[:k * sb]), bytes(out[:r])))
    if not dup_sources:
        assert results[0] == results[1], "the result depends on the build"
    return k, nsb


# ---- the planning, apply and splice steps ------------------------------------------------------------------------------------

@pytest.mark.parametrize("sb", [1024, 96])
def test_plan_apply_and_splice_against_the_model(builds, sb):
    rng = np.random.default_rng([51, sb])
    seen = set()
    turn = 0
    for total in (sb, 2 * sb + 300 % sb + 7, 3 * sb + 41, 4 * sb):
        nsb = -(-total // sb)
        for row_bytes in (1, 7, sb // 4, sb, sb + 5):
            nrows = total // row_bytes
            if nrows == 0:
                continue
            first_sb_rows = [r for r in range(nrows) if (r + 1) * row_bytes <= sb]
            inner = [r for r in range(nrows) if sb <= r * row_bytes and (r + 1) * row_bytes <= 2 * sb]
            sets = {"none": [], "first": first_sb_rows[:1] or [0], "last": [nrows - 1], "first+last": sorted({0, nrows - 1}), "interior": inner[:3] or [0],
                    "quarter": sorted(rng.choice(nrows, max(1, nrows // 4), replace=False).tolist()), "all": list(range(nrows))}
            if row_bytes == 1:
                sets["64"], sets["65"] = list(range(3, 67)), list(range(3, 68))  # the chunk of 64 pieces and one more
            for name, rows in sets.items():
                if name in ("all", "quarter", "64", "65") and row_bytes == 1 and total > 2 * sb + 400:
                    continue
                rows = list(rows)
                rng.shuffle(rows)
                how = ("mixed", "grow", "shrink", "same")[turn % 4]
                k, n = run_case(builds, rng, total, sb, row_bytes, rows, how, header=12 if turn % 5 == 0 else 8, turn=turn)
                seen.add("nothing" if k == 0 else "everything" if k == n else "some")
                turn += 1
    assert seen == {"nothing", "everything", "some"} and turn > 80


def test_more_superblocks_than_planning_threads(builds):
    """2 500 superblocks: a thread of the one-workgroup kernels takes a run of three; touched ones at both ends of runs"""
    rng = np.random.default_rng(52)
    sb, total = 64, 2500 * 64 - 11
    rows = sorted({0, 1, 2, 3, 5, 6, 1023, 1024, 1025, 2047, 2048, 2497, 2498, 2499} | set(rng.choice(2499, 300, replace=False).tolist()))
    k, nsb = run_case(builds, rng, total, sb, 64, rows, "mixed", turn=3)
    assert nsb == 2500 and 300 <= k < nsb
    # 53-byte rows straddle; every row
    run_case(builds, rng, total, sb, 53, list(range(total // 53)), "grow", turn=4)


def test_zstd_based_codes_of_touched_superblocks_are_flagged(builds):
    rng = np.random.default_rng(53)
    sb, total = 256, 5 * 256 + 30
    # superblocks 1 and 5 touched and zstd-coded, 3 zstd-coded and untouched (no flag), 0 touched and stored
    run_case(builds, rng, total, sb, 16, [0, 17, 18, total // 16 - 1], "same", codes={1: 3, 3: 5, 5: 2}, turn=1)


def test_repeated_rows_hold_one_of_their_sources_whole(builds):
    rng = np.random.default_rng(54)
    sb, total = 1024, 3 * 1024 + 100
    for row_bytes, rows in ((100, [3, 3, 3, 10, 10, 7, 3]), (1, [5] * 70 + [6] * 70), (1500, [1, 1, 0, 1])):
        run_case(builds, rng, total, sb, row_bytes, rows, "same", turn=row_bytes, dup_sources=True)


def test_bad_indices_are_refused_with_nothing_written(builds):
    rng = np.random.default_rng(55)
    sb, total, header = 512, 4 * 512 + 9, 8
    data = rng.integers(0, 256, total, dtype=np.uint8)
    frame, idx = stored_frame(data, sb)
    nsb = 5
    slot = np.full(nsb, NO_SLOT, dtype=np.uint32)
    slot[2] = 0
    enc = np.frombuffer(bytes([6, 3, 0, 0, 1, 2, 3]), dtype=np.uint8).copy()
    enc_off = np.array([0, 7], dtype=np.uint64)
    for lib in builds:
        ok, new_idx, _, _ = splice(lib, frame, idx, nsb, header, slot, enc, enc_off, 1, 4 * frame.size, MIS[1])
        assert ok == frame.size - (sb + 4) + 7 and new_idx[3] - new_idx[2] == 7
        cases = []
        dec = idx.copy()
        dec[3] = dec[2] - 1  # decreasing offsets (the touched superblock's own entry: checked whether touched or not)
        cases.append((dec, E(4)))
        dec = idx.copy()
        dec[1], dec[2] = dec[2], dec[1]
        cases.append((dec, E(4)))
        short = idx.copy()
        short[1] = short[0] + 3  # a superblock under 4 bytes
        cases.append((short, E(4)))
        beyond = idx.copy()
        beyond[nsb] = frame.size + 1  # the last entry beyond the frame
        cases.append((beyond, E(2)))
        far = idx.copy()
        far[nsb] = 1 << 40
        far[nsb - 1] = (1 << 40) - 20
        cases.append((far, E(2)))  # (no superblock is that long, and the end lies beyond the frame: the latter is reported)
        huge = idx.copy()
        huge[2:] = np.uint64(1 << 63) + np.arange(nsb - 1, dtype=np.uint64) * np.uint64(8)
        cases.append((huge, E(2)))
        for bad, code in cases:
            r, _, words, _ = splice(lib, frame, bad, nsb, header, slot, enc, enc_off, 1, 4 * frame.size, MIS[2])
            assert r == code, (bad.tolist(), hex(r))
            assert words[W_STATUS] & (ST_INVALID | ST_TRUNCATED)


def test_plan_bounds_a_bad_index_entry_of_a_touched_superblock(builds):
    """update_plan reads the code byte of a touched superblock only inside the frame (the audit's read arena ends with it)"""
    rng = np.random.default_rng(56)
    sb, total = 256, 3 * 256
    data = rng.integers(0, 256, total, dtype=np.uint8)
    frame, idx = stored_frame(data, sb)
    ppre, tab, _ = grouped_pieces([0, 20, 40], 16, 16, total, sb, 3, rng)
    src = rng.integers(0, 256, 48, dtype=np.uint8)
    for at in (frame.size - 3, frame.size, frame.size + 1000, (1 << 64) - 2):
        bad = idx.copy()
        bad[1] = at
        for lib in builds:
            _, _, _, words, _ = plan_apply(lib, frame, bad, 3, sb, total, 8, ppre, tab, src, data, MIS[3])
            assert words[W_STATUS] & ST_TRUNCATED and words[W_K] == 3


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

    assert callable(Stenos.update_rows)
    # the header says what is not checked, what repeated rows give, when nothing is written, and where the call loses
    comment = text[:text.index("STENOS_EXPORT size_t " + NAME)].rsplit("/*", 1)[1]
    for phrase in ("WHAT IS CHECKED", "NOT detected", "REPEATED ROW NUMBERS", "WRITES TO d_out", "profiles/update_rate.txt", "DEVICE MEMORY", "never shrink", "stenos_hip_last_index"):
        assert phrase in comment, phrase


def _call(lib, ctx, n, T=4, row_bytes=16, stride=16, rows=0x200000, src=0x300000, out=0x100000, frame=0x1000):
    return lib.stenos_hip_update_rows(ctx, frame, T, 4096, row_bytes, n, rows, src, stride, out, 1 << 20, None, None)


def test_refusals_that_need_no_device(lib):
    """(the device pointers are made up: a call that went on would fault)"""
    ctx = lib.stenos_make_context()
    try:
        bad = E(9)  # STENOS_ERROR_INVALID_PARAMETER
        assert _call(lib, ctx, 3, row_bytes=0) == bad and _call(lib, ctx, 0, row_bytes=0) == bad
        assert _call(lib, ctx, 3, row_bytes=16, stride=15) == bad
        assert _call(lib, ctx, 3, T=0) == bad and _call(lib, ctx, 3, T=65) == bad
        assert _call(lib, ctx, 1 << 61, row_bytes=8, stride=8) == bad  # n * row_bytes
        assert _call(lib, ctx, 3, row_bytes=1 << 63, stride=1 << 63) == bad
        assert _call(lib, ctx, (1 << 40) + 1, row_bytes=1, stride=1 << 24) == bad  # (n - 1) * src_stride + row_bytes
        assert _call(lib, ctx, 2, row_bytes=16, stride=(1 << 64) - 8) == bad
        assert _call(lib, ctx, 3, rows=None) == bad and _call(lib, ctx, 3, src=None) == bad
        assert _call(lib, ctx, 3, out=None) == bad and _call(lib, ctx, 3, frame=None) == bad
        # what stenos_hip_compress_batch refuses to compress
        for level in (2, 5, 9):
            lib.stenos_set_level(ctx, level)
            assert _call(lib, ctx, 3) == bad, level
        lib.stenos_set_level(ctx, 1)
        assert _call(lib, ctx, 3, T=1, row_bytes=16) == bad  # bytesoftype 1 at level 1
        lib.stenos_set_max_nanoseconds(ctx, 1000)
        assert _call(lib, ctx, 3) == bad
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


# ---- build properties of update_kernels.hip ---------------------------------------------------------------------------------

KEYS = [f"update_decodeILj{T}E" for T in (2, 4, 8, 0)]
OTHERS = ["update_planE", "update_applyE", "update_splice_planE", "update_spliceE"]


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_update_decoder_has_no_divergent_branch():
    p = subprocess.run([os.path.join(ROOT, "tools", "divergent_branches.sh"), "update_kernels.hip"] + KEYS, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert [l for l in lines if l.startswith("== ")] == [f"== {k}" for k in KEYS], p.stdout[-1500:]
    assert [l for l in lines if not l.startswith("== ")] == [], "divergent branches:\n" + p.stdout[-1500:]


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_update_kernel_resources():
    """no scratch memory, no spilled vector register, eight waves per SIMD; and the names the budget tests of the other decoders key
    on stay unique"""
    cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-c", os.path.join(ROOT, "stenos_amd", "csrc", "update_kernels.hip"),
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
        assert hits[0]["Occupancy"] == 8, (key, hits[0])
    for name in res:
        assert ("decode_superblocksILj" not in name and "encode_superblocksILj" not in name and "decode_frames_batchILj" not in name
                and "decode_rangesILj" not in name and "gather_decodeILj" not in name), name
