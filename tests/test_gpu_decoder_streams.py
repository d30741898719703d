"""The shipped decoders on streams no encoder writes, and on damaged ones (tests/streamgen.py; the CPU side of the same streams:
tests/test_decoder_streams_cpu.py).  Expected bytes = the data a stream was built from; for a damaged stream the oracle's verdict.
A damaged stream reaches the device only after the audited emulation decoded it on every path without an access outside the
wave's LDS, the payload's 16-byte hull and the destination."""
import ctypes

import numpy as np
import pytest

import streamgen as sg
from _libs import has_error, np_ptr
from stenos_amd.api import ERR_BASE, Stenos
from test_decoder_streams_cpu import _load, audit_decode, audit_paths, mutate, mutation_bases, oracle_decode

pytestmark = pytest.mark.gpu

GUARD = 64
REG_TS, IMAGE_TS, WIDE_TS = [2, 4, 8], [3, 12, 16, 33, 64], [65, 132, 516]


def _cuda():
    import torch

    assert torch.cuda.is_available()
    return torch


def _dev(torch, arr: np.ndarray, off: int = 0, fill: int = 0):
    """arr at byte offset `off` of a device allocation of its own (GUARD bytes of `fill` behind it) -> (allocation, view)"""
    buf = torch.full((off + arr.size + GUARD,), fill, dtype=torch.uint8, device="cuda")
    if arr.size:
        buf[off:off + arr.size] = torch.from_numpy(arr).cuda()
    return buf, buf[off:off + arr.size]


def _dst(torch, n: int, off: int = 0):
    buf = torch.full((off + n + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    return buf, buf[off:off + n]


def _intact(buf, off: int, n: int) -> bool:
    h = buf.cpu().numpy()
    return bool((h[:off] == 0x5A).all() and (h[off + n:] == 0x5A).all())


def _frames_for(T: int):
    """(name, frame, header offsets, data)"""
    rng = np.random.default_rng([21, T])
    if T in REG_TS:
        nsb = 72
    elif T <= 16:
        nsb = 64
    elif T <= 64:
        nsb = 16
    else:
        nsb = 5
    out = [("many", *sg.make_mixed_frame(rng, T, nsb, 1 if T > 4 else 2, 100 * T + 5))]
    out.append(("pairs", *sg.make_mixed_frame(rng, T, 3, 2, 256 * T + 16 * T + 3, p_copy=0.0, names=("oversize", "mix6715", "unmerged", "all15", "lz_literals"))))
    if T in (2, 4):
        out.append(("long", *sg.make_mixed_frame(rng, T, 300, 1, 17 * T + 1)))  # more than 256 superblocks: the parallel header walk
    if T in REG_TS:
        out.append(("default", *sg.make_mixed_frame(rng, T, 1, 0, 5 * 256 * T + 77, p_copy=0.0, default_size=True)))
    return out


@pytest.mark.parametrize("T", REG_TS + IMAGE_TS + WIDE_TS)
def test_legal_frames_on_every_decoder(oracle, T):
    torch = _cuda()
    st = Stenos(level=1)
    try:
        frames = _frames_for(T)
        for name, frame, offs, data in frames:
            n = data.size
            # (the writer and the oracle agree on the frame)
            chk = np.zeros(n + 64, dtype=np.uint8)
            assert oracle.so_decompress(np_ptr(frame), T, frame.size, np_ptr(chk), n, 1) == n and np.array_equal(chk[:n], data), name
            # the host ABI
            host = np.full(n + GUARD, 0x5A, dtype=np.uint8)
            r = st.lib.stenos_decompress_generic(st.ctx, np_ptr(frame), T, frame.size, np_ptr(host), n)
            assert r == n, (name, "host", hex(r))
            assert np.array_equal(host[:n], data) and (host[n:] == 0x5A).all(), (name, "host")
            # the device call: frame and destination at byte offsets of their allocations, without and with an index
            index = torch.tensor(offs, dtype=torch.int64, device="cuda")
            for foff, doff in ((0, 0), (1, 7), (7, 16), (16, 1)):
                fbuf, fview = _dev(torch, frame, foff)
                for idx in (None, index.data_ptr()):
                    dbuf, dview = _dst(torch, n, doff)
                    r = st.lib.stenos_hip_decompress(st.ctx, fview.data_ptr(), T, frame.size, dview.data_ptr(), n, idx, st._stream_ptr())
                    assert r == n, (name, foff, doff, idx is not None, hex(r))
                    assert np.array_equal(dview.cpu().numpy(), data), (name, foff, doff, idx is not None)
                    assert _intact(dbuf, doff, n), (name, foff, doff)
        if T <= 64:  # (the batch calls take the bytesoftype whose scratch is LDS)
            devs = [_dev(torch, f, off) for off, (_, f, _, _) in zip((0, 1, 7, 16), frames)]
            dsts = [_dst(torch, d.size, off) for off, (_, _, _, d) in zip((16, 7, 1, 0), frames)]
            res = st.decompress_batch([v for _, v in devs], T, [f.size for _, f, _, _ in frames], [v for _, v in dsts])
            for k, (name, _, _, data) in enumerate(frames):
                assert res[k] == data.size, (name, "batch", hex(res[k]))
                assert np.array_equal(dsts[k][1].cpu().numpy(), data), (name, "batch")
                assert _intact(dsts[k][0], (16, 7, 1, 0)[k], data.size), (name, "batch")
    finally:
        st.close()


def _damaged_cases(oracle, audit, T: int, count: int):
    """(frame, decoded size, oracle result, oracle bytes), every one audited on the CPU first"""
    rng = np.random.default_rng([33, T])
    bases = mutation_bases(oracle, T)
    cases = []
    for i in range(count):
        payload, dsize = bases[i % len(bases)]
        m = mutate(rng, payload)
        r, want = oracle_decode(oracle, m, T, dsize)
        for regs, mis in audit_paths(T):  # (asserts that no access leaves its region: a violation ends the test here, on the CPU)
            r2, got = audit_decode(audit, m, T, dsize, regs, mis)
            assert has_error(r2) == has_error(r) and (has_error(r) or np.array_equal(got, want)), (T, i, regs, mis)
        cases.append((sg.frame_of_payload(m, T, dsize), dsize, r, want.copy()))
    return cases


@pytest.mark.parametrize("T", [2, 4, 8, 3, 12, 64])
def test_damaged_streams_after_the_audit(oracle, T):
    audit = _load("libstenos_emul_audit.so")
    audit.emul_audit_block_decompress.restype = ctypes.c_size_t
    audit.emul_audit_block_decompress.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int,
                                                  ctypes.POINTER(ctypes.c_uint64)]
    audit.emul_audit_first_name.restype = ctypes.c_char_p
    cases = _damaged_cases(oracle, audit, T, 48 if T <= 12 else 24)
    accepted = sum(1 for c in cases if not has_error(c[2]))
    assert 0 < accepted < len(cases), (accepted, len(cases))
    # intact items between the damaged ones
    rng = np.random.default_rng([34, T])
    good = []
    for k in range(len(cases) // 3):
        data = sg.make_data(rng, T, 256 * T * 2 + 37 * T + k)
        good.append((sg.frame_of_payload(sg.encode_payload(data, T, sg.OVERSIZE, rng), T, data.size), data))
    torch = _cuda()
    st = Stenos(level=1)
    try:
        single = []
        for frame, dsize, r, want in cases:
            fbuf, fview = _dev(torch, frame, 0, 0xEE)
            dbuf, dview = _dst(torch, dsize)
            g = st.lib.stenos_hip_decompress(st.ctx, fview.data_ptr(), T, frame.size, dview.data_ptr(), dsize, None, st._stream_ptr())
            if has_error(r):
                assert g >= ERR_BASE, ("the device accepts what the oracle rejects", hex(g), frame[:40].tobytes().hex())
            else:
                assert g == dsize and np.array_equal(dview.cpu().numpy(), want), (hex(g), frame[:40].tobytes().hex())
            assert _intact(dbuf, 0, dsize)
            single.append(g)
        # one batch, intact and damaged items interleaved
        items = []
        gi = 0
        for k, c in enumerate(cases):
            items.append(("bad", k))
            if k % 3 == 1 and gi < len(good):
                items.append(("good", gi))
                gi += 1
        fr, cs, ds, offs = [], [], [], []
        for n, (kind, k) in enumerate(items):
            frame, dsize = (cases[k][0], cases[k][1]) if kind == "bad" else (good[k][0], good[k][1].size)
            off = (0, 1, 7, 16)[n % 4]
            fr.append(_dev(torch, frame, (16, 7, 1, 0)[n % 4], 0xEE))
            cs.append(frame.size)
            ds.append(_dst(torch, dsize, off))
            offs.append(off)
        res = st.decompress_batch([v for _, v in fr], T, cs, [v for _, v in ds])
        for n, (kind, k) in enumerate(items):
            got = ds[n][1].cpu().numpy()
            if kind == "good":
                assert res[n] == good[k][1].size and np.array_equal(got, good[k][1]), (n, k, hex(res[n]))
            else:
                assert res[n] == single[k], (n, k, hex(res[n]), hex(single[k]))
                if not has_error(cases[k][2]):
                    assert np.array_equal(got, cases[k][3]), (n, k)
            assert _intact(ds[n][0], offs[n], got.size), (n, kind, k)
    finally:
        st.close()
