#!/usr/bin/env python3
"""Byte ranges out of one large frame kept compressed in device memory: stenos_hip_decompress_ranges (index passed in)
against the only way without it -- stenos_hip_decompress of the whole frame into scratch, then device-to-device copies of the
ranges.  Level 1; one frame of 1 GiB int32 rand12, 256 MiB int16 walk, 256 MiB double sine.  Rows: one range of 4 KiB / 64 KiB /
1 MiB / 64 MiB / the whole array at an arbitrary byte offset, and 4 096 / 65 536 random 4 KiB ranges in one call.

One process; both ways are warmed up, then timed interleaved (new, old, new, old, ...) over REPS repetitions each; a host clock
around calls that end in a synchronise.  Reported: microseconds per call as min / median, GB/s of bytes DELIVERED (median), and
the ratio old / new of the medians.  The whole-array row also gives two interleaved series of stenos_hip_decompress itself: their
spread is the noise floor the ranges call's whole-array time is to be read against.

  python tools/range_rate.py [--out FILE] [--label TEXT] [--reps N]
  python tools/range_rate.py --profile     two calls of 4 096 ranges and nothing else that decodes (for rocprofv3 --kernel-trace --stats)
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from stenos_amd.api import Stenos  # noqa: E402
from stenos_amd.datagen import generate_torch  # noqa: E402

CASES = (("rand12", 4, 1 << 30), ("walk", 2, 256 << 20), ("sine", 8, 256 << 20))
SINGLE = (4 << 10, 64 << 10, 1 << 20, 64 << 20)
MANY = (4096, 65536)
HIP = ctypes.CDLL("libamdhip64.so")
HIP.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
HIP.hipStreamSynchronize.argtypes = [ctypes.c_void_p]


class Frame:
    def __init__(self, st, kind, T, total):
        self.st, self.T, self.total = st, T, total
        self.src = generate_torch(kind, T, total // T, 42)
        self.frame = torch.empty(st.bound(total), dtype=torch.uint8, device="cuda")
        self.csize = st.compress(self.src, T, self.frame)
        self.scratch = torch.empty(total, dtype=torch.uint8, device="cuda")  # what the old way inflates into
        self.out = torch.empty(total, dtype=torch.uint8, device="cuda")     # where the ranges go, back to back
        n = ctypes.c_size_t(0)
        # (the context's own index: ranges calls and stenos_hip_decompress calls that are given it leave it alone)
        self.index = st.lib.stenos_hip_frame_index(st.ctx, self.frame.data_ptr(), T, self.csize, ctypes.byref(n), st._stream_ptr())
        assert self.index and n.value

    def calls(self, ranges):
        """(new, old): the two ways to put these ranges into self.out, each a function that returns when the bytes are there"""
        st, lib, T, n = self.st, self.st.lib, self.T, len(ranges)
        U, P = ctypes.c_uint64 * n, ctypes.c_void_p * n
        offs, lens = U(*[o for o, _ in ranges]), U(*[k for _, k in ranges])
        at = np.concatenate(([0], np.cumsum([k for _, k in ranges])[:-1])).tolist()
        base, scratch = self.out.data_ptr(), self.scratch.data_ptr()
        dsts = P(*[base + a for a in at])
        want = sum(k for _, k in ranges)
        stream = st._stream_ptr()
        fp, sp, index = self.frame.data_ptr(), self.scratch.data_ptr(), self.index
        copies = [(base + a, scratch + o, k) for a, (o, k) in zip(at, ranges)]

        def new():
            assert lib.stenos_hip_decompress_ranges(st.ctx, fp, T, self.csize, n, offs, lens, dsts, index, stream) == want

        def old():
            assert lib.stenos_hip_decompress(st.ctx, fp, T, self.csize, sp, self.total, index, stream) == self.total
            for d, s, k in copies:
                HIP.hipMemcpyAsync(d, s, k, 3, stream)
            HIP.hipStreamSynchronize(stream)

        return new, old

    def check(self, ranges):
        at = 0
        for o, k in ranges[:64]:
            assert torch.equal(self.out[at:at + k], self.src[o:o + k]), (o, k)
            at += k


def interleaved(fns, reps):
    ts = [[] for _ in fns]
    for _ in range(reps):
        for f, t in zip(fns, ts):
            t0 = time.perf_counter()
            f()
            t.append(time.perf_counter() - t0)
    return [(min(t) * 1e6, statistics.median(t) * 1e6) for t in ts]


def row(fr, name, ranges, reps):
    new, old = fr.calls(ranges)
    fr.out.zero_()
    new()
    fr.check(ranges)
    fr.out.zero_()
    old()
    fr.check(ranges)
    (nmin, nmed), (omin, omed) = interleaved((new, old), reps)
    nbytes = sum(k for _, k in ranges)
    return (f"{name:28s} ranges call {nmin:10.1f} / {nmed:10.1f} us  {nbytes / nmed / 1e3:8.2f} GB/s   whole decode + copies {omin:10.1f} / {omed:10.1f} us"
            f"  {nbytes / omed / 1e3:8.2f} GB/s   x{omed / nmed:8.1f}")


def whole_row(fr, reps):
    st, lib = fr.st, fr.st.lib
    new, old = fr.calls([(0, fr.total)])
    stream = st._stream_ptr()

    def plain():
        assert lib.stenos_hip_decompress(st.ctx, fr.frame.data_ptr(), fr.T, fr.csize, fr.scratch.data_ptr(), fr.total, fr.index, stream) == fr.total

    new(), old(), plain()
    assert torch.equal(fr.out, fr.src)
    (nmin, nmed), (omin, omed), (amin, amed), (bmin, bmed) = interleaved((new, old, plain, plain), reps)
    gb = fr.total / 1e3
    return (f"{'the whole array':28s} ranges call {nmin:10.1f} / {nmed:10.1f} us  {gb / nmed:8.2f} GB/s   whole decode + copies {omin:10.1f} / {omed:10.1f} us"
            f"  {gb / omed:8.2f} GB/s   x{omed / nmed:8.1f}\n"
            f"{'':28s} stenos_hip_decompress itself, two interleaved series: {amin:10.1f} / {amed:10.1f} us and {bmin:10.1f} / {bmed:10.1f} us"
            f"  ({gb / amed:.2f} GB/s); ranges call / decompress = {nmed / amed:.3f} (medians), spread between the series {abs(amed - bmed) / min(amed, bmed) * 100:.2f} %")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    st = Stenos(level=1)
    rng = np.random.default_rng(7)
    if a.profile:
        fr = Frame(st, "rand12", 4, 256 << 20)
        ranges = [(int(o), 4096) for o in rng.integers(0, fr.total - 4096, 4096)]
        new, _ = fr.calls(ranges)
        new()
        new()
        print("profile run: two calls of 4096 ranges of 4 KiB, int32 rand12, 256 MiB frame")
        return
    lines = [f"# tools/range_rate.py {a.label}".rstrip(),
             f"# {torch.cuda.get_device_name(0)}, level 1, index passed in, {a.reps} interleaved repetitions; us per call as min / median, GB/s of bytes delivered (median),"
             " x = whole decode + copies over ranges call (medians)"]
    for line in lines:
        print(line, flush=True)
    for kind, T, total in CASES:
        fr = Frame(st, kind, T, total)
        lines.append(f"{kind} T={T}, one frame of {total >> 20} MiB, ratio {total / fr.csize:.3f}, {-(-total // (131072 // (256 * T) * 256 * T))} superblocks")
        print(lines[-1], flush=True)
        for size in SINGLE:
            off = int(rng.integers(0, total - size)) | 1
            lines.append(row(fr, f"one range of {size >> 10} KiB", [(off, size)], a.reps))
            print(lines[-1], flush=True)
        lines.append(whole_row(fr, a.reps))
        print(lines[-1], flush=True)
        for n in MANY:
            if n * 4096 > total:
                continue
            ranges = [(int(o), 4096) for o in rng.integers(0, total - 4096, n)]
            lines.append(row(fr, f"{n} random ranges of 4 KiB", ranges, a.reps))
            print(lines[-1], flush=True)
        del fr
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    st.close()


if __name__ == "__main__":
    main()
