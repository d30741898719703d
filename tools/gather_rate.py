#!/usr/bin/env python3
"""Rows out of one large frame kept compressed in device memory, by row numbers that live on the device:
stenos_hip_gather_rows (index passed in) against the only way without it -- rows.cpu(), host arrays of offsets, lengths and
pointers built from it, then stenos_hip_decompress_ranges.  Level 1; one frame of 1 GiB int32 rand12, 256 MiB int16 walk,
256 MiB double sine.  Rows: 1 / 4 096 / 65 536 uniform random rows of 4 KiB, 65 536 / 1 048 576 of 256 B, the same counts with
all row numbers inside 16 superblocks (a hot set), and the identity permutation of 4 KiB rows -- the whole array -- with
stenos_hip_decompress next to it.

One process; every way is warmed up and checked, then timed interleaved (gather, ranges, ranges, ...) over REPS repetitions each;
a host clock around calls that end in a synchronise.  The ranges call is timed with its host arrays ready (built with numpy, which
is faster than the Python lists of Stenos.decompress_ranges); what it costs to get them -- the copy of the row numbers and the
arrays -- is timed on its own and reported next to it ("prep").  Reported: microseconds per call as min / median, GB/s of bytes
DELIVERED (median), x = ranges call over gather call (medians; without and with the preparation), and the spread between the two
interleaved series of the ranges call, which is the noise floor the difference is to be read against.

  python tools/gather_rate.py [--out FILE] [--label TEXT] [--reps N]
  python tools/gather_rate.py --profile     two calls of 65 536 rows of 4 KiB and nothing else that decodes (for rocprofv3 --kernel-trace --stats)
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
SHAPES = ((1, 4096), (4096, 4096), (65536, 4096), (65536, 256), (1 << 20, 256))  # (rows, row_bytes)
HOT_SUPERBLOCKS = 16
U64P = ctypes.POINTER(ctypes.c_uint64)
VPP = ctypes.POINTER(ctypes.c_void_p)


class Frame:
    def __init__(self, st, kind, T, total):
        self.st, self.T, self.total = st, T, total
        self.sb = 131072 // (256 * T) * 256 * T
        self.src = generate_torch(kind, T, total // T, 42)
        self.frame = torch.empty(st.bound(total), dtype=torch.uint8, device="cuda")
        self.csize = st.compress(self.src, T, self.frame)
        self.out = torch.empty(total, dtype=torch.uint8, device="cuda")  # where the rows go, back to back
        n = ctypes.c_size_t(0)
        # (the context's own index: gather, ranges and stenos_hip_decompress calls that are given it leave it alone)
        self.index = st.lib.stenos_hip_frame_index(st.ctx, self.frame.data_ptr(), T, self.csize, ctypes.byref(n), st._stream_ptr())
        assert self.index and n.value

    def host_arrays(self, rows, rb):
        """what the ranges call needs, from row numbers on the device: the copy and three arrays of n"""
        r = rows.cpu().numpy().astype(np.uint64)
        offs = r * np.uint64(rb)
        lens = np.full(r.size, rb, dtype=np.uint64)
        dsts = np.uint64(self.out.data_ptr()) + np.arange(r.size, dtype=np.uint64) * np.uint64(rb)
        return offs, lens, dsts

    def calls(self, rows, rb):
        """(gather, ranges, prep): the two ways to put these rows into self.out, each returns when the bytes are there"""
        st, lib, T, n = self.st, self.st.lib, self.T, rows.numel()
        stream = st._stream_ptr()
        fp, op, index, rp = self.frame.data_ptr(), self.out.data_ptr(), self.index, rows.data_ptr()
        held = list(self.host_arrays(rows, rb))

        def gather():
            assert lib.stenos_hip_gather_rows(st.ctx, fp, T, self.csize, rb, n, rp, op, rb, index, stream) == n * rb

        def ranges():
            offs, lens, dsts = held
            assert lib.stenos_hip_decompress_ranges(st.ctx, fp, T, self.csize, n, offs.ctypes.data_as(U64P), lens.ctypes.data_as(U64P), dsts.ctypes.data_as(VPP), index,
                                                    stream) == n * rb

        def prep():
            held[:] = self.host_arrays(rows, rb)

        return gather, ranges, prep

    def check(self, rows, rb):
        for i in list(range(min(rows.numel(), 32))) + [rows.numel() - 1]:
            r = int(rows[i])
            assert torch.equal(self.out[i * rb:(i + 1) * rb], self.src[r * rb:(r + 1) * rb]), (i, r)


def interleaved(fns, reps):
    ts = [[] for _ in fns]
    for _ in range(reps):
        for f, t in zip(fns, ts):
            t0 = time.perf_counter()
            f()
            t.append(time.perf_counter() - t0)
    return [(min(t) * 1e6, statistics.median(t) * 1e6) for t in ts]


def row(fr, name, rows, rb, reps, extra=None):
    gather, ranges, prep = fr.calls(rows, rb)
    fr.out.zero_()
    gather()
    fr.check(rows, rb)
    fr.out.zero_()
    ranges()
    fr.check(rows, rb)
    fns = (gather, ranges, ranges, prep) + ((extra,) if extra else ())
    res = interleaved(fns, reps)
    (gmin, gmed), (amin, amed), (bmin, bmed), (pmin, pmed) = res[:4]
    nbytes = rows.numel() * rb
    rmed = min(amed, bmed)
    spread = abs(amed - bmed)
    line = (f"{name:34s} gather {gmin:9.1f} / {gmed:9.1f} us {nbytes / gmed / 1e3:8.2f} GB/s   ranges {amin:9.1f} / {amed:9.1f} and {bmin:9.1f} / {bmed:9.1f} us"
            f" {nbytes / rmed / 1e3:8.2f} GB/s   prep {pmin:9.1f} / {pmed:9.1f} us   x{rmed / gmed:6.2f} (with prep x{(rmed + pmed) / gmed:7.2f})"
            f"   spread of the ranges series {spread:7.1f} us")
    if extra:
        emin, emed = res[4]
        line += f"\n{'':34s} stenos_hip_decompress of the whole frame {emin:9.1f} / {emed:9.1f} us {fr.total / emed / 1e3:8.2f} GB/s; gather / decompress = {gmed / emed:.3f} (medians)"
    return line, gmed, rmed, spread


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    st = Stenos(level=1)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    if a.profile:
        fr = Frame(st, "rand12", 4, 1 << 30)
        rows = torch.randint(0, fr.total // 4096, (65536,), device="cuda", generator=gen)
        gather, _, _ = fr.calls(rows, 4096)
        gather()
        gather()
        print("profile run: two gather calls of 65536 rows of 4 KiB, int32 rand12, 1 GiB frame")
        return
    lines = [f"# tools/gather_rate.py {a.label}".rstrip(),
             f"# {torch.cuda.get_device_name(0)}, level 1, index passed in, {a.reps} interleaved repetitions; us per call as min / median, GB/s of bytes delivered (median);",
             "# ranges: stenos_hip_decompress_ranges with its host arrays ready, two interleaved series; prep: rows.cpu() and the three host arrays (numpy);",
             "# x = ranges (the faster series' median) over gather (median)"]
    for line in lines:
        print(line, flush=True)
    verdict = None
    for kind, T, total in CASES:
        fr = Frame(st, kind, T, total)
        lines.append(f"{kind} T={T}, one frame of {total >> 20} MiB, ratio {total / fr.csize:.3f}, {-(-total // fr.sb)} superblocks")
        print(lines[-1], flush=True)
        for hot in (False, True):
            for n, rb in SHAPES:
                if hot and n == 1:
                    continue
                span = (HOT_SUPERBLOCKS * fr.sb if hot else total) // rb
                first = (total // 3 // fr.sb * fr.sb) // rb + 1 if hot else 0  # (hot: 16 superblocks a third into the array)
                rows = torch.randint(0, span, (n,), device="cuda", generator=gen) + first
                name = f"{n} rows of {rb} B, " + (f"inside {HOT_SUPERBLOCKS} superblocks" if hot else "uniform")
                line, gmed, rmed, spread = row(fr, name, rows, rb, a.reps)
                lines.append(line)
                print(line, flush=True)
                if kind == "rand12" and not hot and (n, rb) == (65536, 4096):
                    verdict = (gmed, rmed, spread)
        stream = st._stream_ptr()

        def plain():
            assert st.lib.stenos_hip_decompress(st.ctx, fr.frame.data_ptr(), fr.T, fr.csize, fr.out.data_ptr(), fr.total, fr.index, stream) == fr.total

        plain()
        rows = torch.arange(total // 4096, device="cuda")
        line, _, _, _ = row(fr, f"identity, {total // 4096} rows of 4096 B", rows, 4096, a.reps, extra=plain)
        assert torch.equal(fr.out, fr.src)
        lines.append(line)
        print(line, flush=True)
        del fr
        torch.cuda.empty_cache()
    gmed, rmed, spread = verdict
    lines.append(f"# the condition (65536 uniform random rows of 4 KiB, int32): gather {gmed:.1f} us, ranges {rmed:.1f} us, gap {rmed - gmed:.1f} us, "
                 f"spread of the two ranges series {spread:.1f} us: " + ("met" if rmed - gmed > spread and gmed < rmed else "NOT met"))
    print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    st.close()


if __name__ == "__main__":
    main()
