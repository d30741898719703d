#!/usr/bin/env python3
"""Variable-length ranges out of one large frame kept compressed in device memory, by offsets and lengths that live on the device:
stenos_hip_gather_ranges (index passed in, out_offsets asked for) against the only way without it -- offsets.cpu() and
lengths.cpu(), the destination addresses formed on the host (a cumulative sum), then one stenos_hip_decompress_ranges.  Both sides
are timed from device-resident offsets to delivered bytes.  Level 1; one frame of 1 GiB int32 rand12.  Lines:

  65 536 ranges at uniform random offsets, lengths uniform in 1..8 KiB
  2^20 ranges, lengths uniform in 1..512 B
  16 ranges of 16 MiB
  one range of 4 KiB
  65 536 ranges of exactly 4 KiB at multiples of 4 KiB -- also through stenos_hip_gather_rows: the cost of raggedness itself

One process; every way is run once and checked against the source, then all ways are run three untimed rounds at the shape that is
timed, then timed interleaved (gather_ranges, baseline, baseline, ...) over REPS repetitions each; a host clock around calls that
end in a synchronise.  dst_size is the sum of the lengths rounded up to 1 MiB.  Reported: microseconds per call as min / median, GB/s of bytes DELIVERED (median), x = baseline over gather_ranges
(medians), the spread between the two interleaved baseline series (the noise floor), how much of the baseline is its host
preparation (timed on its own), and the device memory the context keeps for the call (the formula of include/stenos_hip.h).

  python tools/gather_ranges_rate.py [--out FILE] [--label TEXT] [--reps N]
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

U64P = ctypes.POINTER(ctypes.c_uint64)
VPP = ctypes.POINTER(ctypes.c_void_p)
KIND, T, TOTAL = "rand12", 4, 1 << 30


class Frame:
    def __init__(self, st):
        self.st = st
        self.sb = 131072 // (256 * T) * 256 * T
        self.src = generate_torch(KIND, T, TOTAL // T, 42)
        self.frame = torch.empty(st.bound(TOTAL), dtype=torch.uint8, device="cuda")
        self.csize = st.compress(self.src, T, self.frame)
        n = ctypes.c_size_t(0)
        # (the context's own index: the calls that are given it leave it alone)
        self.index = st.lib.stenos_hip_frame_index(st.ctx, self.frame.data_ptr(), T, self.csize, ctypes.byref(n), st._stream_ptr())
        assert self.index and n.value
        self.nsb = n.value

    def held_bytes(self, n, dst_size):
        """what the context keeps for a call with out_offsets given (include/stenos_hip.h, DEVICE MEMORY)"""
        pmax = 2 * n + dst_size // self.sb
        return 16 * pmax + 4 * (n + 1) + 12 * ((n + 255) // 256) + 16 * self.nsb + 64

    def host_arrays(self, offs, lens, out):
        """what the ranges call needs, from offsets and lengths on the device: two copies, a cumulative sum, three arrays of n"""
        o = offs.cpu().numpy().astype(np.uint64)
        l = lens.cpu().numpy().astype(np.uint64)
        d = np.zeros(o.size, dtype=np.uint64)
        np.cumsum(l[:-1], out=d[1:])
        return o, l, d + np.uint64(out.data_ptr())

    def calls(self, offs, lens, out, dst_size, out_offsets):
        st, lib, n = self.st, self.st.lib, offs.numel()
        stream = st._stream_ptr()
        fp, index = self.frame.data_ptr(), self.index
        want = int(lens.sum().item())

        def gather_ranges():
            assert lib.stenos_hip_gather_ranges(st.ctx, fp, T, self.csize, n, offs.data_ptr(), lens.data_ptr(), out.data_ptr(), dst_size, out_offsets.data_ptr(), index,
                                                stream) == want

        def baseline():
            o, l, d = self.host_arrays(offs, lens, out)
            assert lib.stenos_hip_decompress_ranges(st.ctx, fp, T, self.csize, n, o.ctypes.data_as(U64P), l.ctypes.data_as(U64P), d.ctypes.data_as(VPP), index, stream) == want

        def prep():
            self.host_arrays(offs, lens, out)

        return gather_ranges, baseline, prep

    def check(self, offs, lens, out, out_offsets=None):
        o, l = offs.cpu().tolist(), lens.cpu().tolist()
        at = np.concatenate([[0], np.cumsum(np.asarray(l, dtype=np.int64))])
        if out_offsets is not None:
            assert out_offsets.cpu().tolist() == at.tolist()
        for i in list(range(min(len(o), 32))) + [len(o) - 1]:
            assert torch.equal(out[at[i]:at[i] + l[i]], self.src[o[i]:o[i] + l[i]]), (i, o[i], l[i])


WARM_ROUNDS = 3  # untimed rounds of all ways in front of the timed ones: code objects, buffers, pinned staging and clocks are up


def interleaved(fns, reps):
    for _ in range(WARM_ROUNDS):
        for f in fns:
            f()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for f, t in zip(fns, ts):
            t0 = time.perf_counter()
            f()
            t.append(time.perf_counter() - t0)
    return [(min(t) * 1e6, statistics.median(t) * 1e6) for t in ts]


def line_of(fr, name, offs, lens, reps, rows_of=None):
    nbytes = int(lens.sum().item())
    dst_size = (nbytes + (1 << 20) - 1) >> 20 << 20
    out = torch.empty(dst_size, dtype=torch.uint8, device="cuda")
    out_offsets = torch.zeros(offs.numel() + 1, dtype=torch.int64, device="cuda")
    gather_ranges, baseline, prep = fr.calls(offs, lens, out, dst_size, out_offsets)
    out.zero_()
    gather_ranges()
    fr.check(offs, lens, out, out_offsets)
    out.zero_()
    baseline()
    fr.check(offs, lens, out)
    fns = [gather_ranges, baseline, baseline, prep]
    if rows_of:
        rb = rows_of
        rows = offs // rb
        stream = fr.st._stream_ptr()

        def gather_rows():
            assert fr.st.lib.stenos_hip_gather_rows(fr.st.ctx, fr.frame.data_ptr(), T, fr.csize, rb, rows.numel(), rows.data_ptr(), out.data_ptr(), rb, fr.index, stream) == nbytes

        out.zero_()
        gather_rows()
        fr.check(offs, lens, out)
        fns.append(gather_rows)
    res = interleaved(fns, reps)
    (gmin, gmed), (amin, amed), (bmin, bmed), (pmin, pmed) = res[:4]
    bmed2, spread = min(amed, bmed), abs(amed - bmed)
    verdict = "gather_ranges wins" if bmed2 - gmed > spread and gmed < bmed2 else ("gather_ranges LOSES" if gmed - bmed2 > spread else "inside the noise")
    line = (f"{name:46s} gather_ranges {gmin:10.1f} / {gmed:10.1f} us {nbytes / gmed / 1e3:8.2f} GB/s   baseline {amin:10.1f} / {amed:10.1f} and {bmin:10.1f} / {bmed:10.1f} us"
            f" {nbytes / bmed2 / 1e3:8.2f} GB/s (of it host preparation {pmin:9.1f} / {pmed:9.1f} us)   x{bmed2 / gmed:7.2f}   spread of the baseline series {spread:7.1f} us"
            f"   device memory held {fr.held_bytes(offs.numel(), dst_size) / 1048576:8.2f} MiB   {verdict}")
    if rows_of:
        rmin, rmed = res[4]
        line += f"\n{'':46s} stenos_hip_gather_rows, the same rows {rmin:10.1f} / {rmed:10.1f} us {nbytes / rmed / 1e3:8.2f} GB/s; gather_ranges / gather_rows = {gmed / rmed:.3f} (medians)"
    del out
    torch.cuda.empty_cache()
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="")
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    st = Stenos(level=1)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    fr = Frame(st)
    lines = [f"# tools/gather_ranges_rate.py {a.label}".rstrip(),
             f"# {torch.cuda.get_device_name(0)}, level 1, index passed in, {WARM_ROUNDS} untimed rounds then {a.reps} interleaved repetitions per line; us per call as min / median, GB/s of bytes delivered (median);",
             "# gather_ranges: stenos_hip_gather_ranges with d_dst_offsets, dst_size = the sum of the lengths rounded up to 1 MiB;",
             "# baseline: offsets.cpu(), lengths.cpu(), destination addresses by a cumulative sum (numpy), one stenos_hip_decompress_ranges -- two interleaved series;",
             "# x = baseline (the faster series' median) over gather_ranges (median); both sides from device-resident offsets to delivered bytes",
             f"{KIND} T={T}, one frame of {TOTAL >> 20} MiB, ratio {TOTAL / fr.csize:.3f}, {fr.nsb} superblocks"]
    for line in lines:
        print(line, flush=True)

    def rand(n, hi):
        lens = torch.randint(1, hi + 1, (n,), device="cuda", generator=gen)
        offs = torch.randint(0, TOTAL - hi, (n,), device="cuda", generator=gen)
        return offs, lens

    cases = [("65536 ranges of 1..8192 B, uniform offsets", *rand(65536, 8192), None),
             ("1048576 ranges of 1..512 B, uniform offsets", *rand(1 << 20, 512), None),
             ("16 ranges of 16 MiB", torch.randint(0, TOTAL - (16 << 20), (16,), device="cuda", generator=gen), torch.full((16,), 16 << 20, dtype=torch.int64, device="cuda"), None),
             ("1 range of 4096 B", torch.randint(0, TOTAL - 4096, (1,), device="cuda", generator=gen), torch.full((1,), 4096, dtype=torch.int64, device="cuda"), None),
             ("65536 ranges of exactly 4096 B, row aligned", torch.randint(0, TOTAL // 4096, (65536,), device="cuda", generator=gen) * 4096,
              torch.full((65536,), 4096, dtype=torch.int64, device="cuda"), 4096)]
    for name, offs, lens, rows_of in cases:
        lines.append(line_of(fr, name, offs, lens, a.reps, rows_of))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    st.close()


if __name__ == "__main__":
    main()
