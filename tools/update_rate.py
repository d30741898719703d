#!/usr/bin/env python3
"""Rows of one large frame kept compressed in device memory replaced by row numbers that live on the device:
stenos_hip_update_rows (index passed in, the updated frame into a second buffer) against the only way without it --
stenos_hip_decompress of the whole frame into a scratch tensor of the array's size, index_copy_ of the rows, stenos_hip_compress into
the second buffer.  Level 1; one frame of 1 GiB int32 rand12; 1 / 256 / 4 096 / 65 536 uniform random rows of 4 KiB (unique), and
every row.

One process, one context per way (so that what each keeps in device memory can be told apart); every way is warmed up and checked
-- both must leave the same frame, byte for byte --, then timed interleaved (update, baseline, baseline, ...) over REPS repetitions
each; a host clock around calls that end in a synchronise.  Reported: microseconds per call as min / median, x = baseline over update
(medians), the spread between the two interleaved series of the baseline, which is the noise floor the difference is to be read
against, the superblocks the rows touch, and the extra device memory of both ways (what the context holds after the calls, plus the
baseline's scratch tensor).

  python tools/update_rate.py [--out FILE] [--label TEXT] [--reps N]
  python tools/update_rate.py --profile     two calls of 4 096 rows and nothing else that decodes (for rocprofv3 --kernel-trace --stats)
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from stenos_amd.api import Stenos  # noqa: E402
from stenos_amd.datagen import generate_torch  # noqa: E402

KIND, T, TOTAL, ROW = "rand12", 4, 1 << 30, 4096
COUNTS = (1, 256, 4096, 65536)


def free_bytes():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


class Setup:
    def __init__(self):
        self.up, self.base = Stenos(level=1), Stenos(level=1)
        self.sb = 131072 // (256 * T) * 256 * T
        self.src = generate_torch(KIND, T, TOTAL // T, 42)
        cap = self.up.bound(TOTAL)
        self.frame = torch.empty(cap, dtype=torch.uint8, device="cuda")
        self.csize = self.base.compress(self.src, T, self.frame)
        self.out_up = torch.empty(cap, dtype=torch.uint8, device="cuda")
        self.out_base = torch.empty(cap, dtype=torch.uint8, device="cuda")
        # an index of the caller's own (the update replaces the context's with the new frame's)
        n = ctypes.c_size_t(0)
        p = self.base.lib.stenos_hip_frame_index(self.base.ctx, self.frame.data_ptr(), T, self.csize, ctypes.byref(n), self.base._stream_ptr())
        assert p and n.value == -(-TOTAL // self.sb)
        self.nsb = n.value
        self.index = torch.empty(self.nsb + 1, dtype=torch.int64, device="cuda")
        hip = ctypes.CDLL("libamdhip64.so")
        assert hip.hipMemcpy(ctypes.c_void_p(self.index.data_ptr()), ctypes.c_void_p(p), ctypes.c_size_t((self.nsb + 1) * 8), 3) == 0
        self.scratch = None
        self.rows_of_noise = torch.randint(0, 1 << 12, (TOTAL // ROW, ROW // 4), dtype=torch.int32, device="cuda").view(torch.uint8).reshape(TOTAL // ROW, ROW)

    def calls(self, rows):
        n = rows.numel()
        src = self.rows_of_noise[:n].contiguous()
        lib, stream = self.up.lib, self.up._stream_ptr()
        fp, ip = self.frame.data_ptr(), self.index.data_ptr()
        sizes = {}

        def update():
            sizes["update"] = r = lib.stenos_hip_update_rows(self.up.ctx, fp, T, self.csize, ROW, n, rows.data_ptr(), src.data_ptr(), ROW, self.out_up.data_ptr(),
                                                             self.out_up.numel(), ip, stream)
            assert r < (1 << 63), hex(r)

        def baseline():
            if self.scratch is None:
                self.scratch = torch.empty(TOTAL, dtype=torch.uint8, device="cuda")
            assert lib.stenos_hip_decompress(self.base.ctx, fp, T, self.csize, self.scratch.data_ptr(), TOTAL, ip, stream) == TOTAL
            self.scratch.view(-1, ROW).index_copy_(0, rows, src)
            sizes["baseline"] = r = lib.stenos_hip_compress(self.base.ctx, self.scratch.data_ptr(), T, TOTAL, self.out_base.data_ptr(), self.out_base.numel(), stream)
            assert r < (1 << 63), hex(r)

        return update, baseline, sizes


def interleaved(fns, reps):
    ts = [[] for _ in fns]
    for _ in range(reps):
        for f, t in zip(fns, ts):
            t0 = time.perf_counter()
            f()
            t.append(time.perf_counter() - t0)
    return [(min(t) * 1e6, statistics.median(t) * 1e6) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    su = Setup()
    nrows = TOTAL // ROW
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    perm = torch.randperm(nrows, device="cuda", generator=gen)
    if a.profile:
        update, _, _ = su.calls(perm[:4096].contiguous())
        update()
        update()
        print("profile run: two update calls of 4096 rows of 4 KiB, int32 rand12, 1 GiB frame")
        return
    lines = [f"# tools/update_rate.py {a.label}".rstrip(),
             f"# {torch.cuda.get_device_name(0)}, level 1, index passed in, {a.reps} interleaved repetitions; us per call as min / median;",
             "# update: stenos_hip_update_rows into a second buffer; baseline: stenos_hip_decompress into a scratch tensor, index_copy_, stenos_hip_compress into the",
             "# second buffer, two interleaved series; x = baseline (the faster series' median) over update (median); both ways leave the same frame (checked)",
             f"{KIND} T={T}, one frame of {TOTAL >> 20} MiB, ratio {TOTAL / su.csize:.3f}, {su.nsb} superblocks of {su.sb} bytes, rows of {ROW} B, unique, uniform"]
    for line in lines:
        print(line, flush=True)
    verdict = None
    mem = {}
    for n in COUNTS + (nrows,):
        rows = (perm[:n] if n < nrows else torch.arange(nrows, device="cuda")).contiguous()
        update, baseline, sizes = su.calls(rows)
        for name, fn in (("update", update), ("baseline", baseline)):
            before = free_bytes()
            fn()
            held = before - free_bytes()
            mem[name + "_sum"] = mem.get(name + "_sum", 0) + held
        assert sizes["update"] == sizes["baseline"], sizes
        assert torch.equal(su.out_up[:sizes["update"]], su.out_base[:sizes["update"]]), "the two ways leave different frames"
        touched = int(torch.unique(rows * ROW // su.sb).numel())
        (umin, umed), (amin, amed), (bmin, bmed) = interleaved((update, baseline, baseline), a.reps)
        bmed_best, spread = min(amed, bmed), abs(amed - bmed)
        line = (f"{n:7d} rows, {touched:5d} superblocks touched   update {umin:10.1f} / {umed:10.1f} us   baseline {amin:10.1f} / {amed:10.1f} and {bmin:10.1f} / {bmed:10.1f} us"
                f"   x{bmed_best / umed:7.2f}   spread of the baseline series {spread:8.1f} us   extra device memory so far: update {mem['update_sum'] / 2**20:7.1f} MiB,"
                f" baseline {mem['baseline_sum'] / 2**20:7.1f} MiB")
        lines.append(line)
        print(line, flush=True)
        if n == 256:
            verdict = (umed, bmed_best, spread)
    lines.append(f"# extra device memory: what the way's context (and torch, for the baseline's scratch tensor of {TOTAL >> 20} MiB) holds after the line's first call, "
                 "largest so far; the update's grows with the superblocks touched")
    print(lines[-1], flush=True)
    umed, bmed, spread = verdict
    lines.append(f"# the condition (256 uniform random rows of 4 KiB): update {umed:.1f} us, baseline {bmed:.1f} us, gap {bmed - umed:.1f} us, "
                 f"spread of the two baseline series {spread:.1f} us: " + ("met" if bmed - umed > spread and umed < bmed else "NOT met"))
    print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    su.up.close()
    su.base.close()


if __name__ == "__main__":
    main()
