#!/usr/bin/env python3
"""Rows of many frames kept compressed in device memory replaced by (frame number, row number) pairs that live on the device:
stenos_hip_update_rows_batch (index passed in, every updated frame into a second buffer) against the only way without it -- the
pairs brought to the host and grouped by frame there, one stenos_hip_update_rows per touched frame (its row numbers uploaded, its
source rows put in order by one device gather; the frame's index passed in), one device copy per untouched frame.  Level 1, int32
rand12.  Lines:
  4 096 frames of 64 KiB, rows of 256 B: 256 and 65 536 random unique pairs, and every row
  16 and 8 frames of 128 MiB, rows of 4 KiB, 4 096 random unique pairs
  1 frame of 1 GiB, rows of 4 KiB, 4 096 random unique pairs: against stenos_hip_update_rows itself

One process, one context per way (so that what each keeps in device memory can be told apart); every way is warmed up and checked
-- both must leave the same frames, byte for byte --, then timed interleaved (batch, baseline, baseline, ...) over REPS repetitions
each; a host clock around calls that end in a synchronise.  Reported: microseconds per call as min / median, x = baseline over batch
(medians), the spread between the two interleaved series of the baseline, which is the noise floor the difference is to be read
against, the frames and superblocks touched, and the device memory each way's context holds after the line.

  python tools/update_batch_rate.py [--out FILE] [--label TEXT] [--reps N] [--only NAME]
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

KIND, T = "rand12", 4
SB = 131072 // (256 * T) * 256 * T


def free_bytes():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


class Store:
    """m frames of `nbytes` each on the device, their outputs for both ways, the index of all of them in a tensor of the caller's"""

    def __init__(self, m, nbytes, row):
        self.m, self.nbytes, self.row = m, nbytes, row
        self.batch, self.base = Stenos(level=1), Stenos(level=1)
        cap = self.batch.bound(nbytes)
        src = generate_torch(KIND, T, nbytes // T, 42).view(torch.uint8)
        self.frames, self.csizes = [], []
        step = max(1, min(m, (1 << 30) // nbytes))
        for at in range(0, m, step):  # (the frames differ: the data is rotated by a row per frame)
            k = min(step, m - at)
            srcs = [torch.roll(src, (at + i) * row) for i in range(k)]
            dsts = [torch.empty(cap, dtype=torch.uint8, device="cuda") for _ in range(k)]
            res = self.base.compress_batch(srcs, T, dsts)
            assert all(r < (1 << 63) for r in res)
            self.frames += dsts
            self.csizes += res
        del src, srcs
        self.out_batch = [torch.empty(cap, dtype=torch.uint8, device="cuda") for _ in range(m)]
        self.out_base = [torch.empty(cap, dtype=torch.uint8, device="cuda") for _ in range(m)]
        self.nsb = -(-nbytes // SB)
        p, entries = self.base.frames_index(self.frames, T, self.csizes)
        assert entries == m * (self.nsb + 1)
        self.index = torch.empty(entries, dtype=torch.int64, device="cuda")
        hip = ctypes.CDLL("libamdhip64.so")
        assert hip.hipMemcpy(ctypes.c_void_p(self.index.data_ptr()), ctypes.c_void_p(p), ctypes.c_size_t(entries * 8), 3) == 0
        self.rows_per_frame = nbytes // row

    def close(self):
        self.batch.close()
        self.base.close()

    def calls(self, fids, rows, single=False):
        """fids, rows: int64 CUDA tensors of n unique pairs; the source rows are noise of the data's kind"""
        n, m, row = rows.numel(), self.m, self.row
        gen = torch.Generator(device="cuda")
        gen.manual_seed(n)
        src = torch.randint(0, 1 << 12, (n, row // 4), dtype=torch.int32, device="cuda", generator=gen).view(torch.uint8).reshape(n, row)
        P, Z = ctypes.c_void_p * m, ctypes.c_size_t * m
        fp, fz = P(*[t.data_ptr() for t in self.frames]), Z(*self.csizes)
        op, oz = P(*[t.data_ptr() for t in self.out_batch]), Z(*[t.numel() for t in self.out_batch])
        res = Z(*([0] * m))
        lib, stream, ip = self.batch.lib, self.batch._stream_ptr(), self.index.data_ptr()
        sizes = {}

        def batch():
            r = lib.stenos_hip_update_rows_batch(self.batch.ctx, m, T, fp, fz, row, n, fids.data_ptr(), rows.data_ptr(), src.data_ptr(), row, op, oz, res, ip, stream)
            assert r == 0, hex(r)
            sizes["batch"] = list(res)

        def baseline():
            # the pairs come down and are grouped by frame on the host; the sources are put in that order by one device gather
            hf, hr = fids.cpu().numpy(), rows.cpu().numpy()
            order = np.argsort(hf, kind="stable")
            counts = np.bincount(hf, minlength=m)
            starts = np.concatenate(([0], np.cumsum(counts)))
            d_rows = torch.from_numpy(np.ascontiguousarray(hr[order])).cuda()
            d_src = src.index_select(0, torch.from_numpy(order).cuda())
            out = []
            for f in range(m):
                k = int(counts[f])
                if k == 0:
                    self.out_base[f][:self.csizes[f]].copy_(self.frames[f][:self.csizes[f]])
                    out.append(self.csizes[f])
                    continue
                a = int(starts[f])
                r = lib.stenos_hip_update_rows(self.base.ctx, self.frames[f].data_ptr(), T, self.csizes[f], row, k, d_rows.data_ptr() + 8 * a, d_src.data_ptr() + row * a, row,
                                               self.out_base[f].data_ptr(), self.out_base[f].numel(), ip + 8 * f * (self.nsb + 1), stream)
                assert r < (1 << 63), hex(r)
                out.append(r)
            torch.cuda.synchronize()
            sizes["baseline"] = out

        def single_call():  # (m == 1: stenos_hip_update_rows itself, nothing brought down)
            r = lib.stenos_hip_update_rows(self.base.ctx, self.frames[0].data_ptr(), T, self.csizes[0], row, n, rows.data_ptr(), src.data_ptr(), row,
                                           self.out_base[0].data_ptr(), self.out_base[0].numel(), ip, stream)
            assert r < (1 << 63), hex(r)
            sizes["baseline"] = [r]

        return batch, (single_call if single else baseline), sizes


def interleaved(fns, reps):
    ts = [[] for _ in fns]
    for _ in range(reps):
        for f, t in zip(fns, ts):
            t0 = time.perf_counter()
            f()
            t.append(time.perf_counter() - t0)
    return [(min(t) * 1e6, statistics.median(t) * 1e6) for t in ts]


def measure(st, name, fids, rows, reps, single=False):
    batch, baseline, sizes = st.calls(fids, rows, single)
    held = {}
    for way, fn in (("batch", batch), ("baseline", baseline)):
        before = free_bytes()
        fn()
        held[way] = before - free_bytes()
    assert sizes["batch"] == sizes["baseline"], "the two ways leave frames of different sizes"
    for f, r in enumerate(sizes["batch"]):
        assert torch.equal(st.out_batch[f][:r], st.out_base[f][:r]), f"the two ways leave different frames ({f})"
    frames_touched = int(torch.unique(fids).numel())
    sbs_touched = int(torch.unique(fids * st.nsb + rows * st.row // SB).numel())
    (umin, umed), (amin, amed), (bmin, bmed) = interleaved((batch, baseline, baseline), reps)
    best, spread = min(amed, bmed), abs(amed - bmed)
    line = (f"{name:44s} {rows.numel():8d} pairs, {frames_touched:5d} frames, {sbs_touched:6d} superblocks touched   batch {umin:11.1f} / {umed:11.1f} us   baseline "
            f"{amin:11.1f} / {amed:11.1f} and {bmin:11.1f} / {bmed:11.1f} us   x{best / umed:8.2f}   spread of the baseline series {spread:9.1f} us   device memory "
            f"taken by the line's first call: batch {held['batch'] / 2**20:8.1f} MiB, baseline {held['baseline'] / 2**20:8.1f} MiB")
    print(line, flush=True)
    return line, (umed, best, spread)


def random_pairs(st, n, seed):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    all_pairs = st.m * st.rows_per_frame
    pick = torch.randperm(all_pairs, device="cuda", generator=gen)[:n] if n < all_pairs else torch.arange(all_pairs, device="cuda")
    return (pick // st.rows_per_frame).contiguous(), (pick % st.rows_per_frame).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default=None, help="small, large or one")
    a = ap.parse_args()
    lines = [f"# tools/update_batch_rate.py {a.label}".rstrip(),
             f"# {torch.cuda.get_device_name(0)}, level 1, {KIND} T={T}, superblocks of {SB} bytes, index passed in, {a.reps} interleaved repetitions; us per call as min / median;",
             "# batch: stenos_hip_update_rows_batch, every frame into a second buffer; baseline: the pairs to the host, grouped by frame, one stenos_hip_update_rows per touched",
             "# frame, one device copy per untouched frame, two interleaved series; x = baseline (the faster series' median) over batch (median); both ways leave the same",
             "# frames (checked, byte for byte)"]
    for line in lines:
        print(line, flush=True)
    verdict = None
    if a.only in (None, "small"):
        st = Store(4096, 65536, 256)
        for n in (256, 65536, st.m * st.rows_per_frame):
            line, v = measure(st, "4096 frames of 64 KiB, rows of 256 B", *random_pairs(st, n, 7), a.reps)
            lines.append(line)
            if n == 65536:
                verdict = v
        st.close()
        del st
    if a.only in (None, "large"):
        for m in (16, 8):
            st = Store(m, 128 << 20, 4096)
            line, _ = measure(st, f"{m} frames of 128 MiB, rows of 4 KiB", *random_pairs(st, 4096, 8), a.reps)
            lines.append(line)
            st.close()
            del st
            torch.cuda.empty_cache()
    if a.only in (None, "one"):
        st = Store(1, 1 << 30, 4096)
        line, _ = measure(st, "1 frame of 1 GiB, rows of 4 KiB (against stenos_hip_update_rows itself)", *random_pairs(st, 4096, 9), a.reps, single=True)
        lines.append(line)
        st.close()
    lines.append("# device memory: what the way's context takes during the line's first call (the contexts keep their buffers, so a later line of the same store shows "
                 "only the growth)")
    if verdict:
        umed, bmed, spread = verdict
        lines.append(f"# the condition (4 096 frames, 65 536 random unique pairs): batch {umed:.1f} us, baseline {bmed:.1f} us, gap {bmed - umed:.1f} us, "
                     f"spread of the two baseline series {spread:.1f} us: " + ("met" if bmed - umed > spread and umed < bmed else "NOT met"))
    for line in lines[-2:]:
        print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
