#!/usr/bin/env python3
"""Rows out of many frames kept compressed in device memory, by (frame number, row number) pairs that live on the device:
stenos_hip_gather_rows_batch (index of stenos_hip_frames_index passed in) against the only way without it -- the pairs to the
host, grouped by frame, then one stenos_hip_gather_rows per frame touched with that frame's index ready (its slice of the batch
index).  Level 1, int32 rand12:
  4 096 frames of 64 KiB (the batch of profiles/batch_rate.txt): 65 536 and 1 048 576 uniform random pairs of 256 B, 65 536 pairs
      of 4 KiB, 65 536 pairs of 256 B concentrated in 16 frames;
  8 frames of 128 MiB: 65 536 pairs of 256 B and of 4 KiB;
  one frame of 1 GiB (m = 1): the same pairs, next to stenos_hip_gather_rows on that frame.

One process; every way is warmed up and checked, then timed interleaved (batch, loop, batch, ...) over REPS repetitions each; a
host clock around calls that end in a synchronise.  The loop is timed with its host-side grouping done and the sorted row numbers
back on the device; that preparation -- ids.cpu(), the stable sort by frame, the upload -- is timed on its own ("prep").  The loop
delivers the rows in frame order, the batch call in pair order: the same bytes.  Reported: microseconds as min / median, GB/s of
bytes DELIVERED (median), x = loop over batch (medians; without and with the preparation).

  python tools/gather_batch_rate.py [--out FILE] [--label TEXT] [--reps N]
  python tools/gather_batch_rate.py --profile    two batch calls of 65 536 pairs of 256 B over the 4 096 frames and nothing else that decodes
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

T, SB = 4, 131072


class Store:
    """m frames of `size` bytes each, compressed in one batch call, and their index"""

    def __init__(self, st, m, size):
        self.st, self.m, self.size = st, m, size
        self.src = generate_torch("rand12", T, m * size // T, 42)
        srcs = [self.src[f * size:(f + 1) * size] for f in range(m)]
        self.frames = [torch.empty(st.bound(size), dtype=torch.uint8, device="cuda") for _ in range(m)]
        if m > 1:
            self.csizes = st.compress_batch(srcs, T, self.frames)
        else:
            self.csizes = [st.compress(srcs[0], T, self.frames[0])]
        assert all(c < (1 << 63) for c in self.csizes)
        self.P, self.Z = (ctypes.c_void_p * m)(*[f.data_ptr() for f in self.frames]), (ctypes.c_size_t * m)(*self.csizes)
        self.index, self.entries = st.frames_index(self.frames, T, self.csizes)  # (the context's own: the gather calls given it leave it alone)
        nsb = -(-size // SB)
        self.slice = [self.index + 8 * f * (nsb + 1) for f in range(m)]  # frame f's own index inside it
        self.out = torch.empty(0, dtype=torch.uint8, device="cuda")

    def group(self, ids, rows):
        """what the loop needs, from pairs on the device: (sorted rows on the device, [(frame, first, count)] on the host)"""
        order = torch.sort(ids, stable=True)
        f = order.values.cpu().numpy()
        sorted_rows = rows[order.indices].contiguous()
        starts = np.flatnonzero(np.r_[True, f[1:] != f[:-1]])
        counts = np.diff(np.r_[starts, f.size])
        torch.cuda.synchronize()
        return sorted_rows, [(int(f[s]), int(s), int(c)) for s, c in zip(starts, counts)], order.indices

    def calls(self, ids, rows, rb):
        st, lib, n = self.st, self.st.lib, rows.numel()
        stream = st._stream_ptr()
        if self.out.numel() < n * rb:
            self.out = torch.empty(n * rb, dtype=torch.uint8, device="cuda")
        op, ip, rp = self.out.data_ptr(), ids.data_ptr(), rows.data_ptr()
        held = list(self.group(ids, rows))

        def batch():
            assert lib.stenos_hip_gather_rows_batch(st.ctx, self.m, T, self.P, self.Z, rb, n, ip, rp, op, rb, self.index, stream) == n * rb

        def loop():
            sorted_rows, groups, _ = held
            base = sorted_rows.data_ptr()
            for f, first, count in groups:
                assert lib.stenos_hip_gather_rows(st.ctx, self.frames[f].data_ptr(), T, self.csizes[f], rb, count, base + 8 * first, op + first * rb, rb, self.slice[f],
                                                  stream) == count * rb

        def prep():
            held[:] = self.group(ids, rows)

        return batch, loop, prep, held

    def check(self, ids, rows, rb, order=None):
        i = torch.arange(0, rows.numel(), max(1, rows.numel() // 4096), device="cuda")
        k = i if order is None else order[i]
        at = (ids[k] * self.size + rows[k] * rb)[:, None] + torch.arange(rb, device="cuda")
        got = self.out[: rows.numel() * rb].view(-1, rb)[i]
        assert torch.equal(got, self.src[at]), "rows differ"


def interleaved(fns, reps):
    ts = [[] for _ in fns]
    for _ in range(reps):
        for f, t in zip(fns, ts):
            t0 = time.perf_counter()
            f()
            t.append(time.perf_counter() - t0)
    return [(min(t) * 1e6, statistics.median(t) * 1e6) for t in ts]


def row(store, name, ids, rows, rb, reps, single=None):
    batch, loop, prep, held = store.calls(ids, rows, rb)
    store.out.zero_()
    batch()
    store.check(ids, rows, rb)
    store.out.zero_()
    loop()
    store.check(ids, rows, rb, held[2])
    fns = (batch, loop, batch, prep) + ((single,) if single else ())
    res = interleaved(fns, reps)
    (amin, amed), (lmin, lmed), (bmin, bmed), (pmin, pmed) = res[:4]
    bmed2 = min(amed, bmed)
    nbytes = rows.numel() * rb
    line = (f"{name:44s} batch {amin:10.1f} / {amed:10.1f} and {bmin:10.1f} / {bmed:10.1f} us {nbytes / bmed2 / 1e3:8.2f} GB/s   loop of {len(held[1]):5d} calls "
            f"{lmin:11.1f} / {lmed:11.1f} us {nbytes / lmed / 1e3:8.2f} GB/s   prep {pmin:9.1f} / {pmed:9.1f} us   x{lmed / bmed2:8.2f} (with prep x{(lmed + pmed) / bmed2:8.2f})"
            f"   spread of the batch series {abs(amed - bmed):7.1f} us")
    if single:
        smin, smed = res[4]
        line += f"\n{'':44s} stenos_hip_gather_rows on the frame {smin:10.1f} / {smed:10.1f} us; batch / single = {bmed2 / smed:.3f} (medians)"
    return line, bmed2, lmed


def pairs(gen, m, size, n, rb, frames=None):
    ids = torch.randint(0, frames or m, (n,), device="cuda", generator=gen)
    if frames:
        ids = ids * (m // frames) + 3  # (16 frames spread over the store)
    return ids, torch.randint(0, size // rb, (n,), device="cuda", generator=gen)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    st = Stenos(level=1)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    if a.profile:
        store = Store(st, 4096, 64 << 10)
        ids, rows = pairs(gen, store.m, store.size, 65536, 256)
        batch = store.calls(ids, rows, 256)[0]
        batch()
        batch()
        print("profile run: two batch gather calls of 65536 pairs of 256 B, 4096 int32 rand12 frames of 64 KiB")
        return
    lines = [f"# tools/gather_batch_rate.py {a.label}".rstrip(),
             f"# {torch.cuda.get_device_name(0)}, level 1, int32 rand12, index passed in, {a.reps} interleaved repetitions; us as min / median, GB/s of bytes delivered (median);",
             "# batch: stenos_hip_gather_rows_batch, two interleaved series; loop: one stenos_hip_gather_rows per frame touched, pairs grouped and per-frame indices ready;",
             "# prep: ids.cpu(), stable sort by frame, sorted rows back on the device; x = loop (median) over batch (the faster series' median)"]
    for line in lines:
        print(line, flush=True)
    verdict = None
    for m, size, shapes in ((4096, 64 << 10, ((65536, 256, None), (1 << 20, 256, None), (65536, 4096, None), (65536, 256, 16))),
                            (8, 128 << 20, ((65536, 256, None), (65536, 4096, None))),
                            (1, 1 << 30, ((65536, 256, None), (65536, 4096, None)))):
        store = Store(st, m, size)
        lines.append(f"{m} frame(s) of {size >> 10} KiB, ratio {m * size / sum(store.csizes):.3f}, {store.entries - m} superblocks")
        print(lines[-1], flush=True)
        for n, rb, hot in shapes:
            ids, rows = pairs(gen, m, size, n, rb, hot)
            single = None
            if m == 1:
                stream = st._stream_ptr()

                def single(n=n, rb=rb, rows=rows):
                    assert st.lib.stenos_hip_gather_rows(st.ctx, store.frames[0].data_ptr(), T, store.csizes[0], rb, n, rows.data_ptr(), store.out.data_ptr(), rb, store.index,
                                                         stream) == n * rb
            name = f"{n} pairs of {rb} B, " + (f"inside {hot} frames" if hot else "uniform")
            line, bmed, lmed = row(store, name, ids, rows, rb, a.reps, single)
            lines.append(line)
            print(line, flush=True)
            if m == 4096 and (n, rb, hot) == (65536, 256, None):
                verdict = (bmed, lmed)
        del store
        torch.cuda.empty_cache()
    bmed, lmed = verdict
    lines.append(f"# the condition (4096 frames, 65536 uniform pairs of 256 B): batch {bmed:.1f} us, loop without its preparation {lmed:.1f} us, x{lmed / bmed:.2f}: "
                 + ("met" if bmed < lmed else "NOT met"))
    print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    st.close()


if __name__ == "__main__":
    main()
