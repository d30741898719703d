#!/usr/bin/env python3
"""Many small device-resident arrays: a loop of single calls (stenos_hip_compress / stenos_hip_decompress) against one batch
call (stenos_hip_compress_batch / stenos_hip_decompress_batch), level 1, in GB/s of input bytes.  One process, one warm-up
call of each kind before anything is timed; call time is a host clock around calls that end in a synchronise (both entry
points wait for their result).  Items are slices of one ~256 MiB array; the loop is timed over its first LOOP_ITEMS items at
most (its rate does not depend on how many follow).  The last row is one 1 GiB item: batch against the single call, which
has the fused encoder the batch lacks.  Crossover (profiles/batch_rate.txt, int32): compression is faster in a batch up to items
of 64 MiB (759 GB/s against 447 for the loop) and faster through single calls from 256 MiB (1 716 against 770); decompression
is never slower in a batch (at par from 256 MiB).

  python tools/batch_rate.py [--out FILE] [--label TEXT]
  python tools/batch_rate.py --profile      4096 x 64 KiB int32 batches in each direction (for rocprofv3 --kernel-trace --stats)
  python tools/batch_rate.py --walk         the chain walk of a frame of k superblocks: one lane against the parallel walk
                                            (needs the test build, tests/hooks/libstenos_hooks.so: its switch picks the walk)
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from stenos_amd.api import ERR_BASE, Stenos  # noqa: E402
from stenos_amd.datagen import generate_torch  # noqa: E402

TOTAL = 256 << 20
LOOP_ITEMS = 512
CASES = (("rand12", 4), ("walk", 2), ("sine", 8))
SIZES = (4 << 10, 64 << 10, 1 << 20, 16 << 20)


class Batch:
    """ctypes arrays of one batch, built once: the timed region is the library call alone"""

    def __init__(self, st, T, srcs, sizes, dsts, dst_sizes):
        n = len(srcs)
        P, Z = ctypes.c_void_p * n, ctypes.c_size_t * n
        self.st, self.T, self.n = st, T, n
        self.srcs, self.sizes, self.dsts, self.dst_sizes = P(*srcs), Z(*sizes), P(*dsts), Z(*dst_sizes)
        self.res = Z()

    def run(self, fn):
        r = fn(self.st.ctx, self.n, self.T, self.srcs, self.sizes, self.dsts, self.dst_sizes, self.res, self.st._stream_ptr())
        assert r == 0, hex(r)
        return list(self.res)


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return statistics.median(ts)


def setup(st, kind, T, size, total):
    n = max(1, total // size)
    src = generate_torch(kind, T, n * size // T, 42)
    cap = st.bound(size)
    frames = torch.empty(n * cap, dtype=torch.uint8, device="cuda")
    back = torch.empty_like(src)
    s0, f0, b0 = src.data_ptr(), frames.data_ptr(), back.data_ptr()
    enc = Batch(st, T, [s0 + i * size for i in range(n)], [size] * n, [f0 + i * cap for i in range(n)], [cap] * n)
    csizes = enc.run(st.lib.stenos_hip_compress_batch)
    assert all(c < ERR_BASE for c in csizes)
    dec = Batch(st, T, [f0 + i * cap for i in range(n)], csizes, [b0 + i * size for i in range(n)], [size] * n)
    assert dec.run(st.lib.stenos_hip_decompress_batch) == [size] * n
    assert torch.equal(back, src)
    return n, (src, frames, back), enc, dec, csizes


def row(st, kind, T, size):
    lib, ctx, stream = st.lib, st.ctx, st._stream_ptr()
    n, keep, enc, dec, csizes = setup(st, kind, T, size, TOTAL)
    m = min(n, LOOP_ITEMS)

    def loop_c():
        for i in range(m):
            assert lib.stenos_hip_compress(ctx, enc.srcs[i], T, size, enc.dsts[i], enc.dst_sizes[i], stream) == csizes[i]

    def loop_d():
        for i in range(m):
            assert lib.stenos_hip_decompress(ctx, dec.srcs[i], T, csizes[i], dec.dsts[i], size, None, stream) == size

    loop_c(), loop_d()  # (warm-up)
    tcl, tdl = timed(loop_c, 3), timed(loop_d, 3)
    tcb, tdb = timed(lambda: enc.run(lib.stenos_hip_compress_batch), 5), timed(lambda: dec.run(lib.stenos_hip_decompress_batch), 5)
    cl, cb, dl, db = m * size / tcl / 1e9, n * size / tcb / 1e9, m * size / tdl / 1e9, n * size / tdb / 1e9
    return (f"{kind:7s} T={T} {size >> 10:6d} KiB x {n:6d}  ratio {n * size / sum(csizes):6.3f}   compress loop {cl:8.2f}  batch {cb:8.2f} GB/s  x{cb / cl:7.1f}"
            f"   decompress loop {dl:8.2f}  batch {db:8.2f} GB/s  x{db / dl:7.1f}")


def large_row(st):
    lib, ctx, stream = st.lib, st.ctx, st._stream_ptr()
    size = 1 << 30
    n, keep, enc, dec, csizes = setup(st, "rand12", 4, size, size)

    def one_c():
        assert lib.stenos_hip_compress(ctx, enc.srcs[0], 4, size, enc.dsts[0], enc.dst_sizes[0], stream) == csizes[0]

    def one_d():
        assert lib.stenos_hip_decompress(ctx, dec.srcs[0], 4, csizes[0], dec.dsts[0], size, None, stream) == size

    one_c(), one_d()
    tc, td = timed(one_c, 5), timed(one_d, 5)
    tcb, tdb = timed(lambda: enc.run(lib.stenos_hip_compress_batch), 5), timed(lambda: dec.run(lib.stenos_hip_decompress_batch), 5)
    return (f"rand12  T=4 1 GiB x 1 item         compress single {size / tc / 1e9:8.2f}  batch {size / tcb / 1e9:8.2f} GB/s  x{tc / tcb:5.2f}"
            f"   decompress single {size / td / 1e9:8.2f}  batch {size / tdb / 1e9:8.2f} GB/s  x{td / tdb:5.2f}")


def walk_rows():
    """Decode time of a single call on a frame of k superblocks (int32) that comes without an index: the serial walk by one lane
    against the parallel walk.  In a decode batch every item's serial walk runs at the same time on a lane of its own, while the
    parallel walk is one launch per item (batch_host.cpp, kBatchSerialWalkMax)."""
    from stenos_amd.api import load_library

    lib = load_library(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "hooks", "libstenos_hooks.so"))
    st = Stenos(level=1, lib=lib)
    lines = []
    for k in (8, 16, 32, 64, 128, 256, 1024):
        src = generate_torch("rand12", 4, k * (128 << 10) // 4, 42)
        frame = torch.empty(st.bound(src.numel()), dtype=torch.uint8, device="cuda")
        c = st.compress(src, 4, frame)
        back = torch.empty_like(src)
        t = {}
        for serial in (1, 0):
            lib.stenos_hip_test_walk(st.ctx, serial)
            st.decompress(frame, 4, c, back)
            t[serial] = timed(lambda: st.decompress(frame, 4, c, back), 20)
            assert torch.equal(back, src)
        lib.stenos_hip_test_walk(st.ctx, 0)
        lines.append(f"walk  {k:5d} superblocks  decode with the serial walk {t[1] * 1e6:8.1f} us   with the parallel walk {t[0] * 1e6:8.1f} us")
        print(lines[-1], flush=True)
    st.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--label", default="")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--walk", action="store_true")
    a = ap.parse_args()
    if a.walk:
        lines = walk_rows()
        if a.out:
            with open(a.out, "a") as f:
                f.write("\n".join(lines) + "\n")
        return
    st = Stenos(level=1)
    if a.profile:
        setup(st, "rand12", 4, 64 << 10, 4096 * (64 << 10))  # (a warm-up batch in each direction, then one more of each)
        setup(st, "rand12", 4, 64 << 10, 4096 * (64 << 10))
        print("profile run: 4096 x 64 KiB int32 rand12, two batches each way")
        return
    lines = [f"# tools/batch_rate.py {a.label}".rstrip(),
             f"# {torch.cuda.get_device_name(0)}, level 1, ~{TOTAL >> 20} MiB per batch, loop timed over <= {LOOP_ITEMS} items, GB/s of input bytes;"
             " the reference's CPU path on this host's 16-CPU share: 10-13 GB/s (README)"]
    for line in lines:
        print(line, flush=True)
    for kind, T in CASES:
        for size in SIZES + ((64 << 20, 256 << 20) if kind == "rand12" else ()):
            lines.append(row(st, kind, T, size))
            print(lines[-1], flush=True)
            torch.cuda.empty_cache()
    lines.append(large_row(st))
    print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    st.close()


if __name__ == "__main__":
    main()
