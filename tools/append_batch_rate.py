#!/usr/bin/env python3
"""Bytes appended in place to many frames kept compressed in device memory: stenos_hip_append_batch (index passed in) against the
only way without it -- a loop of stenos_hip_append, one call per frame that grows, each given its frame's slice of a caller-held
frames index.  (The loop leaves the context with the index of the last frame only: the next call over many frames has to walk
every chain again.  That is noted here, not timed.)  Level 1, int32 rand12.  Lines:
  4 096 frames of 64 KiB: 256 B and 4 KiB appended to every frame, and 256 B to every 16th
  8 frames of 128 MiB: 1 MiB each
  1 frame of 1 GiB: 4 KiB and 64 MiB, against stenos_hip_append itself

One process, one context per way (so that what each keeps in device memory can be told apart).  The call works in place, so each
way has its own copy of the store in one slab, which is put back from a third copy before every call, outside the clock.  Every
way is warmed up and checked -- both must leave the same slab, byte for byte --, then timed interleaved (batch, baseline, baseline,
...) over REPS repetitions each; a host clock around calls that end in a synchronise.  Reported: microseconds per call as min /
median, x = baseline over batch (medians), the spread between the two interleaved series of the baseline, which is the noise floor
the difference is to be read against, and the device memory each way's context takes during the line's first call.

  python tools/append_batch_rate.py [--out FILE] [--label TEXT] [--reps N] [--only NAME]
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

KIND, T = "rand12", 4
SB = 131072 // (256 * T) * 256 * T


def free_bytes():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


class Store:
    """m frames of `nbytes` each, every one in a buffer with room for `grow` more bytes; the buffers of a way are one slab"""

    def __init__(self, m, nbytes, grow):
        self.m, self.nbytes = m, nbytes
        self.batch, self.base = Stenos(level=1), Stenos(level=1)
        self.cap = (self.batch.bound(nbytes + grow) + 255) & ~255
        self.orig = torch.zeros(m * self.cap, dtype=torch.uint8, device="cuda")
        src = generate_torch(KIND, T, nbytes // T, 42).view(torch.uint8)
        views = [self.orig[f * self.cap:(f + 1) * self.cap] for f in range(m)]
        self.csizes = []
        step = max(1, min(m, (1 << 30) // nbytes))
        for at in range(0, m, step):  # (the frames differ: the data is rotated by 256 bytes per frame)
            k = min(step, m - at)
            srcs = [torch.roll(src, (at + i) * 256) for i in range(k)]
            res = self.base.compress_batch(srcs, T, views[at:at + k])
            assert all(r < (1 << 63) for r in res)
            self.csizes += res
        del src, srcs
        self.nsb = -(-nbytes // SB)
        p, entries = self.base.frames_index(views, T, self.csizes)
        assert entries == m * (self.nsb + 1)
        self.index = torch.empty(entries, dtype=torch.int64, device="cuda")
        hip = ctypes.CDLL("libamdhip64.so")
        assert hip.hipMemcpy(ctypes.c_void_p(self.index.data_ptr()), ctypes.c_void_p(p), ctypes.c_size_t(entries * 8), 3) == 0
        self.slab = {"batch": self.orig.clone(), "baseline": self.orig.clone()}

    def close(self):
        self.batch.close()
        self.base.close()

    def restore(self, way):
        self.slab[way].copy_(self.orig)
        torch.cuda.synchronize()

    def calls(self, nbytes, every):
        """nbytes of noise of the data's kind appended to every `every`-th frame"""
        m, cap = self.m, self.cap
        grows = [f % every == 0 for f in range(m)]
        gen = torch.Generator(device="cuda")
        gen.manual_seed(nbytes + every)
        src = torch.randint(0, 1 << 12, (sum(grows), nbytes // 4), dtype=torch.int32, device="cuda", generator=gen).view(torch.uint8).reshape(sum(grows), nbytes)
        P, Z = ctypes.c_void_p * m, ctypes.c_size_t * m
        sptr, k = [], 0
        for g in grows:
            sptr.append(src.data_ptr() + k * nbytes if g else None)
            k += g
        fp = {way: P(*[self.slab[way].data_ptr() + f * cap for f in range(m)]) for way in self.slab}
        fz, cz, sp, sz = Z(*self.csizes), Z(*([cap] * m)), P(*sptr), Z(*[nbytes if g else 0 for g in grows])
        res = Z(*([0] * m))
        lib, stream, ip = self.batch.lib, self.batch._stream_ptr(), self.index.data_ptr()
        sizes = {"keepalive": src}

        def batch():
            r = lib.stenos_hip_append_batch(self.batch.ctx, m, T, fp["batch"], fz, cz, sp, sz, res, ip, stream)
            assert r == 0, hex(r)
            sizes["batch"] = list(res)

        def baseline():
            out = []
            base = self.slab["baseline"].data_ptr()
            for f in range(m):
                if not grows[f]:
                    out.append(self.csizes[f])
                    continue
                r = lib.stenos_hip_append(self.base.ctx, base + f * cap, T, self.csizes[f], cap, sptr[f], nbytes, ip + 8 * f * (self.nsb + 1), stream)
                assert r < (1 << 63), hex(r)
                out.append(r)
            sizes["baseline"] = out

        return batch, baseline, sizes


def interleaved(st, fns, reps):
    ts = [[] for _ in fns]
    for _ in range(reps):
        for (way, f), t in zip(fns, ts):
            st.restore(way)
            t0 = time.perf_counter()
            f()
            t.append(time.perf_counter() - t0)
    return [(min(t) * 1e6, statistics.median(t) * 1e6) for t in ts]


def measure(st, name, nbytes, every, reps):
    batch, baseline, sizes = st.calls(nbytes, every)
    held = {}
    for way, fn in (("batch", batch), ("baseline", baseline)):
        st.restore(way)
        before = free_bytes()
        fn()
        held[way] = before - free_bytes()
    assert sizes["batch"] == sizes["baseline"], "the two ways leave frames of different sizes"
    assert torch.equal(st.slab["batch"], st.slab["baseline"]), "the two ways leave different frames"
    grown = sum(1 for f in range(st.m) if f % every == 0)
    (umin, umed), (amin, amed), (bmin, bmed) = interleaved(st, (("batch", batch), ("baseline", baseline), ("baseline", baseline)), reps)
    best, spread = min(amed, bmed), abs(amed - bmed)
    line = (f"{name:52s} {nbytes:9d} bytes to {grown:5d} frames   batch {umin:11.1f} / {umed:11.1f} us   baseline "
            f"{amin:11.1f} / {amed:11.1f} and {bmin:11.1f} / {bmed:11.1f} us   x{best / umed:8.2f}   spread of the baseline series {spread:9.1f} us   device memory "
            f"taken by the line's first call: batch {held['batch'] / 2**20:8.1f} MiB, baseline {held['baseline'] / 2**20:8.1f} MiB")
    print(line, flush=True)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default=None, help="small, large or one")
    a = ap.parse_args()
    lines = [f"# tools/append_batch_rate.py {a.label}".rstrip(),
             f"# {torch.cuda.get_device_name(0)}, level 1, {KIND} T={T}, superblocks of {SB} bytes, index passed in, {a.reps} interleaved repetitions; us per call as min / median;",
             "# batch: stenos_hip_append_batch; baseline: a loop of stenos_hip_append, one call per frame that grows, each given its frame's slice of the caller's frames index,",
             "# two interleaved series; x = baseline (the faster series' median) over batch (median); both ways leave the same frames (checked, byte for byte, whole buffers);",
             "# the store is put back before every call, outside the clock.  Not timed: after the baseline the context holds the index of the last frame only, after the",
             "# batch call that of all new frames"]
    for line in lines:
        print(line, flush=True)
    if a.only in (None, "small"):
        st = Store(4096, 65536, 4096)
        for nbytes, every in ((256, 1), (4096, 1), (256, 16)):
            lines.append(measure(st, "4096 frames of 64 KiB" + (", every 16th grows" if every > 1 else ""), nbytes, every, a.reps))
        st.close()
        del st
        torch.cuda.empty_cache()
    if a.only in (None, "large"):
        st = Store(8, 128 << 20, 1 << 20)
        lines.append(measure(st, "8 frames of 128 MiB", 1 << 20, 1, a.reps))
        st.close()
        del st
        torch.cuda.empty_cache()
    if a.only in (None, "one"):
        st = Store(1, 1 << 30, 64 << 20)
        for nbytes in (4096, 64 << 20):
            lines.append(measure(st, "1 frame of 1 GiB (against stenos_hip_append itself)", nbytes, 1, a.reps))
        st.close()
    lines.append("# device memory: what the way's context takes during the line's first call (the contexts keep their buffers, so a later line of the same store shows "
                 "only the growth)")
    print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
