#!/usr/bin/env python3
"""Bytes appended to the array of one large frame kept compressed in device memory: stenos_hip_append (in place, index passed in)
against the only way without it -- stenos_hip_decompress of the whole frame into a scratch tensor with room for the new bytes, a
device copy of the new bytes behind it, stenos_hip_compress of the concatenation back into the frame's buffer.  Level 1; one frame
of 1 GiB int32 rand12 (8 192 superblocks); 4 KiB, 1 MiB, 64 MiB and 1 GiB appended, each to an array that ends on a superblock
boundary (r = 0: nothing is decoded or staged) and to one that ends half a superblock earlier (r = sb / 2: the last superblock is
decoded, stitched and encoded again).

One process, one context per way (so that what each keeps in device memory can be told apart); every way is warmed up and checked
-- both must leave the same frame, byte for byte --, then timed interleaved (append, baseline, baseline, ...) over REPS repetitions
each; a host clock around calls that end in a synchronise.  Both ways change their buffer, so before every timed call the buffer
is put back (outside the clock): the append's 8 header bytes and the bytes from the header of its last superblock on, the
baseline's whole frame.  Reported: microseconds per call as min / median, x = baseline over append (medians), the spread between
the two interleaved series of the baseline, which is the noise floor the difference is to be read against, and the extra device
memory of both ways (what the context holds after the calls, plus the baseline's scratch tensor).

  python tools/append_rate.py [--out FILE] [--label TEXT] [--reps N]
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

KIND, T, TOTAL = "rand12", 4, 1 << 30
SB = 131072 // (256 * T) * 256 * T
APPENDS = (4096, 1 << 20, 64 << 20, 1 << 30)


def free_bytes():
    torch.cuda.synchronize()
    torch.cuda.empty_cache()  # (what torch has freed and kept is not held by either way)
    return torch.cuda.mem_get_info()[0]


class Setup:
    """the array of `total` bytes (the head of one long sequence, so that what is appended continues it), its frame in two
    buffers with room for the largest append, and an index of the caller's own"""

    def __init__(self, src, total):
        self.ap, self.base = Stenos(level=1), Stenos(level=1)
        self.src, self.total = src, total
        cap = self.ap.bound(total + max(APPENDS))
        self.frame_ap = torch.empty(cap, dtype=torch.uint8, device="cuda")
        self.frame_base = torch.empty(cap, dtype=torch.uint8, device="cuda")
        self.csize = self.base.compress(src[:total], T, self.frame_base)
        self.orig = self.frame_base[:self.csize].clone()
        self.frame_ap[:self.csize] = self.orig
        n = ctypes.c_size_t(0)
        p = self.base.lib.stenos_hip_frame_index(self.base.ctx, self.frame_base.data_ptr(), T, self.csize, ctypes.byref(n), self.base._stream_ptr())
        self.nsb = -(-total // SB)
        assert p and n.value == self.nsb
        self.index = torch.empty(self.nsb + 1, dtype=torch.int64, device="cuda")
        hip = ctypes.CDLL("libamdhip64.so")
        assert hip.hipMemcpy(ctypes.c_void_p(self.index.data_ptr()), ctypes.c_void_p(p), ctypes.c_size_t((self.nsb + 1) * 8), 3) == 0
        self.p = int(self.index[total // SB].item())  # where the append's new stream starts
        self.scratch = None

    def calls(self, n):
        b = self.src[self.total:self.total + n]
        lib, stream = self.ap.lib, self.ap._stream_ptr()
        ip = self.index.data_ptr()
        sizes = {}

        def restore_append():
            self.frame_ap[:8] = self.orig[:8]
            self.frame_ap[self.p:self.csize] = self.orig[self.p:]
            torch.cuda.synchronize()

        def restore_baseline():
            self.frame_base[:self.csize] = self.orig
            torch.cuda.synchronize()

        def append():
            sizes["append"] = r = lib.stenos_hip_append(self.ap.ctx, self.frame_ap.data_ptr(), T, self.csize, self.frame_ap.numel(), b.data_ptr(), n, ip, stream)
            assert r < (1 << 63), hex(r)

        def baseline():
            if self.scratch is None or self.scratch.numel() < self.total + n:
                self.scratch = None
                self.scratch = torch.empty(self.total + n, dtype=torch.uint8, device="cuda")
            fb = self.frame_base.data_ptr()
            assert lib.stenos_hip_decompress(self.base.ctx, fb, T, self.csize, self.scratch.data_ptr(), self.total, ip, stream) == self.total
            self.scratch[self.total:self.total + n].copy_(b)
            sizes["baseline"] = r = lib.stenos_hip_compress(self.base.ctx, self.scratch.data_ptr(), T, self.total + n, fb, self.frame_base.numel(), stream)
            assert r < (1 << 63), hex(r)

        return (append, restore_append), (baseline, restore_baseline), sizes


def interleaved(pairs, reps):
    ts = [[] for _ in pairs]
    for _ in range(reps):
        for (f, restore), t in zip(pairs, ts):
            restore()
            t0 = time.perf_counter()
            f()
            t.append(time.perf_counter() - t0)
    return [(min(t) * 1e6, statistics.median(t) * 1e6) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="")
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    src = generate_torch(KIND, T, (TOTAL + max(APPENDS)) // T, 42)
    lines = [f"# tools/append_rate.py {a.label}".rstrip(),
             f"# {torch.cuda.get_device_name(0)}, level 1, index passed in, {a.reps} interleaved repetitions; us per call as min / median;",
             "# append: stenos_hip_append in place; baseline: stenos_hip_decompress into a scratch tensor, the new bytes copied behind it, stenos_hip_compress of the",
             "# concatenation back into the frame's buffer, two interleaved series; x = baseline (the faster series' median) over append (median); both ways leave the",
             "# same frame (checked); r: bytes of the array behind its last whole superblock (0: nothing decoded or staged; sb / 2: the last superblock is stitched)"]
    for line in lines:
        print(line, flush=True)
    for r in (0, SB // 2):
        total = TOTAL - (SB - r) % SB
        su = Setup(src, total)
        head = f"{KIND} T={T}, one frame of {total} bytes, ratio {total / su.csize:.3f}, {su.nsb} superblocks of {SB} bytes, r = {total % SB}"
        lines.append(head)
        print(head, flush=True)
        mem = {}
        for n in APPENDS:
            (append, restore_a), (baseline, restore_b), sizes = su.calls(n)
            for name, fn, restore in (("append", append, restore_a), ("baseline", baseline, restore_b)):
                restore()
                before = free_bytes()
                fn()
                mem[name] = mem.get(name, 0) + before - free_bytes()
            assert sizes["append"] == sizes["baseline"], sizes
            assert torch.equal(su.frame_ap[:sizes["append"]], su.frame_base[:sizes["append"]]), "the two ways leave different frames"
            (umin, umed), (amin, amed), (bmin, bmed) = interleaved(((append, restore_a), (baseline, restore_b), (baseline, restore_b)), a.reps)
            best, spread = min(amed, bmed), abs(amed - bmed)
            line = (f"append {n:10d} B   append {umin:10.1f} / {umed:10.1f} us   baseline {amin:10.1f} / {amed:10.1f} and {bmin:10.1f} / {bmed:10.1f} us   x{best / umed:7.2f}"
                    f"   spread of the baseline series {spread:8.1f} us   extra device memory so far: append {mem['append'] / 2**20:7.1f} MiB, baseline {mem['baseline'] / 2**20:7.1f} MiB")
            lines.append(line)
            print(line, flush=True)
        su.ap.close()
        su.base.close()
        del su
        torch.cuda.empty_cache()
    lines.append("# extra device memory: what the way's context (and torch, for the baseline's scratch tensor of the array's size + the appended bytes) holds after the line's "
                 "first call, summed over the lines so far; the append's grows with the appended bytes, never with the array")
    print(lines[-1], flush=True)
    lines.append("# (the second block's contexts are made after the first block's were destroyed: the runtime serves their first buffers from memory it already holds, so that "
                 "block's first lines read low by what the first block's contexts had; quote the first block for memory)")
    print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
