"""ctypes binding of libstenos.so: the frozen C ABI (include/stenos.h, mirroring the reference's
stenos/stenos.h:115-301) plus the device-pointer entry points (include/stenos_hip.h)."""
from __future__ import annotations

import ctypes
import os
import subprocess
from ctypes import c_int, c_size_t, c_uint64, c_void_p

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("STENOS_LIB_PATH") or os.path.join(HERE, "lib", "libstenos.so")  # override: experiments with other builds
ERR_BASE = (1 << 64) - 100

ERROR_NAMES = {
    (1 << 64) - 1: "STENOS_ERROR_UNDEFINED",
    (1 << 64) - 2: "STENOS_ERROR_SRC_OVERFLOW",
    (1 << 64) - 3: "STENOS_ERROR_ALLOC",
    (1 << 64) - 4: "STENOS_ERROR_INVALID_INPUT",
    (1 << 64) - 5: "STENOS_ERROR_INVALID_INSTRUCTION_SET",
    (1 << 64) - 6: "STENOS_ERROR_DST_OVERFLOW",
    (1 << 64) - 7: "STENOS_ERROR_INVALID_BYTESOFTYPE",
    (1 << 64) - 8: "STENOS_ERROR_ZSTD_INTERNAL",
    (1 << 64) - 9: "STENOS_ERROR_INVALID_PARAMETER",
}


class StenosError(RuntimeError):
    def __init__(self, code: int):
        super().__init__(ERROR_NAMES.get(code, f"stenos error {code:#x}"))
        self.code = code


def build_library() -> str:
    """Compile libstenos.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    subprocess.check_call(["make", "-C", os.path.join(HERE, "csrc")])
    return LIB_PATH


def load_library(path: str = LIB_PATH) -> ctypes.CDLL:
    if not os.path.exists(path):
        raise ImportError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` (no CPU fallback exists)")
    # PyTorch-ROCm ships its own libamdhip64 and asks for it under a name the loader does not match with an
    # already loaded /opt/rocm copy; two HIP runtimes in one process cannot both open the GPU.  Loading torch
    # first makes libstenos.so resolve to the copy torch uses.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = ctypes.CDLL(path)
    sz, vp = c_size_t, c_void_p
    sigs = {
        "stenos_make_context": (vp, []),
        "stenos_destroy_context": (None, [vp]),
        "stenos_reset_context": (None, [vp]),
        "stenos_set_level": (sz, [vp, c_int]),
        "stenos_set_threads": (sz, [vp, c_int]),
        "stenos_set_max_nanoseconds": (sz, [vp, c_uint64]),
        "stenos_set_block_size": (sz, [vp, sz]),
        "stenos_memory_footprint": (sz, [vp]),
        "stenos_has_error": (c_int, [sz]),
        "stenos_bound": (sz, [sz]),
        "stenos_compress_generic": (sz, [vp, vp, sz, sz, vp, sz]),
        "stenos_decompress_generic": (sz, [vp, vp, sz, sz, vp, sz]),
        "stenos_compress": (sz, [vp, sz, sz, vp, sz, c_int]),
        "stenos_decompress": (sz, [vp, sz, sz, vp, sz]),
        "stenos_get_info": (sz, [vp, sz, sz, vp]),
        "stenos_make_timer": (vp, []),
        "stenos_destroy_timer": (None, [vp]),
        "stenos_tick": (None, [vp]),
        "stenos_tock": (c_uint64, [vp]),
        "stenos_private_compress_block": (sz, [vp, vp, sz, sz, sz, vp, sz]),
        "stenos_private_decompress_block": (sz, [vp, vp, sz, sz, sz, vp, sz]),
        "stenos_private_block_size": (sz, [vp, sz]),
        "stenos_private_block_csize": (sz, [vp]),
        "stenos_private_create_compression_header": (sz, [sz, sz, vp, sz]),
        "stenos_hip_device_count": (c_int, []),
        "stenos_hip_last_devices": (c_int, [vp]),
        "stenos_hip_set_devices": (None, [vp, c_int]),
        "stenos_hip_stage_ms": (c_int, [vp, ctypes.POINTER(ctypes.c_double), c_int, c_int]),
        "stenos_hip_fused_fallbacks": (c_int, [vp]),
        "stenos_hip_workspace_bytes": (sz, [sz, sz]),
        "stenos_hip_compress": (sz, [vp, vp, sz, sz, vp, sz, vp]),
        "stenos_hip_compress_async": (sz, [vp, vp, sz, sz, vp, sz, vp]),
        "stenos_hip_finish": (sz, [vp]),
        "stenos_hip_last_index": (vp, [vp, ctypes.POINTER(sz)]),
        "stenos_hip_frame_index": (vp, [vp, vp, sz, sz, ctypes.POINTER(sz), vp]),
        "stenos_hip_decompress": (sz, [vp, vp, sz, sz, vp, sz, vp, vp]),
        "stenos_hip_decompress_async": (sz, [vp, vp, sz, sz, vp, sz, vp, vp]),
        "stenos_hip_shuffle": (sz, [vp, sz, sz, vp, vp]),
        "stenos_hip_unshuffle": (sz, [vp, sz, sz, vp, vp]),
        "stenos_hip_delta": (sz, [vp, vp, sz, vp]),
        "stenos_hip_delta_inv": (sz, [vp, vp, sz, vp]),
        "stenos_hip_compress_batch": (sz, [vp, sz, sz, ctypes.POINTER(vp), ctypes.POINTER(sz), ctypes.POINTER(vp), ctypes.POINTER(sz), ctypes.POINTER(sz), vp]),
        "stenos_hip_decompress_batch": (sz, [vp, sz, sz, ctypes.POINTER(vp), ctypes.POINTER(sz), ctypes.POINTER(vp), ctypes.POINTER(sz), ctypes.POINTER(sz), vp]),
        "stenos_hip_decompress_ranges": (sz, [vp, vp, sz, sz, sz, ctypes.POINTER(c_uint64), ctypes.POINTER(c_uint64), ctypes.POINTER(vp), vp, vp]),
        "stenos_hip_gather_rows": (sz, [vp, vp, sz, sz, sz, sz, vp, vp, sz, vp, vp]),
        "stenos_hip_gather_ranges": (sz, [vp, vp, sz, sz, sz, vp, vp, vp, sz, vp, vp, vp]),
        "stenos_hip_gather_rows_batch": (sz, [vp, sz, sz, ctypes.POINTER(vp), ctypes.POINTER(sz), sz, sz, vp, vp, vp, sz, vp, vp]),
        "stenos_hip_frames_index": (vp, [vp, sz, sz, ctypes.POINTER(vp), ctypes.POINTER(sz), ctypes.POINTER(sz), vp]),
        "stenos_hip_update_rows": (sz, [vp, vp, sz, sz, sz, sz, vp, vp, sz, vp, sz, vp, vp]),
        "stenos_hip_update_rows_batch": (sz, [vp, sz, sz, ctypes.POINTER(vp), ctypes.POINTER(sz), sz, sz, vp, vp, vp, sz, ctypes.POINTER(vp), ctypes.POINTER(sz),
                                         ctypes.POINTER(sz), vp, vp]),
        "stenos_hip_last_frames_index": (vp, [vp, ctypes.POINTER(sz)]),
        "stenos_hip_append": (sz, [vp, vp, sz, sz, sz, vp, sz, vp, vp]),
        "stenos_hip_append_batch": (sz, [vp, sz, sz, ctypes.POINTER(vp), ctypes.POINTER(sz), ctypes.POINTER(sz), ctypes.POINTER(vp), ctypes.POINTER(sz),
                                    ctypes.POINTER(sz), vp, vp]),
        "stenos_hip_batch_workspace_bytes": (sz, [sz, sz, ctypes.POINTER(sz)]),
        "stenos_hip_set_profiling": (None, [vp, c_int]),
        "stenos_hip_kernel_ms": (ctypes.c_double, [vp, c_int]),
    }
    for name, (res, args) in sigs.items():
        fn = getattr(lib, name)  # AttributeError if the library does not export the symbol
        fn.restype = res
        fn.argtypes = args
    lib._stenos_symbols = tuple(sigs)
    # the test suite's own build (tests/hooks/Makefile, -DSTENOS_TEST_HOOKS) has three switches more; libstenos.so has none
    hooks = {"stenos_hip_test_lanes": (None, [vp, c_int, c_int]), "stenos_hip_test_walk": (c_int, [vp, c_int]), "stenos_hip_test_fused_timeouts": (None, [vp, c_int])}
    lib._stenos_test_hooks = all(hasattr(lib, name) for name in hooks)
    if lib._stenos_test_hooks:
        for name, (res, args) in hooks.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
    return lib


class Stenos:
    """A compression context on torch CUDA tensors (device-resident path) -- plumbing for tests and bench."""

    def __init__(self, level: int = 1, lib: ctypes.CDLL | None = None):
        self.lib = lib or load_library()
        self.ctx = self.lib.stenos_make_context()
        if not self.ctx:
            raise MemoryError("stenos_make_context failed")
        self.lib.stenos_set_level(self.ctx, level)

    def close(self):
        if self.ctx:
            self.lib.stenos_destroy_context(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _check(r: int) -> int:
        if r >= ERR_BASE:
            raise StenosError(r)
        return r

    def bound(self, nbytes: int) -> int:
        return self.lib.stenos_bound(nbytes)

    @staticmethod
    def _stream_ptr():
        import torch

        return torch.cuda.current_stream().cuda_stream

    def compress(self, src, bytesoftype: int, dst, wait: bool = True) -> int:
        """src, dst: contiguous uint8 CUDA tensors.  Returns the frame size (0 when wait=False)."""
        fn = self.lib.stenos_hip_compress if wait else self.lib.stenos_hip_compress_async
        return self._check(fn(self.ctx, src.data_ptr(), bytesoftype, src.numel(), dst.data_ptr(), dst.numel(), self._stream_ptr()))

    def finish(self) -> int:
        return self._check(self.lib.stenos_hip_finish(self.ctx))

    def set_profiling(self, enabled: bool = True):
        self.lib.stenos_hip_set_profiling(self.ctx, 1 if enabled else 0)

    def kernel_ms(self, which: int) -> float:
        """elapsed ms of the last encode_blocks (0) / decode_superblocks (1) launch"""
        return self.lib.stenos_hip_kernel_ms(self.ctx, which)

    def stage_ms(self, reset: bool = True):
        """wall milliseconds per stage of the levels >= 2 strategy layer since the last reset (include/stenos_hip.h)"""
        names = ("gpu_pass", "estimates", "wait_block_streams", "zstd", "layout", "wait_upload", "inflate", "device_decode")
        buf = (ctypes.c_double * len(names))()
        self.lib.stenos_hip_stage_ms(self.ctx, buf, len(names), 1 if reset else 0)
        return {k: round(buf[i], 3) for i, k in enumerate(names)}

    def last_index(self):
        n = c_size_t(0)
        p = self.lib.stenos_hip_last_index(self.ctx, ctypes.byref(n))
        return p, n.value

    def frame_index(self, frame, bytesoftype: int, csize: int):
        """Offsets of the superblock headers of any frame on the device (nsb + 1 of them, the last one is the end) as a
        list of ints; raises for a malformed or truncated frame."""
        import torch

        n = c_size_t(0)
        p = self.lib.stenos_hip_frame_index(self.ctx, frame.data_ptr(), bytesoftype, csize, ctypes.byref(n), self._stream_ptr())
        if not p:
            raise StenosError((1 << 64) - 4)
        host = torch.empty(n.value + 1, dtype=torch.int64)
        hip = ctypes.CDLL("libamdhip64.so")
        if hip.hipMemcpy(c_void_p(host.data_ptr()), c_void_p(p), c_size_t((n.value + 1) * 8), 2) != 0:
            raise StenosError((1 << 64) - 1)
        return host.tolist()

    def decompress(self, frame, bytesoftype: int, csize: int, dst, index_ptr: int | None = None, wait: bool = True) -> int:
        fn = self.lib.stenos_hip_decompress if wait else self.lib.stenos_hip_decompress_async
        return self._check(fn(self.ctx, frame.data_ptr(), bytesoftype, csize, dst.data_ptr(), dst.numel(), index_ptr, self._stream_ptr()))

    def _batch(self, fn, srcs, bytesoftype: int, sizes, dsts) -> list[int]:
        n = len(srcs)
        if len(sizes) != n or len(dsts) != n:
            raise ValueError("srcs, sizes and dsts must have the same length")
        P, Z = c_void_p * n, c_size_t * n
        res = Z()
        r = fn(self.ctx, n, bytesoftype, P(*[t.data_ptr() for t in srcs]), Z(*sizes), P(*[t.data_ptr() for t in dsts]), Z(*[t.numel() for t in dsts]), res,
               self._stream_ptr())
        self._check(r)
        return list(res)

    def compress_batch(self, srcs, bytesoftype: int, dsts) -> list[int]:
        """srcs, dsts: lists of contiguous uint8 CUDA tensors, one frame per item in one pass of kernels.  Returns every item's
        frame size or error code (ERROR_NAMES); raises StenosError only when the call as a whole fails."""
        return self._batch(self.lib.stenos_hip_compress_batch, srcs, bytesoftype, [t.numel() for t in srcs], dsts)

    def decompress_batch(self, frames, bytesoftype: int, csizes, dsts) -> list[int]:
        """frames[i][:csizes[i]] -> dsts[i] for every item in one pass of kernels.  Returns every item's decompressed size or
        error code; raises StenosError only when the call as a whole fails."""
        return self._batch(self.lib.stenos_hip_decompress_batch, frames, bytesoftype, list(csizes), dsts)

    def decompress_ranges(self, frame, bytesoftype: int, csize: int, ranges, dsts, index_ptr: int | None = None) -> int:
        """Bytes [offset, offset + length) of the ORIGINAL array, for every (offset, length) of `ranges`, out of frame[:csize] into
        dsts[i][:length] in one call (dsts: contiguous uint8 CUDA tensors that do not overlap, or raw device addresses).  Only the
        superblocks a range touches are read.  index_ptr: as for decompress; the pointer of frame_index / last_index may be
        passed to any number of these calls.  Returns the bytes delivered."""
        n = len(ranges)
        if len(dsts) != n:
            raise ValueError("ranges and dsts must have the same length")
        U, P = c_uint64 * n, c_void_p * n
        offs, lens = U(*[int(o) for o, _ in ranges]), U(*[int(l) for _, l in ranges])
        ptrs = P(*[d if isinstance(d, int) else d.data_ptr() for d in dsts])
        return self._check(self.lib.stenos_hip_decompress_ranges(self.ctx, frame.data_ptr(), bytesoftype, csize, n, offs, lens, ptrs, index_ptr, self._stream_ptr()))

    def decompress_range(self, frame, bytesoftype: int, csize: int, offset: int, length: int, dst, index_ptr: int | None = None) -> int:
        """One range: bytes [offset, offset + length) of the original array -> dst[:length]."""
        return self.decompress_ranges(frame, bytesoftype, csize, [(offset, length)], [dst], index_ptr)

    def gather_rows(self, frame, bytesoftype: int, csize: int, row_bytes: int, rows, out, index_ptr: int | None = None, dst_stride: int | None = None) -> int:
        """Row rows[i] of the ORIGINAL array (bytes [r * row_bytes, (r + 1) * row_bytes)) out of frame[:csize] into
        out[i * dst_stride : i * dst_stride + row_bytes], for every i, in one call.  rows: a contiguous int64 or uint64 CUDA tensor
        (it stays on the device and may have been written by earlier work on the current stream; a negative int64 is a huge
        unsigned value and therefore an invalid row).  out: a uint8 CUDA tensor or a raw device address.  dst_stride defaults to
        row_bytes.  index_ptr: as for decompress_ranges.  Returns the bytes delivered; an invalid row raises
        STENOS_ERROR_INVALID_PARAMETER with its slot untouched."""
        import torch

        if not rows.is_cuda or rows.dtype not in (torch.int64, torch.uint64) or not rows.is_contiguous():
            raise ValueError("rows must be a contiguous int64 or uint64 CUDA tensor")
        stride = row_bytes if dst_stride is None else dst_stride
        dst = out if isinstance(out, int) else out.data_ptr()
        return self._check(self.lib.stenos_hip_gather_rows(self.ctx, frame.data_ptr(), bytesoftype, csize, row_bytes, rows.numel(), rows.data_ptr(), dst, stride, index_ptr,
                                                           self._stream_ptr()))

    def gather_ranges(self, frame, bytesoftype: int, csize: int, offsets, lengths, out, out_offsets=None, index_ptr: int | None = None,
                      out_size: int | None = None) -> int:
        """Bytes [offsets[i], offsets[i] + lengths[i]) of the ORIGINAL array out of frame[:csize], packed back to back into out:
        range i begins at D[i], the exclusive prefix sum of the lengths.  offsets, lengths: contiguous int64 or uint64 CUDA
        tensors of equal length n (they stay on the device and may have been written by earlier work on the current stream; a
        negative int64 is a huge unsigned value and therefore invalid).  out: a uint8 CUDA tensor, or a raw device address
        together with out_size; out_size (the real capacity, it sizes the call's tables) defaults to out.numel().  out_offsets:
        an optional int64 or uint64 CUDA tensor of n + 1 that receives D, D[n] being the total.  index_ptr: as for gather_rows.
        Returns the bytes delivered; an invalid range raises STENOS_ERROR_INVALID_PARAMETER, lengths that sum to more than
        out_size raise STENOS_ERROR_DST_OVERFLOW, both with out untouched."""
        import torch

        for t, name in ((offsets, "offsets"), (lengths, "lengths")):
            if not t.is_cuda or t.dtype not in (torch.int64, torch.uint64) or not t.is_contiguous():
                raise ValueError(f"{name} must be a contiguous int64 or uint64 CUDA tensor")
        n = offsets.numel()
        if lengths.numel() != n:
            raise ValueError("offsets and lengths must have the same length")
        if out_offsets is not None and (not out_offsets.is_cuda or out_offsets.dtype not in (torch.int64, torch.uint64) or not out_offsets.is_contiguous()
                                        or out_offsets.numel() != n + 1):
            raise ValueError("out_offsets must be a contiguous int64 or uint64 CUDA tensor of n + 1")
        if isinstance(out, int):
            if out_size is None:
                raise ValueError("a raw address needs out_size")
            dst = out
        else:
            dst = out.data_ptr()
            out_size = out.numel() if out_size is None else out_size
        return self._check(self.lib.stenos_hip_gather_ranges(self.ctx, frame.data_ptr(), bytesoftype, csize, n, offsets.data_ptr(), lengths.data_ptr(), dst, out_size,
                                                             None if out_offsets is None else out_offsets.data_ptr(), index_ptr, self._stream_ptr()))

    def frames_index(self, frames, bytesoftype: int, csizes):
        """The superblock header offsets of all `frames` (frames[f][:csizes[f]]) in one device array, as gather_rows_batch takes
        them: (device pointer, entries).  Frame f's superblocks + 1 offsets start at entry f + the superblocks of the frames in
        front of it.  The pointer is the context's own index: valid until the next call on this context that is not a
        gather_rows_batch given it.  Raises for a malformed or truncated frame."""
        m = len(frames)
        if len(csizes) != m:
            raise ValueError("frames and csizes must have the same length")
        P, Z = c_void_p * m, c_size_t * m
        n = c_size_t(0)
        p = self.lib.stenos_hip_frames_index(self.ctx, m, bytesoftype, P(*[t.data_ptr() for t in frames]), Z(*csizes), ctypes.byref(n), self._stream_ptr())
        if not p:
            raise StenosError((1 << 64) - 4)
        return p, n.value

    def gather_rows_batch(self, frames, bytesoftype: int, csizes, row_bytes: int, frame_ids, rows, out, index_ptr: int | None = None,
                          dst_stride: int | None = None) -> int:
        """gather_rows over many frames in one call: row rows[i] of the ORIGINAL array of frames[frame_ids[i]] goes to
        out[i * dst_stride : i * dst_stride + row_bytes].  frames: a list of uint8 CUDA tensors (frames[f][:csizes[f]], the same
        tensor may be listed twice); frame_ids, rows: contiguous int64 or uint64 CUDA tensors of the same length, which stay on
        the device and may have been written by earlier work on the current stream.  index_ptr: the pointer of frames_index (None:
        every chain is walked first).  Returns the bytes delivered; an invalid pair (a frame number >= len(frames), a row beyond
        that frame's array) raises STENOS_ERROR_INVALID_PARAMETER with its slot untouched."""
        import torch

        for t, name in ((frame_ids, "frame_ids"), (rows, "rows")):
            if not t.is_cuda or t.dtype not in (torch.int64, torch.uint64) or not t.is_contiguous():
                raise ValueError(f"{name} must be a contiguous int64 or uint64 CUDA tensor")
        if frame_ids.numel() != rows.numel():
            raise ValueError("frame_ids and rows must have the same length")
        m = len(frames)
        if len(csizes) != m:
            raise ValueError("frames and csizes must have the same length")
        P, Z = c_void_p * m, c_size_t * m
        stride = row_bytes if dst_stride is None else dst_stride
        dst = out if isinstance(out, int) else out.data_ptr()
        return self._check(self.lib.stenos_hip_gather_rows_batch(self.ctx, m, bytesoftype, P(*[t.data_ptr() for t in frames]), Z(*csizes), row_bytes, rows.numel(),
                                                                 frame_ids.data_ptr(), rows.data_ptr(), dst, stride, index_ptr, self._stream_ptr()))

    def update_rows(self, frame, bytesoftype: int, csize: int, row_bytes: int, rows, src, out, index_ptr: int | None = None, src_stride: int | None = None) -> int:
        """The frame of the ORIGINAL array with row rows[i] (bytes [r * row_bytes, (r + 1) * row_bytes)) replaced by
        src[i * src_stride : i * src_stride + row_bytes], for every i: frame[:csize] -> out, a complete frame, in one call; the input
        frame is not modified.  rows: as for gather_rows (on the device, ordered on the current stream, as are the source rows).
        src: a uint8 CUDA tensor or a raw device address; out: a uint8 CUDA tensor that overlaps neither.  src_stride defaults to
        row_bytes.  index_ptr: as for gather_rows; afterwards last_index() is the index of the new frame.  Returns the new frame's
        size; an invalid row, a frame that does not fit or damage in a touched superblock raises with `out` untouched.  Where row
        numbers repeat, each piece of the row holds the bytes of one of its sources."""
        import torch

        n = 0 if rows is None else rows.numel()
        if n and (not rows.is_cuda or rows.dtype not in (torch.int64, torch.uint64) or not rows.is_contiguous()):
            raise ValueError("rows must be a contiguous int64 or uint64 CUDA tensor")
        stride = row_bytes if src_stride is None else src_stride
        s = src if isinstance(src, int) or src is None else src.data_ptr()
        return self._check(self.lib.stenos_hip_update_rows(self.ctx, frame.data_ptr(), bytesoftype, csize, row_bytes, n, rows.data_ptr() if n else None, s, stride,
                                                           out.data_ptr(), out.numel(), index_ptr, self._stream_ptr()))

    def update_rows_batch(self, frames, bytesoftype: int, csizes, row_bytes: int, frame_ids, rows, src, outs, index_ptr: int | None = None,
                          src_stride: int | None = None) -> list[int]:
        """update_rows over many frames in one call: row rows[i] of the ORIGINAL array of frames[frame_ids[i]] is replaced by
        src[i * src_stride : i * src_stride + row_bytes]; outs[f] receives a complete frame for every listed frame (a byte copy
        where no pair names it).  frames, outs: lists of uint8 CUDA tensors (frames[f][:csizes[f]]; the same input tensor may be
        listed twice; an entry of outs may be a (device address, capacity) tuple); frame_ids, rows: as for gather_rows_batch, on
        the device, ordered on the current stream, as are the source rows.  All frames of non-empty arrays must have one superblock
        size.  index_ptr: the pointer of frames_index or last_frames_index (None: every chain is walked first); afterwards
        last_frames_index() is the index of the new frames.  Returns the new sizes.  All or nothing: an invalid pair, a frame that
        does not fit its output or damage in a touched superblock raises with every output untouched."""
        import torch

        n = 0 if rows is None else rows.numel()
        if n:
            for t, name in ((frame_ids, "frame_ids"), (rows, "rows")):
                if not t.is_cuda or t.dtype not in (torch.int64, torch.uint64) or not t.is_contiguous():
                    raise ValueError(f"{name} must be a contiguous int64 or uint64 CUDA tensor")
            if frame_ids.numel() != n:
                raise ValueError("frame_ids and rows must have the same length")
        m = len(frames)
        if len(csizes) != m or len(outs) != m:
            raise ValueError("frames, csizes and outs must have the same length")
        P, Z = c_void_p * m, c_size_t * m
        stride = row_bytes if src_stride is None else src_stride
        s = src if isinstance(src, int) or src is None else src.data_ptr()
        optr = [o[0] if isinstance(o, tuple) else o.data_ptr() for o in outs]
        ocap = [o[1] if isinstance(o, tuple) else o.numel() for o in outs]
        results = Z(*([0] * m))
        self._check(self.lib.stenos_hip_update_rows_batch(self.ctx, m, bytesoftype, P(*[t.data_ptr() for t in frames]), Z(*csizes), row_bytes, n,
                                                               frame_ids.data_ptr() if n else None, rows.data_ptr() if n else None, s, stride, P(*optr), Z(*ocap),
                                                               results, index_ptr, self._stream_ptr()))
        return list(results)

    def append(self, frame, bytesoftype: int, csize: int, src, index_ptr: int | None = None) -> int:
        """Append IN PLACE: frame[:csize] is the frame of an array A, frame.numel() the capacity of its buffer; afterwards `frame`
        holds the frame of A followed by the bytes of src, and its size is returned.  frame: a uint8 CUDA tensor; src: a uint8
        CUDA tensor, or a (device address, length) tuple, that does not overlap it; its bytes may have been written by earlier
        work on the current stream.  Superblocks in front of A's last whole one stay where and what they are; size the buffer with
        bound(final array size).  index_ptr: as for gather_rows (it may be last_index()); afterwards last_index() is the index of
        the new frame.  A frame that does not fit, a refused index or damage in the last superblock raises with `frame` untouched."""
        s, n = src if isinstance(src, tuple) else (src.data_ptr(), src.numel())
        return self._check(self.lib.stenos_hip_append(self.ctx, frame.data_ptr(), bytesoftype, csize, frame.numel(), s if n else None, n, index_ptr, self._stream_ptr()))

    def append_batch(self, frames, bytesoftype: int, csizes, srcs, index_ptr: int | None = None) -> list[int]:
        """append over many frames in one call, IN PLACE: frames[f][:csizes[f]] is the frame of an array A_f; afterwards frames[f]
        holds the frame of A_f followed by the bytes of srcs[f].  frames: uint8 CUDA tensors (the capacity of a buffer is its
        numel()) or (device address, capacity) tuples; srcs: uint8 CUDA tensors, (device address, length) tuples, or None for
        nothing; their bytes may have been written by earlier work on the current stream.  No two buffers may overlap, and no
        source may overlap a buffer.  All frames of non-empty arrays must have one superblock size.  index_ptr: the pointer of
        frames_index or last_frames_index (None: every chain is walked first); afterwards last_frames_index() is the index of the
        new frames.  Returns the new sizes.  All or nothing: a frame that does not fit its buffer, a refused index entry or damage
        in a partial last superblock of any frame raises StenosError with every buffer untouched."""
        m = len(frames)
        if len(csizes) != m or len(srcs) != m:
            raise ValueError("frames, csizes and srcs must have the same length")
        P, Z = c_void_p * m, c_size_t * m
        fptr = [t[0] if isinstance(t, tuple) else t.data_ptr() for t in frames]
        fcap = [t[1] if isinstance(t, tuple) else t.numel() for t in frames]
        pairs = [(None, 0) if s is None else s if isinstance(s, tuple) else (s.data_ptr(), s.numel()) for s in srcs]
        results = Z(*([0] * m))
        self._check(self.lib.stenos_hip_append_batch(self.ctx, m, bytesoftype, P(*fptr), Z(*csizes), Z(*fcap), P(*[p if n else None for p, n in pairs]),
                                                     Z(*[n for _, n in pairs]), results, index_ptr, self._stream_ptr()))
        return list(results)

    def last_frames_index(self):
        """(device pointer, entries) of the many-frame index the last frames_index, update_rows_batch or append_batch on this
        context left, in the layout of frames_index; (None, 0) when the last call left none."""
        n = c_size_t(0)
        p = self.lib.stenos_hip_last_frames_index(self.ctx, ctypes.byref(n))
        return (p, n.value) if p else (None, 0)
