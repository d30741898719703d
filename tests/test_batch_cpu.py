"""CPU-side checks of the batch entry points (include/stenos_hip.h: stenos_hip_compress_batch, stenos_hip_decompress_batch,
stenos_hip_batch_workspace_bytes): declared, exported and bound; loud failure without a device; workspace planning; and the
build properties of their kernels (csrc/batch_kernels.hip, csrc/batch_decode_kernels.hip)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from _libs import ROOT
from stenos_amd.api import load_library

NAMES = ("stenos_hip_compress_batch", "stenos_hip_decompress_batch", "stenos_hip_batch_workspace_bytes")
E = lambda k: (1 << 64) - k  # noqa: E731


@pytest.fixture(scope="module")
def lib():
    so = os.path.join(ROOT, "stenos_amd", "lib", "libstenos.so")
    if not os.path.exists(so):
        import __graft_entry__

        __graft_entry__.build()
    return load_library()


def test_declared_exported_and_bound(lib):
    text = open(os.path.join(ROOT, "include", "stenos_hip.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "stenos_amd", "lib", "libstenos.so")], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in NAMES:
        assert re.search(r"STENOS_EXPORT[^;(]*\b" + name + r"\s*\(", text), name
        assert name in exported, name
        assert name in lib._stenos_symbols, name


def _arrays(n, fill):
    P, Z = ctypes.c_void_p * n, ctypes.c_size_t * n
    return P(*[0x1000 * (k + 1) for k in range(n)]), Z(*[4096] * n), P(*[0x100000 * (k + 1) for k in range(n)]), Z(*[8192] * n), Z(*[fill] * n)


def test_no_gpu_means_loud_failure(lib):
    """Without a device both batch calls fail as a whole, touch neither results[] nor any buffer (the device pointers here are
    made up: a call that went on would fault)."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    ctx = lib.stenos_make_context()
    try:
        for fn in (lib.stenos_hip_compress_batch, lib.stenos_hip_decompress_batch):
            srcs, sizes, dsts, dsizes, res = _arrays(3, 0x5A5A)
            assert fn(ctx, 3, 4, srcs, sizes, dsts, dsizes, res, None) == E(5)  # STENOS_ERROR_INVALID_INSTRUCTION_SET
            assert list(res) == [0x5A5A] * 3
            assert fn(ctx, 0, 4, srcs, sizes, dsts, dsizes, res, None) == 0  # n == 0: nothing to do
    finally:
        lib.stenos_destroy_context(ctx)


def _ws(lib, T, sizes):
    Z = ctypes.c_size_t * max(len(sizes), 1)
    return lib.stenos_hip_batch_workspace_bytes(T, len(sizes), Z(*sizes))


@pytest.mark.parametrize("T", [1, 2, 4, 8, 12, 64])
def test_workspace_covers_the_input_and_grows_with_items(lib, T):
    rng = np.random.default_rng(T)
    sizes = []
    prev = _ws(lib, T, sizes)
    for _ in range(40):
        sizes.append(int(rng.integers(0, 1 << 20)) if rng.random() < 0.9 else 0)
        w = _ws(lib, T, sizes)
        assert w >= sum(sizes) and w >= prev, (T, sizes[-1], w, prev)
        prev = w
    assert _ws(lib, 0, sizes) == 0 and _ws(lib, 65, sizes) == 0


# ---- build properties of the batch kernels ----------------------------------------------------------------------------

def _usage(source, flags):
    cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-c", os.path.join(ROOT, "stenos_amd", "csrc", source),
           "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"] + flags
    err = subprocess.run(cmd, capture_output=True, text=True, timeout=900).stderr
    res, cur = {}, None
    for line in err.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = res.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[bytes/lane\]| \[waves/SIMD\])?: (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return res


def _one(res, key):
    hits = [v for k, v in res.items() if key in k]
    assert len(hits) == 1, (key, [k for k in res if key in k])
    return hits[0]


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_batch_decoder_has_no_divergent_branch():
    keys = [f"decode_frames_batchILj{T}E" for T in (2, 4, 8, 0)]
    p = subprocess.run([os.path.join(ROOT, "tools", "divergent_branches.sh"), "batch_decode_kernels.hip"] + keys, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert [l for l in lines if l.startswith("== ")] == [f"== {k}" for k in keys], p.stdout[-1500:]
    assert [l for l in lines if not l.startswith("== ")] == [], "divergent branches:\n" + p.stdout[-1500:]


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_batch_kernel_resources():
    """The batch decoders use no scratch memory; the batch block encoders have at least the occupancy of encode_blocks."""
    dec = _usage("batch_decode_kernels.hip", ["-mllvm", "-structurizecfg-skip-uniform-regions=1"])
    for T in (2, 4, 8, 0):
        d = _one(dec, f"decode_frames_batchILj{T}E")
        assert d["ScratchSize"] == 0 and d["VGPRs Spill"] == 0, (T, d)
    enc = _usage("batch_kernels.hip", ["-DWV_PREDICATE_BRANCHES"])
    ref = _usage("kernels.hip", ["-DWV_PREDICATE_BRANCHES"])
    for T in (2, 4, 8, 0):
        got, want = _one(enc, f"encode_blocks_batchILj{T}E")["Occupancy"], _one(ref, f"encode_blocksILj{T}E")["Occupancy"]
        assert got >= want, (T, got, want)
    # the names the budget test of the single-frame kernels keys on stay unique (tests/test_build_properties.py)
    for name in list(enc) + list(dec):
        assert "encode_superblocksILj" not in name and "decode_superblocksILj" not in name, name


def test_batch_decoder_body_is_the_single_decoders():
    """decode_body.h (decode_frames_batch) keeps a copy of decode_superblocks' steps (decode_kernels.hip, whose listing is held
    fixed): from the header checks to the last status, the two are the same text."""
    def region(name):
        text = open(os.path.join(ROOT, "stenos_amd", "csrc", name)).read()
        a = text.index("if (p > a.size || a.size - p < 4)")
        b = text.index("status_or(a.status, DECODE_STATUS_INVALID);\n", text.index("else if (code >= 2 && code <= 5)")) + len("status_or(a.status, DECODE_STATUS_INVALID);")
        return [line.strip() for line in text[a:b].splitlines()]

    single, batch = region("decode_kernels.hip"), region("decode_body.h")
    assert len(single) > 25 and single == batch
