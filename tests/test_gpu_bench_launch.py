"""bench.py as the driver starts it, and the collectives of the sharded form on real backends.

* `python bench.py --gpus N --full` WITHOUT an outer torch.distributed.run: the script starts its ranks itself as a child process
  (nothing that has touched the GPU ever execs) and relays rank 0's line.  One GPU here: STENOS_BENCH_ONE_DEVICE=1 puts every
  rank on cuda:0 and moves the collectives to gloo.  With 2 ranks and with 4: this pool lets a job have six processes on a
  card at once, the test runner being one of them, so the 8-way partition, its segment table and its empty ranges run on the
  CPU instead (tests/test_sharded_cpu.py, world size 8 over gloo).
* gather_frames / decompress_sharded with the "nccl" backend (RCCL), world size 1, on cuda:0: RCCL loads and the
  device-tensor collectives and point-to-point calls of stenos_amd/sharded.py execute.
"""
import json
import os
import subprocess
import sys
import textwrap

import pytest

from _libs import ROOT

pytestmark = pytest.mark.gpu


def _bench(gpus, gib):
    env = dict(os.environ, STENOS_BENCH_ONE_DEVICE="1", HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="2")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(gpus), "--gib", str(gib), "--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline"]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.parametrize("gpus,gib", [(2, 0.25), (4, 0.125)])
def test_bench_starts_its_own_ranks(gpus, gib):
    out = _bench(gpus, gib)
    assert out["n_gpus"] == gpus and out["scaling"] == "weak" and out["value"] > 0
    ex = out["sharded_exchange"]
    assert ex.get("sharded_roundtrip_ok") is True, ex
    assert ex["backend"] == "gloo" and ex["gather_bytes_to_rank0"] > 0


NCCL_WORKER = textwrap.dedent("""
    import os, sys, torch, torch.distributed as dist
    sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests"))
    from stenos_amd.api import Stenos
    from stenos_amd.datagen import generate_torch
    from stenos_amd.sharded import compress_sharded, decompress_sharded
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1)
    assert dist.get_backend() == "nccl"
    T = 4
    src = generate_torch("rand12", T, (24 << 20) // T + 333, 42, device="cuda:0")
    st = Stenos(1)
    def compress(chunk):
        dst = torch.empty(st.bound(chunk.numel()), dtype=torch.uint8, device="cuda:0")
        return dst[:st.compress(chunk, T, dst)]
    t = torch.ones(4, device="cuda:0"); dist.all_reduce(t); assert float(t.sum()) == 4.0   # RCCL runs a collective on device memory
    frame = compress_sharded(compress, src, T)
    assert frame.is_cuda and torch.equal(frame, compress(src)), "sharded frame differs from the single-GPU frame"
    index = st.frame_index(frame, T, frame.numel())
    def decompress(local, nbytes):
        out = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
        assert st.decompress(local, T, local.numel(), out) == nbytes
        return out
    whole, o0, o1 = decompress_sharded(decompress, frame, index, src.numel(), T, "cuda:0", gather_output=True)
    assert (o0, o1) == (0, src.numel()) and torch.equal(whole, src)
    dist.barrier(); dist.destroy_process_group()
    print("NCCL_OK")
""")


def test_sharded_collectives_on_rccl(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(NCCL_WORKER.format(root=ROOT))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29533", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1", "--master-addr", "127.0.0.1", "--master-port", "29533", str(script)]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    assert "NCCL_OK" in p.stdout


def _plain_run(out_dir):
    env = dict(os.environ, OMP_NUM_THREADS="2")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "STENOS_BENCH_ONE_DEVICE"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--gib", "0.25", "--steps", "3", "--warmup", "1", "--dump-outputs", str(out_dir)]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_is_the_headline_and_dumps_the_last_step(tmp_path):
    """Without --full: the timed steps and the line, nothing beside them; --dump-outputs writes the last step's frame and
    decoded array (float32 / float64, bounded), the same values run after run."""
    import numpy as np

    out = _plain_run(tmp_path / "a")
    assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0 and out["value"] > 0
    assert out["unit"] == "GB/s" and out["higher_is_better"] is True and out["dtype"] == "u8" and out["metric"].startswith("encode+decode GB/s")
    assert abs(out["compression_ratio"] - 2.52) < 0.01
    for k in ("cpu_baseline", "full_entropy", "other_configs", "parity_bytes", "host_pointer", "decode_indexed_gbps", "sharded_exchange"):
        assert k not in out, k
    assert "device_copy" not in out["roofline"]

    names = ("compressed_size", "frame_head", "frame_sample", "frame_chunk_sums", "decoded_sample", "decoded_chunk_sums")
    a = {nm: np.load(tmp_path / "a" / f"{nm}.npy") for nm in names}
    assert sorted(f.name for f in (tmp_path / "a").iterdir()) == sorted(f"{nm}.npy" for nm in names)
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(f.stat().st_size for f in (tmp_path / "a").iterdir()) <= 64 << 20
    n = (1 << 28) // 4
    csize = int(a["compressed_size"][0])
    assert abs(n * 4 / csize - out["compression_ratio"]) < 1e-3
    assert a["frame_chunk_sums"].shape == ((csize + (1 << 20) - 1) >> 20, 2)
    assert a["frame_head"].size == 64 << 10 and a["frame_sample"].size == 1 << 21
    pos = np.sort(np.random.default_rng(1234).integers(0, csize, size=1 << 21, dtype=np.int64))
    head = pos < (64 << 10)
    assert np.array_equal(a["frame_sample"][head], a["frame_head"][pos[head]])
    assert a["frame_chunk_sums"][:, 0].sum() >= a["frame_head"].sum()
    # the decoded elements are the input: rand12 = splitmix64(42) & 0xFFF at the sampled positions
    pos = np.sort(np.random.default_rng(1235).integers(0, n, size=1 << 21, dtype=np.int64)).astype(np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(42) + (pos + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        want = (z ^ (z >> np.uint64(31))) & np.uint64(0xFFF)
    assert np.array_equal(a["decoded_sample"], want.astype(np.float64))
    assert a["decoded_chunk_sums"].shape == (n >> 20,) and 0 < a["decoded_chunk_sums"].sum() < n * 4096

    _plain_run(tmp_path / "b")  # same arguments, same outputs
    for nm in names:
        assert np.array_equal(a[nm], np.load(tmp_path / "b" / f"{nm}.npy")), nm
