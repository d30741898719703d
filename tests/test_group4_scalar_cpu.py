"""What the group of four int32 blocks decides with fewer scalar instructions (superblock_codec.h: group4) -- the scan of its
blocks against the planes the wave expects, the transposition of the planes decided once for the group, the mini-LZ gate in lanes
-- in the host emulation of the real headers, as a program of its own (tests/emul_group4_scalar), built plain and with the address
and undefined-behaviour sanitizers.  Streams equal the C oracle's byte for byte; the counters of the emulation say which way every
run went: the groups taken, and the groups whose scan against the expectation was accepted.  Inputs: tests/group4_scalar_inputs.py.
No GPU: it proves the kernel logic, not the shipped binary (tests/test_gpu_group4_scalar.py does that)."""
import os
import subprocess

import numpy as np
import pytest

import group4_inputs as g4in
import group4_scalar_inputs as gsi
from _libs import ROOT, np_ptr


def _oracle_blocks(oracle, data):
    ref = np.zeros(data.nbytes * 2 + 4096, dtype=np.uint8)
    r = oracle.so_block_compress(np_ptr(data), 4, data.nbytes, np_ptr(ref), ref.nbytes)
    return ref[:r]


@pytest.fixture(scope="module")
def runs(oracle):
    """(name, elements, (groups, accepted by the expectation) or None, gate: None / True = it refuses a group / False)"""
    out = [("rand12", gsi.rand12_run(), (8, 7), None)]
    for g, pos in gsi.PLACES:
        for k in (0, 1):
            v = gsi.const_plane(k, g, pos)
            out.append((f"const_plane{k}-g{g}-p{pos}", v, gsi.model(gsi.acts(v)), None))
        for lane in gsi.LANES:
            v = gsi.third_plane(lane, g, pos)
            out.append((f"third_plane-l{lane}-g{g}-p{pos}", v, gsi.model(gsi.acts(v)), None))
    out.append(("plane_pairs-1", gsi.plane_pairs(1), (8, 0), None))  # the expectation is wrong every time
    out.append(("plane_pairs-2", gsi.plane_pairs(2), (8, 4), None))  # wrong once, then right
    out.append(("first_varies", gsi.first_varies(), (8, 7), None))
    # the gate: one group alone (taken or not: exactly the gate's answer), and the block in a run of 32
    for t, (f, d) in enumerate(gsi.GATE_TARGETS):
        for pos in range(4):
            out.append((f"gate-f{f}-d{d}-n4-p{pos}", gsi.gate_run(oracle, 4, pos, f, d), None, gsi.gate_refuses(f, d)))
        for n, g in enumerate(gsi.GROUPS):
            pos = (t + n) % 4
            out.append((f"gate-f{f}-d{d}-g{g}-p{pos}", gsi.gate_run(oracle, gsi.RUN, 4 * g + pos, f, d), None, gsi.gate_refuses(f, d)))
    for kind in ("dict", "low_two"):  # blocks the mini-LZ takes, or nearly takes: few low bytes among the first 80 values
        for pos in range(4):
            v = g4in.rand12(4, 11)
            g4in.change_block(v, pos, kind, 11)
            out.append((f"{kind}-n4-p{pos}", v, None, True))
    return out


def test_the_model_and_the_oracle_split_the_inputs(oracle, runs):
    """The inputs prove something only if they differ: some groups the gate refuses and some it accepts, with blocks on either
    side of each inequality; the oracle itself takes the mini-LZ for some blocks and not for others; and the runs that are meant
    to lose a group lose one in the model."""
    refused = [name for name, _, _, gate in runs if gate is True]
    accepted = [name for name, _, _, gate in runs if gate is False]
    assert len(refused) >= 8 and len(accepted) >= 8, (refused, accepted)
    assert gsi.gate_refuses(342, 3) and not gsi.gate_refuses(341, 3)
    assert gsi.gate_refuses(405, 24) and not gsi.gate_refuses(404, 24) and not gsi.gate_refuses(405, 25) and gsi.gate_refuses(405, 23)
    for f, d in gsi.GATE_TARGETS:
        e = gsi.gate_block(oracle, f, d)
        assert gsi.plain_bytes(oracle, e) == f and gsi.sampled_keys(e) == d
    lz = {}
    for name, v, _, gate in runs:
        if gate is not None and "-n4-" in name:
            size = _oracle_blocks(oracle, v.view(np.uint8)).size
            plain = sum(gsi.plain_bytes(oracle, v[b * gsi.BLOCK:(b + 1) * gsi.BLOCK]) + gsi.HS for b in range(4))
            lz[name] = size != plain  # (a block written by the mini-LZ has another size than its planes)
    assert any(lz.values()) and not all(lz.values()), lz
    for name, _, counts, _ in runs:
        if name.startswith(("const_plane", "third_plane")):
            assert counts[0] < 8 and counts[1] >= 4, (name, counts)


@pytest.fixture(scope="module")
def programs():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "emul_group4_scalar")], stdout=subprocess.DEVNULL)
    return {name: os.path.join(ROOT, "build", name) for name in ("emul_group4_scalar", "emul_group4_scalar_san")}


@pytest.mark.parametrize("name", ["emul_group4_scalar", "emul_group4_scalar_san"])
def test_the_runs_in_the_emulation_plain_and_sanitized(oracle, runs, programs, tmp_path, name):
    """Every run in one call of the stand-alone program: streams equal the oracle's; the groups are taken, and the scan against
    the expected planes accepted, exactly where the model says; a group the gate refuses is not taken and one it accepts is.
    The sanitized build (input, LDS and staging are mallocs of their exact sizes) has to come through without a report."""
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(b"".join(v.tobytes() for _, v, _, _ in runs))
    p = subprocess.run([programs[name], str(src), str(dst)] + [str(v.size // gsi.BLOCK) for _, v, _, _ in runs], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [tuple(int(x) for x in l.split()) for l in p.stdout.split("\n") if l.strip()]
    assert len(lines) == len(runs)
    streams = np.frombuffer(dst.read_bytes(), dtype=np.uint8)
    at = 0
    for (run, v, counts, gate), (size, groups, packed, expected) in zip(runs, lines):
        ref = _oracle_blocks(oracle, v.view(np.uint8))
        assert size == ref.size and np.array_equal(streams[at:at + size], ref), run
        at += size
        n = v.size // gsi.BLOCK
        assert packed <= groups, (run, groups, packed)  # (a scan can be accepted and its group still refused: the gate comes later)
        if counts is not None:
            assert (groups, expected) == counts, (run, groups, expected, counts)
        if gate is True:
            assert groups < n // 4, (run, groups)
        if gate is False:  # (the first group of a run has no expectation, every other one finds it right)
            assert groups == n // 4 and expected == groups - 1, (run, groups, expected)
        if run in ("rand12", "first_varies"):
            assert packed == groups, (run, groups, packed)
    assert at == streams.size


def test_the_sanitized_build_is_one(programs):
    """(a build without the sanitizers' runtime would pass the test above for nothing)"""
    out = subprocess.run(["nm", programs["emul_group4_scalar_san"]], capture_output=True, text=True, check=True).stdout
    assert "__asan_init" in out and "__ubsan_handle" in out
    assert "__asan_init" not in subprocess.run(["nm", programs["emul_group4_scalar"]], capture_output=True, text=True, check=True).stdout
