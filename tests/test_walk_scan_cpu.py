"""Phase A of the parallel header walk as walk_speculate runs it (stenos_amd/csrc/walk.h: scan_lane, scan_deferred -- several steps'
loads at once, a filter on two bytes, the candidates' exact test put off to a list) against scan_window16, the form it had
and that tests/emul still replays: the same set of roots and the same count on every window.  tests/emul_walk_scan is a program of
its own; it runs here as a child process, plain and built with the address and undefined-behaviour sanitizers (its frames are
mallocs of exactly their size).  Its inputs: uniform bytes; bytes mostly 0..8 (look-alikes by the hundred: more than 64 roots, more
candidates than the list holds); planted headers that point at, in front of and behind the window's and the frame's end; frames
that end inside, at and behind the window; windows in a frame's last 0..40 bytes; superblock sizes with top byte 0, 1 and 2 and an
odd one behind a 12-byte frame header; windows cut from the frames under tests/golden.  And for every (code byte, top size byte)
pair: the filter passes exactly what it promises, which is all that plausible() accepts."""
import base64
import json
import os
import re
import subprocess
import zlib

import pytest

import streamgen as sg
from _libs import ROOT


@pytest.fixture(scope="module")
def programs():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "emul_walk_scan")], stdout=subprocess.DEVNULL)
    return {name: os.path.join(ROOT, "build", name) for name in ("emul_walk_scan", "emul_walk_scan_san")}


@pytest.fixture(scope="module")
def golden_frames(tmp_path_factory):
    """the larger frames of tests/golden as files: [path, offset of the first superblock header, superblock size] ..."""
    d = tmp_path_factory.mktemp("walk_scan_frames")
    frames = []
    for c in json.load(open(os.path.join(ROOT, "tests", "golden", "level_frames.json")))["cases"]:
        frames.append((c["T"], base64.b64decode(c["frame_b64"])))
    for c in json.load(open(os.path.join(ROOT, "tests", "golden", "timed_frames.json")))["cases"]:
        frames.append((c["T"], zlib.decompress(base64.b64decode(c["frame_zb64"]))))
    frames.sort(key=lambda f: -len(f[1]))
    args = []
    for i, (T, frame) in enumerate(frames[:12]):
        if frame[0] == 0xFF:
            first, sb = 12, int.from_bytes(frame[8:12], "little")
        else:
            first, sb = 8, sg.base_superblock(T) << frame[0]
        path = d / f"frame{i}.bin"
        path.write_bytes(frame)
        args += [str(path), str(first), str(sb)]
    assert len(args) >= 3 * 4
    return args


def _run(program, args):
    p = subprocess.run([program] + args, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    seen = {k: int(v) for k, v in re.findall(r"(\w+) (\d+)", p.stdout.strip().splitlines()[-1])}
    assert seen["failures"] == 0
    return seen


@pytest.mark.parametrize("name", ["emul_walk_scan", "emul_walk_scan_san"])
def test_scan_in_groups_finds_the_roots_of_scan_window16(programs, golden_frames, name):
    seen = _run(programs[name], golden_frames)
    print(seen)
    # the inputs reached what they are there for
    assert seen["windows"] > 10000 and seen["roots"] > 10000
    assert seen["gave_up"] > 50, "no window with more than 64 roots"
    assert seen["list_full"] > 50, "no window with more candidates than the list holds"
    assert seen["with_groups"] > 3000 and seen["bytewise"] > 3000
    assert seen["target_is_size"] > 100 and seen["at_size_minus_4"] > 100 and seen["hop_is_window"] > 100
    # (16 positions x 13 superblock sizes; every pair was compared, these passed)
    assert seen["filter_passed"] > 16 * 13 * 8


def test_the_sanitized_build_is_one(programs):
    """(a build without the sanitizers' runtime would pass the test above for nothing)"""
    out = subprocess.run(["nm", programs["emul_walk_scan_san"]], capture_output=True, text=True, check=True).stdout
    assert "__asan_init" in out and "__ubsan_handle" in out
    assert "__asan_init" not in subprocess.run(["nm", programs["emul_walk_scan"]], capture_output=True, text=True, check=True).stdout
