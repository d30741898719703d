"""Parity tests proper: the shipped libstenos.so (HIP kernels on the MI355X) through its C ABI against
the oracle, the golden vectors generated from the compiled reference, and -- when the prebuilt
oracle/_ref travelled to the box -- the reference library itself.  Bar: bit-exact."""
import hashlib
import json
import os

import numpy as np
import pytest

from _libs import has_error, load_ref, np_ptr, oracle_compress
from stenos_amd.api import load_library
from stenos_amd.datagen import generate

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "manifest.json")) as f:
    MANIFEST = json.load(f)["cases"]


@pytest.fixture(scope="module")
def lib():
    lib = load_library()
    assert lib.stenos_hip_device_count() >= 1, "no HIP device: the GPU tests cannot run"
    return lib


@pytest.fixture(scope="module")
def ctx(lib):
    c = lib.stenos_make_context()
    yield c
    lib.stenos_destroy_context(c)


def gpu_compress(lib, ctx, data, T, level=1, dst_size=None):
    lib.stenos_set_level(ctx, level)
    cap = lib.stenos_bound(data.nbytes) if dst_size is None else dst_size
    out = np.full(cap + 64, 0xA5, dtype=np.uint8)
    r = lib.stenos_compress_generic(ctx, np_ptr(data), T, data.nbytes, np_ptr(out), cap)
    assert (out[cap:] == 0xA5).all(), "wrote past dst_size"
    return r, (out[:r].copy() if not has_error(r) else None)


def gpu_decompress(lib, ctx, frame, T, nbytes):
    out = np.full(nbytes + 64, 0x5A, dtype=np.uint8)
    r = lib.stenos_decompress_generic(ctx, np_ptr(frame), T, frame.nbytes, np_ptr(out), nbytes)
    assert (out[nbytes:] == 0x5A).all(), "wrote past the decompressed size"
    return r, out[:nbytes]


def _golden_cases():
    # every golden case of supported shape (level-1 path: bytesoftype > 1)
    return [e for e in MANIFEST if e["T"] > 1]


@pytest.mark.parametrize("entry", _golden_cases(), ids=lambda e: f"{e['kind']}-T{e['T']}-n{e['n']}")
def test_golden_vectors(lib, ctx, entry):
    """Frames are byte-identical to those of the compiled reference (tests/golden/manifest.json)."""
    data = generate(entry["kind"], entry["T"], entry["n"], entry["seed"])
    for level in (0, 1):
        r, frame = gpu_compress(lib, ctx, data, entry["T"], level)
        assert not has_error(r), hex(r)
        assert r == entry[f"l{level}_size"]
        assert hashlib.sha256(frame.tobytes()).hexdigest() == entry[f"l{level}_sha256"]
    r2, back = gpu_decompress(lib, ctx, frame, entry["T"], data.nbytes)
    assert r2 == data.nbytes
    assert np.array_equal(back, data)


@pytest.mark.parametrize("T", [2, 3, 4, 5, 6, 7, 8, 9, 12, 15, 16, 24, 33, 64])
def test_matrix_against_oracle(lib, ctx, oracle, T):
    """The reference's own test matrix (tests_comp_decomp.cpp:182-211): bytesoftype x distribution x odd
    sizes, plus sizes around the superblock boundary; GPU frames equal the oracle's, and the GPU decodes
    the oracle's frames."""
    per_sb = 131072 // (256 * T) * 256
    sizes = [0, 1, 15, 16, 17, 100, 255, 256, 257, 511, 1280, 4099, per_sb - 1, per_sb, per_sb + 1, 2 * per_sb + 300]
    for kind in ("rand", "same", "sorted", "walk", "dict16", "runs", "burst", "ramp", "mixed", "lzmix"):
        for n in sizes:
            data = generate(kind, T, n, 77 + n)
            r1, ref = oracle_compress(oracle, data, T, 1)
            r2, frame = gpu_compress(lib, ctx, data, T, 1)
            assert r1 == r2, (kind, n, hex(r2))
            assert np.array_equal(ref, frame), (kind, n)
            r3, back = gpu_decompress(lib, ctx, ref, T, data.nbytes)
            assert r3 == data.nbytes and np.array_equal(back, data), (kind, n)


def test_readme_example(lib, ctx):
    data = generate("sorted_i32", 4, 1_000_000, 0)
    r, frame = gpu_compress(lib, ctx, data, 4, 1)
    assert r == 70464
    assert hashlib.sha256(frame.tobytes()).hexdigest() == "1af6d3035454fff7c0b8a23490dba172c14328795010b563283304c831ed0681"
    # one-shot entry points (reference stenos.cpp:1210-1226)
    out = np.zeros(lib.stenos_bound(data.nbytes), dtype=np.uint8)
    assert lib.stenos_compress(np_ptr(data), 4, data.nbytes, np_ptr(out), out.nbytes, 1) == 70464
    back = np.zeros(data.nbytes, dtype=np.uint8)
    assert lib.stenos_decompress(np_ptr(out), 4, 70464, np_ptr(back), back.nbytes) == data.nbytes
    assert np.array_equal(back, data)


@pytest.mark.parametrize("T,kind,n", [(4, "rand12", 5_000_011), (2, "walk", 9_000_001), (8, "sine", 2_000_003), (4, "dict16", 3_000_017),
                                      (4, "rand", 1_000_003), (4, "burst", 4_000_001), (4, "mixed", 3_000_001), (2, "mixed", 5_000_003), (4, "lzmix", 3_000_001), (8, "lzmix", 1_000_001),
                                      (4, "sorted", 2_000_001)])
def test_medium_sizes_against_oracle(lib, ctx, oracle, T, kind, n):
    data = generate(kind, T, n, 42)
    r1, ref = oracle_compress(oracle, data, T, 1)
    r2, frame = gpu_compress(lib, ctx, data, T, 1)
    assert r1 == r2
    assert np.array_equal(ref, frame)
    r3, back = gpu_decompress(lib, ctx, frame, T, data.nbytes)
    assert r3 == data.nbytes and np.array_equal(back, data)


@pytest.mark.parametrize("T", [2, 4, 8])
@pytest.mark.parametrize("kind", ["sine", "walk", "noise_low", "steps", "slopes", "dict16", "cycle130"])
def test_plane_forms_of_round_4(lib, ctx, oracle, T, kind):
    """The decoder's short plane forms and the encoder's run-length rows by quads and passes of noise on
    inputs made of those row kinds (tests/test_emulation_vs_oracle.py asserts with the oracle's counters that they are), a few
    MiB each so that every resident workgroup of the fused kernel gets superblocks; and blocks the mini-LZ took, for both of its
    decoders (dict16: matches of one byte, the two-phase form; cycle130: two bytes, the chain of groups)."""
    if kind == "sine" and T == 2:
        pytest.skip("float data: bytesoftype 4 and 8")
    n = (24 << 20) // T + 77
    data = generate(kind, T, n, 31)
    r1, ref = oracle_compress(oracle, data, T)
    r2, out = gpu_compress(lib, ctx, data, T)
    assert r1 == r2 and np.array_equal(ref, out)
    r3, back = gpu_decompress(lib, ctx, ref, T, data.nbytes)
    assert r3 == data.nbytes and np.array_equal(back, data)


@pytest.mark.parametrize("T,kind,n", [(4, "rand", 300), (4, "walk", 5000), (2, "burst", 70001), (8, "dict16", 3000), (4, "rand12", 32768 + 200)])
def test_shrinking_dst(lib, ctx, oracle, T, kind, n):
    """Compress must succeed when dst_size >= bound, may only fail with an error below it, and never
    writes past dst_size (tests_comp_decomp.cpp:103-121, 163-177).  When it succeeds the frame is the
    oracle's full-capacity frame."""
    data = generate(kind, T, n, 5)
    bound = lib.stenos_bound(data.nbytes)
    _, ref = oracle_compress(oracle, data, T, 1)
    dst_size = bound
    step = max(10, data.nbytes // 10)
    while True:
        r, frame = gpu_compress(lib, ctx, data, T, 1, dst_size)
        if has_error(r):
            assert dst_size < bound
        else:
            assert r <= dst_size and np.array_equal(frame, ref), dst_size
        if dst_size == 0:
            break
        dst_size = max(0, dst_size - step)


def test_exact_superblock_multiples_decode(lib, ctx, oracle):
    """The reference decoder rejects these frames (stenos.cpp:1115-1116, 1131); this library decodes them."""
    for T, nsb in ((4, 1), (4, 3), (2, 2), (8, 5)):
        data = generate("walk", T, nsb * (131072 // T), 9)
        r, frame = gpu_compress(lib, ctx, data, T, 1)
        r1, ref = oracle_compress(oracle, data, T, 1)
        assert r == r1 and np.array_equal(frame, ref)
        r2, back = gpu_decompress(lib, ctx, frame, T, data.nbytes)
        assert r2 == data.nbytes and np.array_equal(back, data)


def test_corrupt_frames_give_errors(lib, ctx):
    data = generate("burst", 4, 100_000, 3)
    r, frame = gpu_compress(lib, ctx, data, 4, 1)
    out = np.zeros(data.nbytes, dtype=np.uint8)
    # truncated frame
    for cut in (r - 1, r // 2, 20, 12, 9):
        assert has_error(lib.stenos_decompress_generic(ctx, np_ptr(frame), 4, cut, np_ptr(out), out.nbytes))
    # unknown superblock code
    bad = frame.copy()
    bad[8] = 9
    assert has_error(lib.stenos_decompress_generic(ctx, np_ptr(bad), 4, r, np_ptr(out), out.nbytes))
    # garbage block stream: must return (an error or garbage), never hang or write out of bounds
    rng = np.random.default_rng(0)
    for _ in range(8):
        bad = frame.copy()
        pos = rng.integers(12, r, size=64)
        bad[pos] = rng.integers(0, 256, size=64, dtype=np.uint8)
        guard = np.full(data.nbytes + 64, 0x5A, dtype=np.uint8)
        lib.stenos_decompress_generic(ctx, np_ptr(bad), 4, r, np_ptr(guard), data.nbytes)
        assert (guard[data.nbytes:] == 0x5A).all()


def test_custom_block_size_and_private_api(lib, oracle):
    """stenos_set_block_size frames (byte 255 + 4-byte size, stenos.cpp:868-874) and the single-superblock
    private API used by stenos::cvector (stenos.cpp:768-804)."""
    c = lib.stenos_make_context()
    assert lib.stenos_set_block_size(c, 2) == 0  # superblock = 256*T*4
    data = generate("walk", 4, 20_000, 1)
    out = np.zeros(lib.stenos_bound(data.nbytes), dtype=np.uint8)
    r = lib.stenos_compress_generic(c, np_ptr(data), 4, data.nbytes, np_ptr(out), out.nbytes)
    assert not has_error(r) and out[0] == 255 and int.from_bytes(out[8:12].tobytes(), "little") == 4096
    back = np.zeros(data.nbytes, dtype=np.uint8)
    assert lib.stenos_decompress_generic(c, np_ptr(out), 4, r, np_ptr(back), back.nbytes) == data.nbytes
    assert np.array_equal(back, data)
    # one superblock through the private API: [code][csize:3][payload] equals the oracle's payload
    blk = data[:4096]
    sb = np.zeros(4096 + 64, dtype=np.uint8)
    r = lib.stenos_private_compress_block(c, np_ptr(blk), 4, 4096, 4096, np_ptr(sb), sb.nbytes)
    ref = np.zeros(8192, dtype=np.uint8)
    rp = oracle.so_block_compress(np_ptr(blk), 4, 4096, np_ptr(ref), ref.nbytes)
    assert r == rp + 4 and sb[0] == 1 and np.array_equal(sb[4:r], ref[:rp])
    assert lib.stenos_private_block_size(np_ptr(sb), r) == r
    back = np.zeros(4096, dtype=np.uint8)
    assert lib.stenos_private_decompress_block(c, np_ptr(sb), 4, 4096, r, np_ptr(back), 4096) == 4096
    assert np.array_equal(back, blk)
    lib.stenos_destroy_context(c)


def test_small_custom_superblocks_exceed_stenos_bound(lib, ref_det):
    """With stenos_set_block_size(ctx, 0) a superblock is one block, so an incompressible frame carries one 4-byte header
    per 256 elements and is larger than stenos_bound() assumes (superblocks of at least 64 KiB, stenos.h:37-42): the
    frame must fit a roomy destination and must equal the reference's."""
    c = lib.stenos_make_context()
    assert lib.stenos_set_block_size(c, 0) == 0
    data = generate("rand", 4, 300_000, 9)
    assert data.nbytes + 4 * (data.nbytes // 1024 + 1) + 12 > lib.stenos_bound(data.nbytes)
    out = np.zeros(2 * data.nbytes, dtype=np.uint8)
    r = lib.stenos_compress_generic(c, np_ptr(data), 4, data.nbytes, np_ptr(out), out.nbytes)
    assert not has_error(r) and r > lib.stenos_bound(data.nbytes)
    back = np.zeros(data.nbytes, dtype=np.uint8)
    assert lib.stenos_decompress_generic(c, np_ptr(out), 4, r, np_ptr(back), back.nbytes) == data.nbytes
    assert np.array_equal(back, data)
    if ref_det is not None:
        rc = ref_det.stenos_make_context()
        ref_det.stenos_set_block_size(rc, 0)
        ref_det.stenos_set_level(rc, 1)
        exp = np.zeros(2 * data.nbytes, dtype=np.uint8)
        r2 = ref_det.stenos_compress_generic(rc, np_ptr(data), 4, data.nbytes, np_ptr(exp), exp.nbytes)
        ref_det.stenos_destroy_context(rc)
        assert r2 == r and np.array_equal(exp[:r], out[:r])
    lib.stenos_destroy_context(c)


@pytest.mark.parametrize("T,kind,n,shift", [(4, "mixed", 30_000_011, None), (2, "walk", 60_000_001, None), (8, "lzmix", 13_000_003, 3), (4, "rand", 26_000_000, None)])
def test_chunked_host_calls(lib, oracle, T, kind, n, shift):
    """Host-pointer calls of 96 MiB and more are cut into chunks of whole superblocks whose uploads overlap the coding and
    the downloads (host_pointer.cpp::compress_chunked / decompress_chunked): same frame as a single pass, tight destinations
    included, and the same bytes back."""
    c = lib.stenos_make_context()
    if shift is not None:
        assert lib.stenos_set_block_size(c, shift) == 0
    data = generate(kind, T, n, 17)
    assert data.nbytes >= 96 << 20
    r, frame = gpu_compress(lib, c, data, T, 1)
    assert not has_error(r)
    if shift is None:
        r1, ref = oracle_compress(oracle, data, T, 1)
        assert r1 == r and np.array_equal(ref, frame)
    else:  # custom superblock size: check the chunk seams against single passes over the pieces
        assert frame[0] == 255
    r3, back = gpu_decompress(lib, c, frame, T, data.nbytes)
    assert r3 == data.nbytes and np.array_equal(back, data)
    # tight destinations: whatever a single pass of the oracle does with the same capacity (the last superblocks
    # meet less room than they may need, stenos.cpp:893-904)
    if shift is None:
        for cap in (r + 4096, r, r - 1, r // 2):
            r4, again = gpu_compress(lib, c, data, T, 1, dst_size=cap)
            r5, exp = oracle_compress(oracle, data, T, 1, dst_size=cap)
            assert has_error(r4) == has_error(r5), cap
            if not has_error(r4):
                assert r4 == r5 and np.array_equal(again, exp), cap
    # truncated and corrupted frames are refused
    assert has_error(lib.stenos_decompress_generic(c, np_ptr(frame), T, r - 1, np_ptr(np.zeros(data.nbytes, dtype=np.uint8)), data.nbytes))
    lib.stenos_destroy_context(c)


@pytest.mark.parametrize("T", [65, 100, 128, 132, 512, 516, 1000, 20001, 65534])
def test_wide_types(lib, oracle, ref_det, T):
    """bytesoftype above 64 (the reference accepts up to 65534, stenos.h:65): kernels_wide.hip runs the block codec with its
    scratch in HBM.  Same frames as the oracle, tight destinations included, and the same bytes back; the compiled
    reference decodes them."""
    c = lib.stenos_make_context()
    bs = 256 * T
    per = (131072 // bs * 256) if bs <= 131072 else 256
    kinds = ["mixed", "walk", "rand", "lzmix", "dict16", "burst"] if T <= 1000 else ["mixed", "walk"]
    for kind in kinds:
        for n in ([100, 256, 2 * per + 300] if T <= 1000 else [2 * 256 + 77]):
            data = generate(kind, T, n, 31 + n)
            r1, ref = oracle_compress(oracle, data, T, 1)
            r2, frame = gpu_compress(lib, c, data, T, 1)
            assert r1 == r2 and np.array_equal(ref, frame), (kind, n)
            r3, back = gpu_decompress(lib, c, frame, T, data.nbytes)
            assert r3 == data.nbytes and np.array_equal(back, data), (kind, n)
            if T <= 1000:
                for cap in (r1, r1 - 1, max(0, r1 - bs // 3)):
                    r4, again = gpu_compress(lib, c, data, T, 1, dst_size=cap)
                    r5, exp = oracle_compress(oracle, data, T, 1, dst_size=cap)
                    assert has_error(r4) == has_error(r5), (kind, n, cap)
                    if not has_error(r4):
                        assert r4 == r5 and np.array_equal(again, exp), (kind, n, cap)
            # (the reference cannot decode exact multiples of the superblock size, and its partial-block encoder overruns
            # its heap buffer from bytesoftype 19 on, block_compress.h:321, 966-968: whole blocks only, decode only)
            if n % 256 == 0 and data.nbytes % (per * T):
                out = np.zeros(data.nbytes + 65536, dtype=np.uint8)
                assert ref_det.stenos_decompress(np_ptr(frame), T, r2, np_ptr(out), data.nbytes) == data.nbytes
                assert np.array_equal(out[: data.nbytes], data), (kind, n)
    lib.stenos_destroy_context(c)


@pytest.mark.parametrize("T,kind,n,seed", [(424, "dict16", 262, 790841817), (424, "dict16", 3 * 256 + 6, 5), (16, "dict16", 5 * 512 + 40, 7), (4, "dict16", 6 * 8192 + 100, 9), (8, "lzmix", 5 * 4096 + 9, 11)])
def test_capacity_rules_with_several_flagged_superblocks(lib, ctx, oracle, T, kind, n, seed):
    """Destinations between the frame the block codec could make and stenos_bound: whether a superblock's block stream is
    accepted depends on the room behind it (block_compress.h:1152-1176, stenos.cpp:424-429), so superblocks are flagged
    for the replay of the reference's capacity rules (pipeline.h resolve_capacity), the first flagged one found with an
    atomic minimum over all wavefronts.  A fuzz run found the case in front (two flagged superblocks, bytesoftype 424) when
    that minimum was not atomic in one build; error or frame, the result must be the oracle's at every capacity."""
    data = generate(kind, T, n, seed)
    bound = lib.stenos_bound(data.nbytes)
    r0, _ = oracle_compress(oracle, data, T, 1)
    caps = sorted({bound, r0, r0 - 1, r0 - 1000, (r0 * 9) // 10, (r0 * 17) // 20, (r0 * 3) // 4, r0 // 2, bound - 7, bound - 5000})
    for cap in caps:
        if cap <= 0:
            continue
        for _ in range(3):  # (a race does not show every time)
            r1, ref = oracle_compress(oracle, data, T, 1, cap)
            r2, frame = gpu_compress(lib, ctx, data, T, 1, cap)
            assert has_error(r1) == has_error(r2), (cap, hex(r1), hex(r2))
            if not has_error(r1):
                assert r1 == r2 and np.array_equal(ref, frame), cap


@pytest.mark.parametrize("T,level", [(72, 2), (100, 3), (300, 5)])
def test_wide_types_through_the_strategy_layer(lib, ref_det, T, level):
    """levels >= 2 use the same block kernels for their BLOCK / BLOCK_ZSTD candidates (stenos.cpp:546-604)."""
    c = lib.stenos_make_context()
    data = generate("mixed", T, 768, 3)  # whole blocks: see test_wide_types
    r, frame = gpu_compress(lib, c, data, T, level)
    assert not has_error(r)
    r3, back = gpu_decompress(lib, c, frame, T, data.nbytes)
    assert r3 == data.nbytes and np.array_equal(back, data)
    exp = np.zeros(lib.stenos_bound(data.nbytes), dtype=np.uint8)
    r2 = ref_det.stenos_compress(np_ptr(data), T, data.nbytes, np_ptr(exp), exp.nbytes, level)
    assert r2 == r and np.array_equal(exp[:r], frame)
    lib.stenos_destroy_context(c)


def test_invalid_bytesoftype_is_refused(lib):
    c = lib.stenos_make_context()
    data = np.zeros(70000, dtype=np.uint8)
    out = np.zeros(lib.stenos_bound(data.nbytes), dtype=np.uint8)
    for T in (0, 65535, 70000):  # stenos.cpp:119-120
        assert has_error(lib.stenos_compress_generic(c, np_ptr(data), T, data.nbytes, np_ptr(out), out.nbytes))
    assert not out.any()
    lib.stenos_destroy_context(c)


def test_time_limited_compression(lib, oracle):
    """stenos_set_max_nanoseconds (stenos.h:141-154): the output depends on the clock, so only properties are checked --
    every frame decodes to the input with the ordinary decoder, the time limit is respected within a margin where it
    can be (the reference's "if possible"), a generous limit compresses like level 1 or better, a hopeless one degrades
    to copies instead of failing."""
    import time

    c = lib.stenos_make_context()
    data = generate("rand12", 4, 48 * 1024 * 1024 + 1000, 3)  # 192 MiB: 16 slices of 12 MiB (+1000 elements: the reference decodes it too)
    nb = data.nbytes
    out = np.zeros(lib.stenos_bound(nb), dtype=np.uint8)
    back = np.zeros(nb, dtype=np.uint8)
    lib.stenos_set_level(c, 1)
    lib.stenos_compress_generic(c, np_ptr(data), 4, nb, np_ptr(out), out.nbytes)  # warm the context's buffers
    sizes = {}
    for label, ns in (("generous", 5_000_000_000), ("tight", 30_000_000), ("hopeless", 1_000)):
        assert lib.stenos_set_max_nanoseconds(c, ns) == 0
        t = time.perf_counter()
        r = lib.stenos_compress_generic(c, np_ptr(data), 4, nb, np_ptr(out), out.nbytes)
        took = time.perf_counter() - t
        assert not has_error(r), (label, hex(r))
        sizes[label] = r
        back[:] = 0
        assert lib.stenos_decompress_generic(c, np_ptr(out), 4, r, np_ptr(back), nb) == nb
        assert np.array_equal(back, data), label
        # ... and with the checkers: the oracle always, the compiled reference when it travelled to the box
        back[:] = 0
        assert oracle.so_decompress(np_ptr(out), 4, r, np_ptr(back), nb, 1) == nb and np.array_equal(back, data), label
        ref = load_ref(det=True)
        if ref is not None and (nb % (128 * 1024)) != 0:  # (the reference refuses exact multiples of the superblock, stenos.cpp:1115-1116)
            back[:] = 0
            assert ref.stenos_decompress(np_ptr(out), 4, r, np_ptr(back), nb) == nb and np.array_equal(back, data), label
        if label == "generous":
            assert took < ns * 1e-9
        if label == "tight":
            assert took < 0.5, took  # copies of 192 MiB take a few tens of milliseconds; far from the untimed path's cost it is not
    assert sizes["generous"] < nb / 2.4  # the block codec's ratio on this data is 2.52
    assert sizes["hopeless"] >= nb  # nothing fits a microsecond: stored
    assert sizes["generous"] <= sizes["tight"] <= sizes["hopeless"]
    # with a higher level allowed and time to spare, the zstd stage on top of the block codec is used where it pays
    lib.stenos_set_level(c, 5)
    lib.stenos_set_max_nanoseconds(c, 60_000_000_000)
    small = generate("sorted_i32", 4, 2_000_000, 0)
    o2 = np.zeros(lib.stenos_bound(small.nbytes), dtype=np.uint8)
    r = lib.stenos_compress_generic(c, np_ptr(small), 4, small.nbytes, np_ptr(o2), o2.nbytes)
    assert not has_error(r) and r < 70464 * 2  # level 1 gives 2 x 70 464 bytes for this input; zstd on top of it is far below
    b2 = np.zeros(small.nbytes, dtype=np.uint8)
    assert lib.stenos_decompress_generic(c, np_ptr(o2), 4, r, np_ptr(b2), small.nbytes) == small.nbytes and np.array_equal(b2, small)
    lib.stenos_destroy_context(c)


def test_reference_library_decodes_gpu_frames(lib, ctx):
    """When the prebuilt reference travelled to the box: it decodes what the GPU encoded, the GPU
    decodes what it encoded, and both encoders agree byte for byte."""
    ref = load_ref(det=True)
    if ref is None:
        pytest.skip("oracle/_ref/*.so not present")
    for T, kind, n in ((4, "rand12", 300_001), (2, "walk", 500_003), (8, "sine", 100_001), (4, "dict16", 200_003)):
        data = generate(kind, T, n, 42)
        r, frame = gpu_compress(lib, ctx, data, T, 1)
        out = np.zeros(ref.stenos_bound(data.nbytes), dtype=np.uint8)
        rr = ref.stenos_compress(np_ptr(data), T, data.nbytes, np_ptr(out), out.nbytes, 1)
        assert rr == r and np.array_equal(out[:rr], frame)
        back = np.zeros(data.nbytes, dtype=np.uint8)
        assert ref.stenos_decompress(np_ptr(frame), T, r, np_ptr(back), back.nbytes) == data.nbytes
        assert np.array_equal(back, data)
        r2, back2 = gpu_decompress(lib, ctx, out[:rr], T, data.nbytes)
        assert r2 == data.nbytes and np.array_equal(back2, data)


@pytest.mark.parametrize("T", [2, 4])
def test_block_pairs_many_seeds(lib, ctx, oracle, T):
    """The int16 / int32 encoder analyses and writes consecutive blocks in pairs, with mini-LZ attempts sequenced in
    between (superblock_codec.h, encode_run): many seeds of data whose blocks differ in the number of constant planes and
    in whether the mini-LZ applies, at sizes with odd and even block counts per run and short last superblocks."""
    per_sb = 131072 // (256 * T) * 256
    for seed in range(24):
        kind = ("mixed", "lzmix", "burst")[seed % 3]
        n = per_sb * (1 + seed % 3) + (seed * 7919) % per_sb + (seed % 5) * 17
        data = generate(kind, T, n, 1000 + seed)
        r1, ref = oracle_compress(oracle, data, T, 1)
        r2, frame = gpu_compress(lib, ctx, data, T, 1)
        assert r1 == r2, (kind, seed, n)
        assert np.array_equal(ref, frame), (kind, seed, n)
        r3, back = gpu_decompress(lib, ctx, frame, T, data.nbytes)
        assert r3 == data.nbytes and np.array_equal(back, data), (kind, seed, n)


def test_int32_kinds_through_the_fused_kernel(lib, ctx, oracle):
    """int32 data of every kind goes through the slot encoder of the fused kernel (slot_codec.h): blocks with two
    non-constant planes in pairs, floats and noise one block per pass; the frames are the oracle's."""
    for kind, n in (("rand12", 700_001), ("sine", 500_003), ("mixed", 600_001), ("lzmix", 400_003), ("rand", 300_001)):
        data = generate(kind, 4, n, 17)
        r1, ref = oracle_compress(oracle, data, 4, 1)
        r2, frame = gpu_compress(lib, ctx, data, 4, 1)
        assert r1 == r2 and np.array_equal(ref, frame), kind


def test_distinct_contexts_on_concurrent_threads(lib, oracle):
    """stenos.h: a context must not be used concurrently, distinct contexts may (stenos.cpp:762-764).  Four threads, a
    context each, different data and levels, host-pointer calls at the same time: every frame equals the frame the same
    call produces alone and decodes to its input."""
    import threading

    jobs = [("rand12", 4, 3_000_001, 1), ("walk", 2, 2_500_003, 1), ("sine", 8, 600_001, 2), ("mixed", 3, 900_001, 1), ("smooth8", 1, 2_000_000, 3), ("sorted_i32", 4, 1_000_000, 1)]
    datas = [generate(k, T, n, 21 + i).view(np.uint8).ravel() for i, (k, T, n, _) in enumerate(jobs)]

    def once(i, out):
        _, T, _, level = jobs[i]
        d = datas[i]
        c = lib.stenos_make_context()
        lib.stenos_set_level(c, level)
        buf = np.zeros(lib.stenos_bound(d.nbytes), dtype=np.uint8)
        frames = []
        for _ in range(3):
            r = lib.stenos_compress_generic(c, np_ptr(d), T, d.nbytes, np_ptr(buf), buf.nbytes)
            assert not has_error(r), hex(r)
            back = np.zeros(d.nbytes, dtype=np.uint8)
            assert lib.stenos_decompress_generic(c, np_ptr(buf), T, r, np_ptr(back), d.nbytes) == d.nbytes
            assert np.array_equal(back, d)
            frames.append(buf[:r].copy())
        lib.stenos_destroy_context(c)
        out[i] = frames

    alone = {}
    for i in range(len(jobs)):
        once(i, alone)
    together, errors = {}, []

    def guarded(i):
        try:
            once(i, together)
        except BaseException as e:  # noqa: BLE001 -- reported by the main thread
            errors.append((i, repr(e)))

    threads = [threading.Thread(target=guarded, args=(i,)) for i in range(len(jobs))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for i in range(len(jobs)):
        for f in together[i]:
            assert np.array_equal(f, alone[i][0]), jobs[i]
