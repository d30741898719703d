"""Inputs for what the group of four int32 blocks decides in fewer scalar instructions (superblock_codec.h: group4): the scan of
its four blocks against the planes the wave expects (slot_codec.h: scan_expected_group4), the planes' transposition decided once
for the group (write_slots_group4) and the mini-LZ gate evaluated in lanes (block_codec.h: lz_precheck_passes_lanes).  Shared by
test_group4_scalar_cpu.py and test_gpu_group4_scalar.py; the generators of group4_inputs.py are reused.

A run is what one wave of the fused encoder takes from a superblock: 32 blocks, eight groups.  A condition is put on ONE block of
the run, at every position 0..3 of its group and in the first, a middle and the last group.  model() follows the encoder's
control flow on the planes that vary in each block and says how many groups a run takes and how many of them are accepted by the
scan against the expectation; it knows nothing of the mini-LZ, so it is used for the runs whose blocks the gate never stops.
"""
import numpy as np

import group4_inputs as g4in
from stenos_amd.datagen import splitmix64

BLOCK = g4in.BLOCK
RUN = 32                # blocks of a wave's run
GROUPS = (0, 3, 7)      # the first, a middle and the last group of a run
LANES = (0, 17, 63)     # lanes of the one element that makes a third plane vary
PLACES = [(g, pos) for g in GROUPS for pos in range(4)]
BS, HS = 1024, 2        # bytes of a block of 32-bit elements, and of its header
# the elements whose low bytes the group counts (lz_distinct_keys_group4: values 4l and 4l + 1 of lanes 0..19)
SAMPLED = np.array([4 * l + k for l in range(20) for k in (0, 1)])


def acts(data: np.ndarray) -> list:
    """per block: bit k set when plane k is not constant"""
    b = data.view(np.uint8).reshape(-1, BLOCK, 4)
    varies = (b != b[:, :1, :]).any(axis=1)
    return [int(sum(int(v) << k for k, v in enumerate(row))) for row in varies]


def model(act: list) -> tuple:
    """(groups taken, groups accepted by the scan against the expected planes) of a run that begins without an expectation, for
    blocks the mini-LZ gate lets through (encode_blocks_to, 32-bit elements: groups of four, else passes of one or two blocks)."""
    n, i, try_group, want, groups, expected = len(act), 0, True, 0, 0, 0
    pc = lambda a: bin(a).count("1")
    while i + 1 < n:
        if try_group and i + 3 < n:
            a = act[i:i + 4]
            if pc(a[0]) == 2 and a.count(a[0]) == 4:
                expected += a[0] == want
                want = a[0]
                groups += 1
                i += 4
                continue
            try_group = False
        n0, n1 = pc(act[i]), pc(act[i + 1])
        assert not (n0 <= 1 and n1 <= 1), "a wide batch: not modelled"
        nblk = 2 if n0 <= 2 and n0 + n1 <= 4 else 1
        try_group = nblk == 2 and act[i] == act[i + 1] and n0 == 2
        i += nblk
    return groups, expected


def rand12_run(seed: int = 11) -> np.ndarray:
    return g4in.rand12(RUN, seed)


def const_plane(k: int, g: int, pos: int, seed: int = 11) -> np.ndarray:
    """plane k (0 or 1) of block 4g + pos is constant: one test "some lane" fails, no group takes the block"""
    v = rand12_run(seed)
    e = v[(4 * g + pos) * BLOCK:(4 * g + pos + 1) * BLOCK]
    e[:] = (e & np.uint32(0xF00)) | np.uint32(0x5A) if k == 0 else (e & np.uint32(0xFF)) | np.uint32(0x300)
    return v


def third_plane(lane: int, g: int, pos: int, seed: int = 11) -> np.ndarray:
    """one element of one lane of block 4g + pos (not the block's first) sets a bit in plane 2 or 3: the test "no lane" sees it"""
    v = rand12_run(seed)
    v[(4 * g + pos) * BLOCK + 4 * lane + 1 + lane % 3] |= np.uint32(1 << (16 if pos % 2 == 0 else 24))
    return v


PAIRS = ((0, 1), (1, 2), (0, 3), (2, 3))


def plane_pairs(repeat: int, seed: int = 11) -> np.ndarray:
    """the two planes that vary change from group to group, every `repeat` groups: (0,1) -> (1,2) -> (0,3) -> (2,3) -> (0,1) ...
    3-bit values in both planes: the blocks are too small for the mini-LZ, whatever their low bytes are"""
    u = splitmix64(seed, RUN * BLOCK)
    a, b = (u & np.uint64(7)).astype(np.uint32), ((u >> np.uint64(8)) & np.uint64(7)).astype(np.uint32)
    v = np.zeros(RUN * BLOCK, dtype="<u4")
    for g in range(RUN // 4):
        k0, k1 = PAIRS[(g // repeat) % 4]
        s = slice(4 * g * BLOCK, 4 * (g + 1) * BLOCK)
        v[s] = (a[s] << np.uint32(8 * k0)) | (b[s] << np.uint32(8 * k1))
    return v


def first_varies(seed: int = 11) -> np.ndarray:
    """the constant planes 2 and 3 hold another value in every block: the constant bytes come from each block's own first element"""
    v = rand12_run(seed)
    for b in range(RUN):
        v[b * BLOCK:(b + 1) * BLOCK] |= np.uint32(((0x1234 + 0x0B77 * b) & 0xFFFF) << 16)
    return v


# ---- the mini-LZ gate ---------------------------------------------------------------------------------------------------

def plain_bytes(oracle, block: np.ndarray) -> int:
    """f: the bytes of a block's planes when the mini-LZ is not tried (what the gate compares)"""
    out = np.zeros(4096, dtype=np.uint8)
    block = np.ascontiguousarray(block)
    return int(oracle.so_encode_block(block.ctypes.data, 4, out.ctypes.data, 0)) - HS


def sampled_keys(block: np.ndarray) -> int:
    return len(set((block[SAMPLED] & np.uint32(0xFF)).tolist()))


def gate_refuses(f: int, d: int) -> bool:
    """block_compress.h:1210-1221 with lz_precheck_passes (block_codec.h) for 32-bit elements: 80 values, 4 bytes each"""
    return f * 3 > BS and 5 * (80 // 8 + 80 + 3 * d) <= 2 * f


# (f, d) on either side of each inequality: f * 3 > 1024 from 342 on; 5 * (90 + 3 d) <= 2 f holds with equality at (405, 24)
GATE_TARGETS = ((341, 3), (342, 3), (343, 3), (404, 24), (405, 24), (406, 24), (405, 23), (405, 25))


def gate_block(oracle, f: int, d: int, seed: int = 5) -> np.ndarray:
    """A block of `u & 0xFFF` whose planes take exactly f bytes and whose 40 counted low bytes take exactly d values.  Rows of the
    upper plane are narrowed to fewer bits (two bytes a bit), rows of the lower plane behind the counted ones likewise, and a row's
    minimum is raised (a byte): a deterministic search over those, measured by the oracle."""
    keys = ((np.arange(d, dtype=np.uint32) * 37 + 11) & np.uint32(0xFF))
    for trial in range(20000):
        u = splitmix64(seed * 100003 + trial, BLOCK + 128)
        t = u[BLOCK:]
        e = (u[:BLOCK] & np.uint64(0xFFF)).astype(np.uint32)
        narrow = ((t[:16] >> np.uint64(8)) % np.uint64(8) < np.uint64(trial % 9)).astype(np.uint32)  # (none, some or all rows)
        hi_bits = 4 - (t[:16] % np.uint64(5)).astype(np.uint32) * narrow  # 0..4 bits a row of the upper plane
        lo_bits = 8 - (t[16:32] % np.uint64(4)).astype(np.uint32) * (trial % 3 == 0)  # 5..8 bits a row of the lower plane
        raised = (t[32:48] % np.uint64(7) == 0).astype(np.uint32)    # rows whose minimum is 1, not 0
        for r in range(16):
            s = slice(16 * r, 16 * r + 16)
            hi = ((e[s] >> np.uint32(8)) & np.uint32((1 << int(hi_bits[r])) - 1)) + raised[r]
            hi[0], hi[1] = raised[r], raised[r] + ((1 << int(hi_bits[r])) - 1)  # (the row spans exactly its bits)
            lo = e[s] & np.uint32(0xFF)
            if r >= 5:
                lo &= np.uint32((1 << int(lo_bits[r])) - 1)
            e[s] = lo | (hi << np.uint32(8))
        pick = (t[48:88] % np.uint64(d)).astype(np.int64)
        pick[:d] = np.arange(d)  # (every value is there)
        e[SAMPLED] = (e[SAMPLED] & np.uint32(0xFF00)) | keys[pick]
        if acts(e.view(np.uint8)) == [3] and plain_bytes(oracle, e) == f and sampled_keys(e) == d:
            return e
    raise AssertionError(("no block found", f, d))


def gate_run(oracle, nblocks: int, at: int, f: int, d: int) -> np.ndarray:
    """`u & 0xFFF` (blocks the gate lets through: about 410 bytes, 40 values) with gate_block(f, d) as block `at`"""
    v = g4in.rand12(nblocks, 11)
    v[at * BLOCK:(at + 1) * BLOCK] = gate_block(oracle, f, d)
    return v
