"""Inputs for the groups of four int32 blocks of the fused encoder (superblock_codec.h: group4) and for the straight-line
emission of a second pass made of packed rows of values (slot_codec.h: slot_rows_emit_rows_packed), shared by
test_group4_paths_cpu.py and test_gpu_group4_paths.py.

Every input is `u & 0xFFF` in 32-bit elements -- planes 0 and 1 vary, planes 2 and 3 are constant: the shape the groups take --
with ONE block of every group changed; `pos` says which (the second, third or fourth of its group).  What a kind is meant to do:

  group   the group of four takes the blocks (False: it has to give way to the passes of one or two blocks)
  packed  the group's second pass meets the precondition of the straight-line emission (False: one row or plane breaks it and
          the general emission writes the pass)
"""
import numpy as np

from stenos_amd.datagen import splitmix64

BLOCK = 256  # elements
# kind -> (group, packed)
KINDS = {
    "rand12": (True, True),          # nothing changed
    "zero_bits_row": (True, True),   # one row of the upper plane is sixteen equal bytes: a row of 0 bits, still a packed row
    "mins_rle": (True, True),        # upper plane 0..3: every row's minimum is 0, the minima repeat (NORMAL_RLE)
    "mins_plain": (True, True),      # upper plane: the minimum changes from row to row (NORMAL, sixteen minima)
    "rle_row": (True, False),        # one row of the upper plane is two runs of eight: a run-length row (header 7)
    "raw_upper": (True, False),      # the upper plane of one block is noise: every row spans 64 or more, a RAW plane
    "raw_row": (True, False),        # one row of the upper plane spans 0..255 in an otherwise narrow plane: a raw row (header 15)
    "delta_rows": (True, False),     # the upper plane of one block is a slow ramp: rows of differences (headers 8..14)
    "third_plane": (False, False),   # one element of one block has bit 16 set: the block has three planes that vary
    "dict": (False, False),          # one block is drawn from sixteen 12-bit values: the mini-LZ takes it
    "low_two": (False, False),       # the first 80 low bytes of one block take two values: the key count cannot turn the block away
    "low_distinct": (True, True),    # ... are all different: it turns it away at once
}
# distinct low bytes among the first 80 elements, around the count at which the mini-LZ's first rejection test changes sides for
# blocks of this size ((2 * 410 - 450) / 15 = 24.7: block_codec.h, lz_precheck_passes): whichever way a block goes, bytes must agree
THRESHOLD_COUNTS = (20, 22, 23, 24, 25, 26, 27, 29, 33, 41)


def rand12(nblocks: int, seed: int) -> np.ndarray:
    return (splitmix64(seed, nblocks * BLOCK) & np.uint64(0xFFF)).astype("<u4")


def change_block(v: np.ndarray, b: int, kind: str, seed: int, distinct: int = 0) -> None:
    """Block b of the elements v, changed as KINDS says."""
    e = v[b * BLOCK:(b + 1) * BLOCK]
    u = splitmix64(seed + 1000 + b, BLOCK)
    low = e & np.uint32(0xFF)
    row = 5 * 16
    if kind == "rand12":
        return
    if kind == "zero_bits_row":
        e[row:row + 16] = low[row:row + 16] | np.uint32(9 << 8)
    elif kind == "mins_rle":
        e[:] = low | ((u & np.uint64(3)).astype(np.uint32) << 8)
    elif kind == "mins_plain":
        rows = np.repeat(np.arange(16, dtype=np.uint32) % 8, 16)
        e[:] = low | ((rows + (np.arange(BLOCK, dtype=np.uint32) & 1)) << 8)
    elif kind == "rle_row":
        e[row:row + 8] = low[row:row + 8]
        e[row + 8:row + 16] = low[row + 8:row + 16] | np.uint32(15 << 8)
    elif kind == "raw_upper":
        e[:] = (u & np.uint64(0xFFFF)).astype(np.uint32)
        # (a block of two RAW planes is large enough for the mini-LZ unless 39 of the 40 sampled low bytes differ: all of them do)
        e[:80] = (e[:80] & np.uint32(0xFF00)) | ((np.arange(80, dtype=np.uint32) * 37 + 11) & np.uint32(0xFF))
    elif kind == "raw_row":
        e[:] = low | ((u & np.uint64(3)).astype(np.uint32) << 8)
        e[row:row + 16] = low[row:row + 16] | ((u[row:row + 16] & np.uint64(0xFF)).astype(np.uint32) << 8)
        e[row] = low[row]
        e[row + 1] = low[row + 1] | np.uint32(0xFF << 8)
    elif kind == "delta_rows":
        e[:] = low | ((np.arange(BLOCK, dtype=np.uint32) // 2) << 8)
    elif kind == "third_plane":
        e[77] |= np.uint32(1 << 16)
    elif kind == "dict":
        words = (splitmix64(seed + 7, 16) & np.uint64(0xFFF)).astype(np.uint32)
        e[:] = words[(u & np.uint64(15)).astype(np.int64)]
    elif kind == "low_two":  # (far apart, in no order: the rows stay wide and the block large enough for an attempt)
        e[:80] = (e[:80] & np.uint32(0xF00)) | np.where((u[:80] >> np.uint64(20)) & np.uint64(1), np.uint32(0xEE), np.uint32(0x11))
    elif kind == "low_distinct":
        e[:80] = (e[:80] & np.uint32(0xF00)) | ((np.arange(80, dtype=np.uint32) * 37 + 11) & np.uint32(0xFF))
    elif kind == "low_count":
        e[:80] = (e[:80] & np.uint32(0xF00)) | (((np.arange(80, dtype=np.uint32) % distinct) * 37 + 11) & np.uint32(0xFF))
    else:
        raise ValueError(kind)


def make(kind: str, nblocks: int, pos: int, seed: int = 11, distinct: int = 0) -> np.ndarray:
    """nblocks blocks of `u & 0xFFF` as bytes, block `pos` of every whole group of four changed."""
    v = rand12(nblocks, seed)
    for g in range(nblocks // 4):
        change_block(v, 4 * g + pos, kind, seed, distinct)
    return v.view(np.uint8).copy()
