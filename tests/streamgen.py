"""A writer of block-superblock streams that makes FREE choices (test infrastructure).

Every encoder of this project -- the oracle, the reference, the library -- makes the same choices, so streams they
produce reach a small corner of the format.  This writer takes the data a stream must decode to and a seeded numpy
generator and draws, wherever the format leaves a choice, one of the legal alternatives: any row header that can
represent the row (wider than needed included), any minimum that works modulo 256, run-length masks that leave
repeats unmerged, NORMAL planes made of raw rows, mini-LZ streams with two-byte distances below 128, copy blocks
anywhere.  The truth of a test is the data the stream was built from.

Written from the format as oracle/stenos_oracle.c restates it (so_block_decompress, get_plane, get_rle, unpack16,
lz_decode, partial_decompress) and SURVEY.md Appendix A:

  block        [type nibbles: (T + 1) / 2 bytes][plane 0] .. [plane T-1]  |  [252][256 * T raw bytes]  |  [253][mini-LZ]
  plane        SAME: 1 byte.  RAW: 256 bytes.  NORMAL: 8 bytes of row header nibbles, a minimum byte for every row whose
               header is not 6, 7 or 15, the rows.  NORMAL_RLE: the header nibbles, the sixteen minimums as one run-length
               row (value in front of the first: 0), the rows.
  row header   0-5: sixteen values of that many bits + the minimum.  8-14: the same for the differences (0-6 bits) to the
               byte before (in front of row 0: 0).  15: sixteen raw bytes.  7: run-length row of the values (mask16, a set
               bit repeats the byte before; then the other bytes).  6: run-length row of the differences (the difference
               in front of a row's first is 0).
  bit packing  two halves of eight values, each `bits` bytes, value k at bit k * bits (little endian)
  mini-LZ      items of B = 8 (T % 8 == 0) or 4 bytes; per eight items a flags byte, then per item B literal bytes or a
               distance in items: one byte < 128, or (d & 127) | 128, d >> 7
  tail         [254], planes (SAME / NORMAL) over lines = n / (16 * T) rows, then the remaining n - lines * 16 * T raw bytes
  frame        [shift][total: 7 bytes]([superblock bytes: 4] when shift == 255) then per superblock [code][csize: 3][payload],
               code 1 = block stream, 6 = copy
"""
from __future__ import annotations

from dataclasses import dataclass, replace

import numpy as np

SAME, RAW, NORMAL, NORMAL_RLE = 0, 1, 2, 3
BLOCK_COPY, BLOCK_LZ, BLOCK_PARTIAL = 252, 253, 254
PLAIN_HEADERS = (0, 1, 2, 3, 4, 5)
DELTA_HEADERS = (8, 9, 10, 11, 12, 13, 14)
ALL_HEADERS = tuple(range(16))


def header_bytes(T: int) -> int:
    return (T + 1) // 2


def max_block_bytes(T: int) -> int:
    """the longest block an ENCODER writes (superblock_codec.h); the format allows longer ones: Choices.oversize"""
    return 256 * T + header_bytes(T) + 1


def max_format_block_bytes(T: int) -> int:
    """the longest block of the format: every plane NORMAL_RLE, sixteen run-length rows of sixteen literals"""
    return header_bytes(T) + T * (8 + 18 + 16 * 18)


def lz_width(T: int) -> int:
    """item width of the mini-LZ where a block may be one (T % 4 == 0, at most 512); 0: no mini-LZ"""
    if T > 512 or T % 4:
        return 0
    return 8 if T % 8 == 0 else 4


@dataclass(frozen=True)
class Choices:
    """What the writer may choose from.  The defaults allow everything but blocks longer than max_block_bytes(T)."""

    block_kinds: tuple = ("planes", "planes", "planes", "planes", "copy", "lz")  # drawn uniformly; "lz" where the format has it
    plane_types: tuple = (RAW, NORMAL, NORMAL, NORMAL_RLE, NORMAL_RLE)  # of a plane that is not written as SAME
    p_same: float = 0.9  # a constant plane is written as SAME with this probability (otherwise as any other plane)
    headers: tuple = ALL_HEADERS  # row headers to draw from (among those that can represent the row; 6, 7, 15 always can)
    p_plane_one_header: float = 0.2  # a plane draws ONE of 6, 7, 15 and uses it for every row (the decoder's short forms)
    p_odd_row: float = 0.0  # ... but for one row, which takes another of the three (a plane that is ALMOST of a short form)
    row_rle: str = "random"  # run-length masks of rows: "greedy" merges every repeat, "lazy" some, "none" none, "random" one of them per row
    mins_rle: str = "random"  # the same for the mask of a NORMAL_RLE plane's minimums
    oversize: bool = False  # blocks longer than max_block_bytes(T) (no encoder writes them; the format allows them)
    lz_p_match: float = 0.75  # an item that has an equal one in front of it becomes a match
    lz_p_two: float = 0.25  # a distance below 128 is written in the two-byte form
    lz_first_two_group: int = -1  # >= 0: one-byte distances only in front of this group, a two-byte one in it if it has a match
    lz_dist: str = "any"  # "any": any equal item in front, "near": the nearest, "far": the farthest


LEGAL = Choices()
OVERSIZE = replace(LEGAL, oversize=True)


# Choices that steer the decoder into each of its forms (block_codec.h, decode_plane)
PACKED = PLAIN_HEADERS + DELTA_HEADERS
PLANES_ONLY = replace(LEGAL, block_kinds=("planes",), plane_types=(NORMAL, NORMAL_RLE), p_same=0.3)
VARIANTS = {
    "legal": LEGAL,
    "oversize": OVERSIZE,
    "packed": replace(PLANES_ONLY, headers=PACKED, p_plane_one_header=0.0),
    "packed+raw": replace(PLANES_ONLY, headers=PACKED + (15,), p_plane_one_header=0.0),
    "packed+6": replace(PLANES_ONLY, headers=PACKED + (15, 6), p_plane_one_header=0.0),
    "packed+6+7": replace(PLANES_ONLY, headers=ALL_HEADERS, p_plane_one_header=0.0),
    "all7": replace(PLANES_ONLY, plane_types=(NORMAL,), p_same=0.0, headers=(7,), oversize=True),  # decode_plane_runs
    "all6": replace(PLANES_ONLY, plane_types=(NORMAL,), p_same=0.0, headers=(6,), oversize=True),  # decode_plane_slopes
    "all7_rle": replace(PLANES_ONLY, plane_types=(NORMAL_RLE,), p_same=0.0, headers=(7,), oversize=True),  # (minimums nobody uses)
    "all6_rle": replace(PLANES_ONLY, plane_types=(NORMAL_RLE,), p_same=0.0, headers=(6,), oversize=True),
    "all15": replace(PLANES_ONLY, headers=(15,), oversize=True),  # NORMAL planes of sixteen raw rows: 264 bytes
    "mix6715": replace(PLANES_ONLY, headers=(6, 7, 15) + PACKED[:3], p_plane_one_header=0.0, oversize=True),
    "wrap": replace(PLANES_ONLY, headers=PACKED, p_plane_one_header=0.0),  # with "straddle" data: minimums that wrap
    "unmerged": replace(PLANES_ONLY, headers=(6, 7), row_rle="none", mins_rle="none", oversize=True),
    "lz": replace(LEGAL, block_kinds=("lz",), oversize=True),
    "lz_literals": replace(LEGAL, block_kinds=("lz",), lz_p_match=0.0, oversize=True),  # flags 0x00 throughout
    "lz_matches": replace(LEGAL, block_kinds=("lz",), lz_p_match=1.0, lz_p_two=0.0, lz_dist="near"),  # flags 0xFF after the first group
    "lz_two_first": replace(LEGAL, block_kinds=("lz",), lz_p_match=1.0, lz_first_two_group=1, oversize=True),
    "lz_two_middle": replace(LEGAL, block_kinds=("lz",), lz_p_match=1.0, lz_p_two=0.0, lz_first_two_group=15, oversize=True),
    "lz_two_last": replace(LEGAL, block_kinds=("lz",), lz_p_match=1.0, lz_p_two=0.0, lz_first_two_group=31, oversize=True),
    "lz_far": replace(LEGAL, block_kinds=("lz",), lz_p_match=0.9, lz_dist="far", oversize=True),
    "copy": replace(LEGAL, block_kinds=("copy", "planes")),
    "almost": replace(PLANES_ONLY, p_same=0.0, headers=(6, 7, 15), p_plane_one_header=1.0, p_odd_row=1.0, oversize=True),  # fifteen rows of one kind and one of another
}
DATA_STYLE = {"wrap": "straddle", "lz_matches": "dict8", "lz_two_first": "dict8", "lz_two_middle": "dict8", "lz_two_last": "dict8", "lz": "dict", "lz_far": "dict",
              "all7": "steps", "all6": "slopes", "all7_rle": "runs", "all6_rle": "slopes", "unmerged": "runs", "almost": "steps"}


# ---- rows ------------------------------------------------------------------------------------------------------------

_MS = np.arange(256, dtype=np.int64)[:, None]


def _spans(vals: np.ndarray) -> np.ndarray:
    """span[m] = max over the row of (v - m) & 255: the row fits `bits` bits with minimum m when span[m] < 2 ** bits"""
    return ((vals[None, :].astype(np.int64) - _MS) & 255).max(axis=1)


def _pack16(vals, bits: int) -> bytes:
    out = bytearray()
    for h in range(2):
        acc = 0
        for k in range(8):
            acc |= int(vals[8 * h + k]) << (k * bits)
        out += acc.to_bytes(bits, "little")
    return bytes(out)


def _rle_row(vals, prev: int, mode: str, rng) -> bytes:
    """mask16 + literals: bit c set = value c repeats the one before (`prev` in front of the first)"""
    if mode == "random":
        mode = ("greedy", "lazy", "none")[int(rng.integers(3))]
    mask, lits = 0, bytearray()
    for c in range(16):
        v = int(vals[c])
        if v == prev and (mode == "greedy" or (mode == "lazy" and rng.random() < 0.5)):
            mask |= 1 << c
        else:
            lits.append(v)
        prev = v
    return mask.to_bytes(2, "little") + bytes(lits)


def _encode_row(vals: np.ndarray, last: int, ch: Choices, rng, forced: int | None, max_rle_bytes: int):
    """-> (header, minimum or None, payload).  vals: the sixteen bytes, last: the byte in front of them."""
    prev = np.concatenate(([last], vals[:-1])).astype(np.int64)
    diffs = ((vals.astype(np.int64) - prev) & 255).astype(np.uint8)
    cand = {}
    if forced is None:
        sv, sd = _spans(vals), _spans(diffs)
        for h in PLAIN_HEADERS:
            ms = np.flatnonzero(sv < (1 << h))
            if ms.size:
                cand[h] = ("plain", ms)
        for h in DELTA_HEADERS:
            ms = np.flatnonzero(sd < (1 << (h - 8)))
            if ms.size:
                cand[h] = ("delta", ms)
    r7 = _rle_row(vals, last, ch.row_rle, rng)
    r6 = _rle_row(diffs, 0, ch.row_rle, rng)
    if len(r7) <= max_rle_bytes:
        cand[7] = ("rle", r7)
    if len(r6) <= max_rle_bytes:
        cand[6] = ("rle", r6)
    cand[15] = ("raw", None)
    if forced is not None and forced in cand:
        h = forced
    else:
        allowed = [h for h in cand if h in ch.headers] or sorted(cand)
        h = int(allowed[int(rng.integers(len(allowed)))])
    kind, arg = cand[h]
    if kind == "raw":
        return h, None, vals.tobytes()
    if kind == "rle":
        return h, None, arg
    m = int(arg[int(rng.integers(arg.size))])  # ANY minimum that works modulo 256
    src = vals if kind == "plain" else diffs
    bits = h & 7
    return h, m, _pack16((src.astype(np.int64) - m) & 255, bits)


def encode_plane(plane: np.ndarray, lines: int, ptype: int, ch: Choices, rng, max_rle_bytes: int = 18) -> bytes:
    """`lines` rows of one plane (16 = a full block's) as NORMAL or NORMAL_RLE"""
    forced = None
    if rng.random() < ch.p_plane_one_header:
        one = [h for h in (6, 7, 15) if h in ch.headers]
        if one:
            forced = one[int(rng.integers(len(one)))]
    odd_row, odd = -1, None
    if forced is not None and ch.p_odd_row and rng.random() < ch.p_odd_row:
        odd_row = int(rng.integers(lines))
        odd = [h for h in (6, 7, 15) if h != forced][int(rng.integers(2))]
    hdrs, mins, rows = [], [], []
    last = 0
    for r in range(lines):
        vals = plane[16 * r:16 * r + 16]
        h, m, payload = _encode_row(vals, last, ch, rng, odd if r == odd_row else forced, max_rle_bytes)
        hdrs.append(h)
        mins.append(m)
        rows.append(payload)
        last = int(vals[15])
    nib = bytearray((lines + 1) // 2)
    for r, h in enumerate(hdrs):
        nib[r >> 1] |= h << (4 * (r & 1))
    if ptype == NORMAL:
        minbytes = bytes(m for m in mins if m is not None)
    else:
        assert lines == 16
        # every row has a minimum here; rows without a use for one get the one before (so that the mask has bits) or anything
        full, prev = [], 0
        for m in mins:
            if m is None:
                m = prev if rng.random() < 0.6 else int(rng.integers(256))
            full.append(m)
            prev = m
        minbytes = _rle_row(full, 0, ch.mins_rle, rng)
    return bytes(nib) + minbytes + b"".join(rows)


# ---- blocks ----------------------------------------------------------------------------------------------------------


def encode_lz(block: np.ndarray, T: int, ch: Choices, rng) -> bytes:
    """[253] + the mini-LZ stream of a full block; literals and matches at will"""
    B = lz_width(T)
    assert B
    items = block.reshape(-1, B)
    count = items.shape[0]
    keys = [it.tobytes() for it in items]
    seen: dict = {}
    out = bytearray([BLOCK_LZ])
    forced_done = False
    for g in range(count // 8):
        flags, body = 0, bytearray()
        for j in range(8):
            pos = 8 * g + j
            before = seen.get(keys[pos], ())
            only_short = 0 <= g < ch.lz_first_two_group
            want_two = g == ch.lz_first_two_group and not forced_done
            if only_short:
                before = [p for p in before if pos - p < 128]
            if before and (want_two or rng.random() < ch.lz_p_match):
                if ch.lz_dist == "near":
                    src = before[-1]
                elif ch.lz_dist == "far":
                    src = before[0]
                else:
                    src = before[int(rng.integers(len(before)))]
                d = pos - src
                two = d >= 128 or want_two or (not only_short and rng.random() < ch.lz_p_two)
                forced_done = forced_done or want_two
                flags |= 1 << j
                if two:
                    body += bytes([(d & 127) | 128, d >> 7])
                else:
                    body.append(d)
            else:
                body += keys[pos]
            seen.setdefault(keys[pos], []).append(pos)
        out.append(flags)
        out += body
    return bytes(out)


def encode_planes_block(block: np.ndarray, T: int, ch: Choices, rng) -> bytes:
    elems = block.reshape(256, T)
    head = bytearray(header_bytes(T))
    body = bytearray()
    for j in range(T):
        plane = np.ascontiguousarray(elems[:, j])
        if (plane == plane[0]).all() and rng.random() < ch.p_same:
            ptype, enc = SAME, bytes([int(plane[0])])
        else:
            ptype = int(ch.plane_types[int(rng.integers(len(ch.plane_types)))])
            if ptype == RAW:
                enc = plane.tobytes()
            else:
                enc = encode_plane(plane, 16, ptype, ch, rng)
                if len(enc) > 256 and not ch.oversize:  # (what an encoder does with such a plane)
                    ptype, enc = RAW, plane.tobytes()
        head[j >> 1] |= ptype << (4 * (j & 1))
        body += enc
    return bytes(head) + bytes(body)


def encode_block(block: np.ndarray, T: int, ch: Choices, rng, kind: str | None = None) -> bytes:
    """one full block (256 * T bytes, element major)"""
    if kind is None:
        kind = ch.block_kinds[int(rng.integers(len(ch.block_kinds)))]
    if kind == "lz" and lz_width(T):
        enc = encode_lz(block, T, ch, rng)
        if ch.oversize or len(enc) <= max_block_bytes(T):
            return enc
        kind = "planes"
    if kind == "copy":
        return bytes([BLOCK_COPY]) + block.tobytes()
    return encode_planes_block(block, T, ch, rng)


def encode_tail(tail: np.ndarray, T: int, ch: Choices, rng) -> bytes:
    """[254] + the partial block of the n < 256 * T bytes behind the last full block"""
    n = tail.size
    lines = n // (16 * T)
    out = bytearray([BLOCK_PARTIAL])
    if lines:
        elems = tail[:lines * 16 * T].reshape(lines * 16, T)
        head = bytearray(header_bytes(T))
        body = bytearray()
        for j in range(T):
            plane = np.ascontiguousarray(elems[:, j])
            if (plane == plane[0]).all() and rng.random() < ch.p_same:
                ptype, enc = SAME, bytes([int(plane[0])])
            else:  # (no RAW and no NORMAL_RLE planes in a partial block; a run-length row longer than a raw one only on request)
                ptype, enc = NORMAL, encode_plane(plane, lines, NORMAL, ch, rng, 18 if ch.oversize else 16)
            head[j >> 1] |= ptype << (4 * (j & 1))
            body += enc
        out += head + body
    out += tail[lines * 16 * T:].tobytes()
    return bytes(out)


def encode_payload(data: np.ndarray, T: int, ch: Choices, rng, kinds=None) -> bytes:
    """the payload of one BLOCK superblock (code 1) that decodes to `data` (uint8)"""
    data = np.ascontiguousarray(data, dtype=np.uint8).ravel()
    bs = 256 * T
    nb = data.size // bs
    out = bytearray()
    for b in range(nb):
        out += encode_block(data[b * bs:(b + 1) * bs], T, ch, rng, kinds[b] if kinds else None)
    if data.size > nb * bs:
        out += encode_tail(data[nb * bs:], T, ch, rng)
    return bytes(out)


# ---- frames ----------------------------------------------------------------------------------------------------------


def base_superblock(T: int) -> int:
    bs = 256 * T
    return bs if bs > 131072 else (131072 // bs) * bs


def make_frame(data: np.ndarray, T: int, ch: Choices, rng, sb_bytes: int | None = None, shift: int = 0, p_copy: float = 0.0,
               choices_per_superblock=None):
    """-> (frame as uint8 array, offsets of the superblock headers).  sb_bytes: a custom superblock size (frame[0] = 255), a multiple of
    the block size.  p_copy: share of full-size superblocks stored with code 6.  choices_per_superblock: a function s -> Choices."""
    data = np.ascontiguousarray(data, dtype=np.uint8).ravel()
    out = bytearray()
    if sb_bytes is None:
        sb = base_superblock(T) << shift
        out += bytes([shift]) + data.size.to_bytes(7, "little")
    else:
        assert sb_bytes % (256 * T) == 0 and sb_bytes >= 256 * T
        sb = sb_bytes
        out += bytes([255]) + data.size.to_bytes(7, "little") + sb.to_bytes(4, "little")
    offs = []
    for s, lo in enumerate(range(0, data.size, sb)):
        part = data[lo:lo + sb]
        offs.append(len(out))
        if rng.random() < p_copy:
            out += bytes([6]) + part.size.to_bytes(3, "little") + part.tobytes()
        else:
            pay = encode_payload(part, T, choices_per_superblock(s) if choices_per_superblock else ch, rng)
            out += bytes([1]) + len(pay).to_bytes(3, "little") + pay
    offs.append(len(out))
    return np.frombuffer(bytes(out), dtype=np.uint8).copy(), offs


def frame_of_payload(payload: bytes, T: int, dsize: int) -> np.ndarray:
    """one superblock of dsize <= the default superblock size around a payload: [0][n: 7][1][csize: 3][payload]"""
    assert 0 < dsize <= base_superblock(T)
    return np.frombuffer(bytes([0]) + dsize.to_bytes(7, "little") + bytes([1]) + len(payload).to_bytes(3, "little") + payload, dtype=np.uint8).copy()


def frame_of_payloads(payloads, T: int, sb_bytes: int, total: int):
    """A frame of BLOCK superblocks (code 1) around given payloads, whatever they hold: [255][total: 7][sb_bytes: 4], then
    [1][csize: 3][payload] for every payload -> (frame as uint8 array, offsets of the superblock headers and the end), as make_frame"""
    assert sb_bytes % (256 * T) == 0 and sb_bytes >= 256 * T
    assert len(payloads) == -(-total // sb_bytes)
    out = bytearray(bytes([255]) + total.to_bytes(7, "little") + sb_bytes.to_bytes(4, "little"))
    offs = []
    for pay in payloads:
        offs.append(len(out))
        out += bytes([1]) + len(pay).to_bytes(3, "little") + bytes(pay)
    offs.append(len(out))
    return np.frombuffer(bytes(out), dtype=np.uint8).copy(), offs


# ---- data that makes every choice reachable ------------------------------------------------------------------------------

PLANE_STYLES = ("const", "small", "straddle", "runs", "slopes", "walk", "noise", "steps", "rowmix", "tiny_delta")


def _plane(rng, style: str, n: int) -> np.ndarray:
    if style == "const":
        return np.full(n, rng.integers(256), dtype=np.uint8)
    if style == "small":  # a few bits above a base: plain widths, wider ones too
        return (rng.integers(256) + rng.integers(0, 1 << int(rng.integers(1, 6)), n)).astype(np.uint8)
    if style == "straddle":  # a range across 255 / 0: minimums that wrap
        return (250 + rng.integers(0, int(rng.integers(2, 14)), n)).astype(np.uint8)
    if style == "runs":
        reps = rng.integers(1, 40, n)
        return np.repeat(rng.integers(0, 256, n), reps)[:n].astype(np.uint8)
    if style == "steps":
        reps = rng.integers(10, 90, n)
        return np.repeat(rng.integers(0, 256, n), reps)[:n].astype(np.uint8)
    if style == "slopes":  # piecewise linear: runs of equal differences
        reps = rng.integers(2, 50, n)
        d = np.repeat(rng.integers(-3, 4, n), reps)[:n]
        return (rng.integers(256) + np.cumsum(d)).astype(np.uint8)
    if style == "walk":
        return (rng.integers(256) + np.cumsum(rng.integers(-5, 6, n))).astype(np.uint8)
    if style == "tiny_delta":  # differences of one or two bits around a drift: delta widths
        return (rng.integers(256) + np.cumsum(int(rng.integers(0, 4)) + rng.integers(0, int(rng.integers(1, 4)), n))).astype(np.uint8)
    if style == "rowmix":  # another style every row or two
        out = np.empty(n + 32, dtype=np.uint8)
        for lo in range(0, n, 32):
            out[lo:lo + 32] = _plane(rng, PLANE_STYLES[int(rng.integers(7))], 32)
        return out[:n]
    return rng.integers(0, 256, n).astype(np.uint8)


def make_data(rng, T: int, nbytes: int, style: str | None = None) -> np.ndarray:
    """nbytes of data, block by block: each plane of each block in a style of its own (style: one for all), or whole elements
    out of a small dictionary (the mini-LZ's food; style "dict", "dict8": eight distinct elements first, then only repeats of them)"""
    bs = 256 * T
    out = np.empty(((nbytes + bs - 1) // bs) * bs if nbytes else 0, dtype=np.uint8)
    for lo in range(0, out.size, bs):
        s = style
        if s is None and lz_width(T) and rng.random() < 0.3:
            s = "dict"
        if s in ("dict", "dict8"):
            B = lz_width(T) or T
            count = bs // B
            k = 8 if s == "dict8" else int(rng.integers(2, 40))
            words = rng.integers(0, 256, (k, B)).astype(np.uint8)
            words[:, 0] = np.arange(k)  # distinct
            idx = rng.integers(0, k, count)
            if s == "dict8":
                idx[:8] = np.arange(8)
            elif rng.random() < 0.5:  # some noise in between: literals among the matches
                noise = rng.random(count) < 0.2
                blockv = words[idx]
                blockv[noise] = rng.integers(0, 256, (int(noise.sum()), B))
                out[lo:lo + bs] = blockv.ravel()
                continue
            out[lo:lo + bs] = words[idx].ravel()
            continue
        block = np.empty((256, T), dtype=np.uint8)
        for j in range(T):
            block[:, j] = _plane(rng, s or PLANE_STYLES[int(rng.integers(len(PLANE_STYLES)))], 256)
        out[lo:lo + bs] = block.ravel()
    return out[:nbytes].copy()


def make_mixed_frame(rng, T: int, nsb: int, blocks_per_sb: int, last_bytes: int, p_copy: float = 0.15, names=None, default_size: bool = False):
    """A frame of nsb superblocks of blocks_per_sb blocks each -- every one written with a variant of VARIANTS drawn on its own, on
    data in that variant's style, or stored as a copy (code 6) -- and a last superblock of last_bytes (> 0, not a whole superblock).
    default_size: the bytesoftype's default superblock size (frame[0] = 0; blocks_per_sb is ignored), else a custom one (frame[0] = 255).
    -> (frame, header offsets, data)"""
    names = [n for n in (names or VARIANTS) if lz_width(T) or not n.startswith("lz")]
    sb = base_superblock(T) if default_size else blocks_per_sb * 256 * T
    assert 0 < last_bytes < sb
    total = nsb * sb + last_bytes
    out = bytearray(bytes([0 if default_size else 255]) + total.to_bytes(7, "little") + (b"" if default_size else sb.to_bytes(4, "little")))
    parts, offs = [], []
    for s in range(nsb + 1):
        n = sb if s < nsb else last_bytes
        name = names[int(rng.integers(len(names)))]
        part = make_data(rng, T, n, DATA_STYLE.get(name))
        parts.append(part)
        offs.append(len(out))
        if s < nsb and rng.random() < p_copy:
            out += bytes([6]) + n.to_bytes(3, "little") + part.tobytes()
        else:
            pay = encode_payload(part, T, VARIANTS[name], rng)
            out += bytes([1]) + len(pay).to_bytes(3, "little") + pay
    offs.append(len(out))
    return np.frombuffer(bytes(out), dtype=np.uint8).copy(), offs, np.concatenate(parts)
