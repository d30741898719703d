"""The device-frame calls on arrays and frames beyond 4 GiB (include/stenos_hip.h: stenos_hip_frame_index, stenos_hip_decompress,
stenos_hip_decompress_ranges, stenos_hip_gather_rows, stenos_hip_update_rows, the batch calls, and the host-pointer calls once):
byte offsets in the original array at and above 2^31 and 2^32, offsets inside the frame at and above 2^31 and 2^32, row numbers
that need more than 32 bits, products i * stride and n * row_bytes above 2^32, a range longer than 2^32, a batch whose items
together exceed 2^32 bytes, and more than 2^20 superblocks in one frame.  One uint32_t temporary in an address expression is
wrong from the 32 769th int32 superblock onwards; nothing below these sizes can see it.

Two arrays are made once, on the device (stenos_amd.datagen.generate_torch), and compressed at level 1:

  A  bytesoftype 4, 2^32 + 5 * 131072 + 1003 bytes: the first 1.5 GiB `rand` (stored as copies), the rest `rand12` (coded at
     about 0.4).  The frame is about 2.5 GiB, and all three crossings lie in coded superblocks of the rand12 part, in three
     different places: array offset 2^31 (frame offset about 1.7 GiB), frame offset 2^31 (array offset about 2.75 GiB), array
     offset 2^32 (frame offset about 2.5 GiB).  The split is at 1.5 GiB; the fixture asserts what it relies on.
  B  bytesoftype 2 (the row-lane int16 kernels; more than 2^31 elements): 2^32 bytes of `rand`, 8 superblocks of `walk`, 77 bytes
     more of it.  The copies push the walk superblocks behind frame offset 2^32: blocks are decoded and encoded there.  The last
     superblock (77 bytes, under 128) has a zstd-based code, so what touches it goes through the host's part of each call.

The reference is the source tensor on the device: a range or a row is a slice of it, an updated array is the source with slices
written.  Tensors above 1 GiB are compared in chunks of at most 1 GiB (torch switches algorithms above 2^31 elements), and for
every bulk comparison a few KiB around each crossing are brought to the host and compared with numpy.  Nothing of array size
crosses PCIe except in the one host-ABI test.

MEMORY: A and B with their frames hold 14.5 GiB for the whole module; the largest test on top of that (the update with source
rows 2^31 + 8 apart: 4 GiB of source rows, 4 GiB for the reference compression, 2.5 GiB of output) reaches 25 GiB.  The tests
skip only when the device reports less than NEED_BYTES free at the start of the module."""
import ctypes
import time

import numpy as np
import pytest
import torch

from _libs import oracle_compress
from stenos_amd.api import Stenos, StenosError
from stenos_amd.datagen import generate_torch

pytestmark = pytest.mark.gpu

GIB = 1 << 30
NEED_BYTES = 26 * GIB
SB = 131072  # the default superblock of bytesoftype 2 and 4
P31, P32 = 1 << 31, 1 << 32
GUARD, GUARD_BYTE = 64, 0xA5
INVALID_PARAMETER = (1 << 64) - 9
WINDOW = 2048  # bytes on each side of a crossing that are compared on the host


def _hip():
    return ctypes.CDLL("libamdhip64.so")


def _free_cache():
    torch.cuda.empty_cache()


@pytest.fixture(autouse=True)
def _release_between_tests():
    yield
    _free_cache()


@pytest.fixture(scope="module")
def room():
    assert torch.cuda.is_available()
    _free_cache()
    free = torch.cuda.mem_get_info()[0]
    if free < NEED_BYTES:
        pytest.skip(f"needs {NEED_BYTES >> 30} GiB of free device memory, the device reports {free / GIB:.1f} GiB")
    LOW_WATER[0] = free
    yield
    # (sampled where the bulk comparisons run, with the tensors of a test and the contexts' own workspaces in place)
    print(f"\ndevice memory in use at the comparisons of this module: at most {(free - LOW_WATER[0]) / GIB:.1f} GiB of the {NEED_BYTES >> 30} GiB asked for")


# ---- comparisons -------------------------------------------------------------------------------------------------------

LOW_WATER = [0]  # the least free device memory seen by _same and _all_guard


def _sample_memory():
    LOW_WATER[0] = min(LOW_WATER[0], torch.cuda.mem_get_info()[0])


def _first_difference(got, want):
    return int((got != want).nonzero()[0].item())


def _same(got, want, points=(), what=""):
    """two flat uint8 device tensors of one size: equal chunk by chunk (at most 1 GiB each), and equal on the host (numpy) in the
    windows around `points` (offsets into the tensors) and at both ends"""
    _sample_memory()
    n = got.numel()
    assert want.numel() == n and got.dtype == want.dtype == torch.uint8, (what, n, want.numel())
    for o in range(0, n, GIB):
        g, w = got[o:o + GIB], want[o:o + GIB]
        if not torch.equal(g, w):
            raise AssertionError(f"{what}: byte {o + _first_difference(g, w)} of {n} differs")
    for p in list(points) + [0, n]:
        a, b = max(0, min(n, p - WINDOW)), max(0, min(n, p + WINDOW))
        if a < b:
            g, w = got[a:b].cpu().numpy(), want[a:b].cpu().numpy()
            assert np.array_equal(g, w), f"{what}: on the host, byte {a + int(np.flatnonzero(g != w)[0])} of {n} differs (window around {p})"


def _all_guard(t, what):
    _sample_memory()
    for o in range(0, t.numel(), GIB):
        c = t[o:o + GIB]
        if not bool((c == GUARD_BYTE).all().item()):
            raise AssertionError(f"{what}: byte {o + _first_difference(c, torch.full_like(c, GUARD_BYTE))} is no sentinel any more")


def _copy_in_chunks(dst, src):
    assert dst.numel() == src.numel()
    for o in range(0, src.numel(), GIB):
        dst[o:o + GIB].copy_(src[o:o + GIB])


def _index_of(ptr, nsb):
    """the nsb + 1 offsets at the device address ptr: as a list of ints and as a device tensor of the caller's own"""
    dev = torch.empty(nsb + 1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    assert _hip().hipMemcpy(ctypes.c_void_p(dev.data_ptr()), ctypes.c_void_p(ptr), ctypes.c_size_t((nsb + 1) * 8), 3) == 0
    return dev.cpu().tolist(), dev


def _rows_tensor(rows):
    return torch.from_numpy(np.asarray(rows, dtype=np.uint64).view(np.int64)).cuda()


def _code(call):
    try:
        return call()
    except StenosError as err:
        return err.code


def _host(t, lo, n):
    return t[lo:lo + n].cpu().numpy()


# ---- the two arrays ------------------------------------------------------------------------------------------------------

def _fill(out, at, kind, T, nbytes, seed, slab_elements=1 << 26):
    """out[at : at + nbytes] = the first nbytes of the sequence `kind`, made slab by slab"""
    done = 0
    while done < nbytes:
        n = min(slab_elements, -(-(nbytes - done) // T))
        v = generate_torch(kind, T, n, seed, start=done // T)
        take = min(n * T, nbytes - done)
        out[at + done:at + done + take] = v[:take]
        done += take
        del v


class Big:
    """an array on the device, its level-1 frame, the frame's index (host list and device tensor) and the context that made it"""

    def __init__(self, name, T, src, lib):
        self.name, self.T, self.sb, self.src, self.total = name, T, SB, src, src.numel()
        self.st = Stenos(1, lib=lib)
        dst = torch.empty(self.st.bound(self.total), dtype=torch.uint8, device="cuda")
        self.csize = self.st.compress(src, T, dst)
        p, self.nsb = self.st.last_index()
        assert p and self.nsb == -(-self.total // self.sb), (self.nsb, self.total)
        self.index, self.index_dev = _index_of(p, self.nsb)
        assert self.index[0] == 8 and self.index[-1] == self.csize and all(a < b for a, b in zip(self.index, self.index[1:]))
        self.frame = dst[:self.csize].clone()  # (trimmed: the bound's 4 GiB are not kept)
        del dst
        _free_cache()

    @property
    def index_ptr(self):
        return self.index_dev.data_ptr()

    def code(self, k):
        return int(self.frame[self.index[k]].item())

    def superblock_at_frame_offset(self, off):
        k = int(np.searchsorted(np.asarray(self.index, dtype=np.uint64), np.uint64(off), side="right")) - 1
        assert 0 <= k < self.nsb and self.index[k] <= off < self.index[k + 1]
        return k

    def frame_points(self):
        return [p for p in (P31, P32) if p < self.csize]


@pytest.fixture(scope="module")
def A(room, hooks_lib):
    T, total, split = 4, P32 + 5 * SB + 1003, 3 * GIB // 2
    src = torch.empty(total, dtype=torch.uint8, device="cuda")
    _fill(src, 0, "rand", T, split, 11)
    _fill(src, split, "rand12", T, total - split, 12)
    big = Big("A", T, src, hooks_lib)
    assert big.csize > P31 + (64 << 20), f"the frame of A has {big.csize} bytes: frame offsets do not pass 2^31 by 64 MiB"
    big.kf = big.superblock_at_frame_offset(P31)
    assert big.code(big.kf) == 1, f"frame offset 2^31 of A lies in superblock {big.kf} with code {big.code(big.kf)}: not a coded one"
    assert big.code(0) == 6 and big.code(P31 // SB) == 1 and big.kf > P31 // SB and big.index[P32 // SB] > P31
    # crossings as offsets in the array: array 2^31; both ends of the superblock that holds frame offset 2^31; array 2^32
    big.crossings = [P31, big.kf * SB, (big.kf + 1) * SB, P32]
    print(f"\nA: {total} bytes, {big.nsb} superblocks, frame {big.csize} bytes = 2^31 + {(big.csize - P31) / (1 << 20):.1f} MiB; frame offset 2^31 in superblock "
          f"{big.kf} (array offset {big.kf * SB}, code {big.code(big.kf)}); array offset 2^32 at frame offset {big.index[P32 // SB]}")
    yield big
    big.st.close()


@pytest.fixture(scope="module")
def B(room, hooks_lib):
    T, tail = 2, 8 * SB + 77
    total = P32 + tail
    src = torch.empty(total, dtype=torch.uint8, device="cuda")
    _fill(src, 0, "rand", T, P32, 21, slab_elements=1 << 27)
    src[P32:] = generate_torch("walk", T, tail // T + 1, 22)[:tail]
    big = Big("B", T, src, hooks_lib)
    first = P32 // SB
    assert big.index[first] > P32, f"the first walk superblock of B starts at frame offset {big.index[first]}: not beyond 2^32"
    assert all(big.code(first + k) == 1 for k in range(8)), "the walk superblocks of B were meant to be coded"
    big.kf = big.superblock_at_frame_offset(P32)
    big.first_walk = first
    # array 2^31; the superblock that holds frame offset 2^32; array 2^32 = the first walk superblock; the last, 77-byte superblock
    big.crossings = [P31, big.kf * SB, P32, total - 77]
    print(f"\nB: {total} bytes, {big.nsb} superblocks, frame {big.csize} bytes; the walk superblocks start at frame offset 2^32 + {big.index[first] - P32} "
          f"with code {big.code(first)}; frame offset 2^32 in superblock {big.kf} (code {big.code(big.kf)}); the last superblock has code {big.code(big.nsb - 1)}")
    yield big
    big.st.close()


@pytest.fixture(scope="module")
def both(A, B):
    return {"A": A, "B": B}


# ---- 1. index and walk ---------------------------------------------------------------------------------------------------

def _walked(st, frame, T, csize, serial):
    st.lib.stenos_hip_test_walk(st.ctx, 1 if serial else 0)
    try:
        return st.frame_index(frame, T, csize)
    except StenosError:
        return None
    finally:
        st.lib.stenos_hip_test_walk(st.ctx, 0)


def _walks_agree(st, frame, T, csize, encoder_index):
    par = _walked(st, frame, T, csize, serial=False)
    fell_back = st.lib.stenos_hip_test_walk(st.ctx, 0)
    ser = _walked(st, frame, T, csize, serial=True)
    assert par is not None and ser is not None
    assert par == ser, "the parallel walk and the serial walk differ"
    assert fell_back == 0, "a well-formed frame needed the serial walk"
    assert par == encoder_index, "the walk and the encoder's index differ"


@pytest.mark.parametrize("name", ["A", "B"])
def test_index_and_walk(both, name):
    big = both[name]
    _walks_agree(big.st, big.frame, big.T, big.csize, big.index)


def test_round_trip_without_an_index(B):
    back = torch.zeros(B.total, dtype=torch.uint8, device="cuda")
    assert B.st.decompress(B.frame, B.T, B.csize, back) == B.total
    _same(back, B.src, B.crossings, "B decoded without an index")


# ---- 2. frame bytes at high offsets against the oracle ----------------------------------------------------------------------

@pytest.mark.parametrize("name", ["A", "B"])
def test_superblock_bytes_equal_the_oracles(both, name, oracle):
    """a superblock's bytes do not depend on where it stands: the oracle compresses its source bytes as an array of their own, and
    what follows the 8-byte frame header is frame[index[k] : index[k + 1]]"""
    big = both[name]
    if name == "A":
        ks = [P31 // SB, big.kf, P32 // SB, big.nsb - 2, big.nsb - 1]
    else:
        ks = [big.first_walk, big.nsb - 1]
    for k in ks:
        lo = k * big.sb
        data = _host(big.src, lo, min(big.sb, big.total - lo))
        r, ref = oracle_compress(oracle, data, big.T, 1)
        got = _host(big.frame, big.index[k], big.index[k + 1] - big.index[k])
        assert r - 8 == got.size, (name, k, r - 8, got.size)
        assert np.array_equal(got, ref[8:]), (name, k, "first differing byte", int(np.flatnonzero(got != ref[8:])[0]))


# ---- 3. ranges -------------------------------------------------------------------------------------------------------------

def _crossing_ranges(big):
    r = [(P32 - 3, 7)]
    for c in big.crossings:
        for n in (1, 7, 4096, big.sb + 5):
            r += [(c - n, n), (c, n), (c - (n + 1) // 2, n)]  # ends just below, starts on it, straddles it (n = 1: the byte below)
    r = [(lo, min(n, big.total - lo)) for lo, n in r if 0 <= lo < big.total]
    r += [(big.total - 1, 1), (big.total, 0), (1, big.total - 2)]
    assert all(lo + n <= big.total for lo, n in r) and r[-1][1] > P32
    return r


class Carved:
    """destinations out of one buffer at odd addresses, 64 sentinel bytes of 0xA5 between them and at both ends; `want` is the
    image the buffer must equal after the call"""

    def __init__(self, ranges, src):
        self.at, pos = [], GUARD
        for i, (_, n) in enumerate(ranges):
            pos = (pos + 15) // 16 * 16 + 2 * (i % 8) + 1
            self.at.append(pos)
            pos += n + GUARD
        self.size = pos + 16
        self.ranges = ranges
        self.want = torch.full((self.size,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
        for (lo, n), a in zip(ranges, self.at):
            _copy_in_chunks(self.want[a:a + n], src[lo:lo + n])
        # (the sentinels of the image itself, read back: the fill and the copies above are torch's)
        edge = 0
        for (_, n), a in zip(ranges, self.at):
            _all_guard(self.want[edge:a], "the expected image")
            edge = a + n
        _all_guard(self.want[edge:], "the expected image")

    def fresh(self):
        buf = torch.full((self.size,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % 16 == 0
        return buf, [buf.data_ptr() + a for a in self.at]


@pytest.mark.parametrize("name", ["A", "B"])
def test_ranges(both, name):
    big = both[name]
    ranges = _crossing_ranges(big)
    c = Carved(ranges, big.src)
    big_at, (big_lo, _) = c.at[-1], ranges[-1]
    points = [a for a in c.at] + [big_at + (x - big_lo) for x in big.crossings]
    for index_ptr in (big.index_ptr, None):
        buf, ptrs = c.fresh()
        assert big.st.decompress_ranges(big.frame, big.T, big.csize, ranges, ptrs, index_ptr) == sum(n for _, n in ranges)
        _same(buf, c.want, points, f"{name}: ranges with{'' if index_ptr else 'out'} an index")  # (every sentinel is part of the image)
        del buf


# ---- 4. gather --------------------------------------------------------------------------------------------------------------

def _gather_small(big, row_bytes, rows, index_ptr, stride=None, mis=5, skip=(), expect=None):
    """a handful of rows into slots `stride` apart, `mis` bytes behind a 256-byte boundary, in a buffer of 0xA5 that is compared
    whole on the host; skip: slots that must stay untouched (invalid rows; the other slots are then not looked at)"""
    stride = stride or row_bytes
    n, at = len(rows), 256 + mis
    buf = torch.full((at + (n - 1) * stride + row_bytes + GUARD + 16,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
    r = _code(lambda: big.st.gather_rows(big.frame, big.T, big.csize, row_bytes, _rows_tensor(rows), buf.data_ptr() + at, index_ptr, stride))
    assert r == (n * row_bytes if expect is None else expect), (big.name, row_bytes, rows, hex(r))
    got = buf.cpu().numpy()
    want = np.full_like(got, GUARD_BYTE)
    for i, row in enumerate(rows):
        a = at + i * stride
        if i in skip:
            continue
        if skip:  # (a failed call: what the valid slots hold is unspecified)
            want[a:a + row_bytes] = got[a:a + row_bytes]
        else:
            want[a:a + row_bytes] = _host(big.src, row * row_bytes, row_bytes)
    if not np.array_equal(got, want):
        bad = int(np.flatnonzero(got != want)[0])
        raise AssertionError(f"{big.name}: row_bytes {row_bytes}, stride {stride}: byte {bad} of the buffer differs, slot {(bad - at) // stride}, rows {rows}")


def _crossing_rows(big, row_bytes):
    nrows = big.total // row_bytes
    rows = []
    for c in big.crossings:
        rows += [r for r in (c // row_bytes - 1, c // row_bytes, c // row_bytes + 1) if 0 <= r < nrows]
    assert any(r * row_bytes < c < (r + 1) * row_bytes for r in rows for c in big.crossings if c % row_bytes)
    return rows + [nrows - 1]


@pytest.mark.parametrize("name", ["A", "B"])
def test_gather_single_bytes_by_64_bit_row_numbers(both, name):
    big = both[name]
    rows = [P32 - 1, P32, big.total - 1, 0, P31]
    _gather_small(big, 1, rows, big.index_ptr)
    _gather_small(big, 1, rows, None, stride=1 + 64 + 3)


@pytest.mark.parametrize("row_bytes", [4101, SB + 5])
@pytest.mark.parametrize("name", ["A", "B"])
def test_gather_rows_that_straddle_the_crossings(both, name, row_bytes):
    big = both[name]
    rows = _crossing_rows(big, row_bytes)
    _gather_small(big, row_bytes, rows, big.index_ptr, stride=row_bytes + 64 + 3)
    _gather_small(big, row_bytes, rows, None, mis=0)


def test_gather_slots_two_gib_apart(A):
    """i * dst_stride passes 2^32 at the third slot; the 4 GiB between and around the slots must stay as they were"""
    row_bytes, stride, at = 4101, P31 + 8, 256 + 5
    rows = [A.kf * SB // row_bytes, P32 // row_bytes, P31 // row_bytes]
    buf = torch.full((at + 2 * stride + row_bytes + GUARD + 16,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
    assert A.st.gather_rows(A.frame, A.T, A.csize, row_bytes, _rows_tensor(rows), buf.data_ptr() + at, A.index_ptr, stride) == 3 * row_bytes
    edge = 0
    for i, row in enumerate(rows):
        a = at + i * stride
        assert np.array_equal(_host(buf, a, row_bytes), _host(A.src, row * row_bytes, row_bytes)), (i, row)
        _all_guard(buf[edge:a], f"the gap in front of slot {i}")
        assert (_host(buf, max(0, a - WINDOW), min(a, WINDOW)) == GUARD_BYTE).all() and (_host(buf, a + row_bytes, GUARD) == GUARD_BYTE).all(), i
        edge = a + row_bytes
    _all_guard(buf[edge:], "the bytes behind the last slot")


def test_gather_more_than_4_gib_of_rows(A):
    """2^20 + 3 rows of 4 KiB, with repeats, numbered on the stream by torch: the output passes 2^32 bytes, the piece count 2^20.
    The expected rows come from chunks of at most 1 GiB of the source and of the output, as int64 words: no index_select ever
    sees 2^31 elements."""
    row_bytes, n = 4096, (1 << 20) + 3
    nrows = A.total // row_bytes
    g = torch.Generator(device="cuda")
    g.manual_seed(4)
    rows = torch.randint(0, nrows, (n,), dtype=torch.int64, device="cuda", generator=g)
    rows[:6] = torch.tensor([P31 // row_bytes - 1, P31 // row_bytes, A.kf * SB // row_bytes, P32 // row_bytes - 1, P32 // row_bytes, nrows - 1], device="cuda")
    rows[-1] = rows[0]
    out = torch.empty(n * row_bytes, dtype=torch.uint8, device="cuda")
    assert out.numel() > P32
    assert A.st.gather_rows(A.frame, A.T, A.csize, row_bytes, rows, out, A.index_ptr) == n * row_bytes  # (no synchronisation in front: same stream)
    assert len(torch.unique(rows)) < n, "the rows were meant to repeat"
    words = row_bytes // 8
    src_rows = A.src[:nrows * row_bytes].view(torch.int64).view(nrows, words)
    got_rows = out.view(torch.int64).view(n, words)
    per = GIB // row_bytes
    for i0 in range(0, n, per):
        r = rows[i0:i0 + per]
        want = torch.full((r.numel(), words), -1, dtype=torch.int64, device="cuda")
        filled = 0
        for r0 in range(0, nrows, per):
            at = ((r >= r0) & (r < r0 + per)).nonzero().squeeze(1)
            want[at] = src_rows[r0:r0 + per][r[at] - r0]
            filled += at.numel()
        assert filled == r.numel()
        assert torch.equal(got_rows[i0:i0 + per], want), f"slots {i0}.. differ"
        del want
    host_rows = rows.cpu().tolist()
    for i in (0, 1, 2, 3, 4, 5, (1 << 19) + 1, (1 << 20) - 1, 1 << 20, n - 2, n - 1):  # (slot 2^20 starts at output byte 2^32)
        assert np.array_equal(_host(out, i * row_bytes, row_bytes), _host(A.src, host_rows[i] * row_bytes, row_bytes)), (i, host_rows[i])


def test_gather_invalid_rows_among_valid_ones(A):
    row_bytes = 4101
    nrows = A.total // row_bytes
    good = _crossing_rows(A, row_bytes)
    for bad in (nrows, 1 << 63):
        rows = good[:3] + [bad] + good[3:]
        _gather_small(A, row_bytes, rows, A.index_ptr, stride=row_bytes + 64 + 3, skip=(3,), expect=INVALID_PARAMETER)
    _gather_small(A, row_bytes, good[:2] + [nrows, good[2], 1 << 63] + good[3:], None, skip=(2, 4), expect=INVALID_PARAMETER)


# ---- 5. update --------------------------------------------------------------------------------------------------------------

def _update_checked(big, row_bytes, rows, src_buf, stride, hooks_lib):
    """Rows `rows` (unique) replaced by src_buf[i * stride : i * stride + row_bytes]: the output frame is, in size and byte for
    byte, stenos_hip_compress of the updated source; the context's index afterwards is that compression's; the output decodes to
    the updated source; nothing is written behind the returned size.  The updated source is big.src itself with the rows written
    by slice assignment, put back afterwards (a second copy of 4 GiB is not affordable next to the reference compression)."""
    st, T, total = big.st, big.T, big.total
    assert len(set(rows)) == len(rows)
    saved = [big.src[r * row_bytes:(r + 1) * row_bytes].clone() for r in rows]
    ref = Stenos(1, lib=hooks_lib)
    try:
        for i, r in enumerate(rows):
            big.src[r * row_bytes:(r + 1) * row_bytes] = src_buf[i * stride:i * stride + row_bytes]
        want = torch.empty(ref.bound(total), dtype=torch.uint8, device="cuda")
        want_size = ref.compress(big.src, T, want)
        p, nsb = ref.last_index()
        assert p and nsb == big.nsb
        want_index, _ = _index_of(p, nsb)
        touched = sorted({s for r in rows for s in range(r * row_bytes // big.sb, ((r + 1) * row_bytes - 1) // big.sb + 1)})
        assert len(touched) <= 2 * len(rows)
        at, cap = 256 + 5, big.csize + len(touched) * (big.sb + 4) + 4096  # (a touched superblock grows to a copy at the most)
        buf = torch.full((at + cap + GUARD + 16,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
        out = buf[at:at + cap]
        r = st.update_rows(big.frame, T, big.csize, row_bytes, _rows_tensor(rows), src_buf.data_ptr(), out, big.index_ptr, stride)
        assert r == want_size, (big.name, r, want_size)
        points = [p for p in (P31, P32) if p < r] + [want_index[s] for s in touched] + [want_index[s + 1] for s in touched]
        _same(out[:r], want[:r], points, f"{big.name}: the updated frame against the compression of the updated array")
        _all_guard(buf[:at], "the bytes in front of d_out")
        _all_guard(buf[at + r:], "the bytes behind the returned size")
        lp, ln = st.last_index()
        assert lp and ln == nsb
        assert _index_of(lp, ln)[0] == want_index, "the context's index after the update is not the new frame's"
        del want
        _free_cache()
        back = torch.zeros(total, dtype=torch.uint8, device="cuda")
        assert st.decompress(out, T, r, back, lp) == total
        _same(back, big.src, big.crossings + [r * row_bytes for r in rows], f"{big.name}: the decoded update")
        del back, buf, out
    finally:
        for r, s in zip(rows, saved):
            big.src[r * row_bytes:(r + 1) * row_bytes] = s
        ref.close()
        _free_cache()
    # (the input frame is as it was: its superblocks at the crossings still decode to the restored source)
    probe = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    for c in big.crossings:
        lo = min(c - 2048, total - 4096)
        assert st.decompress_range(big.frame, T, big.csize, lo, 4096, probe, big.index_ptr) == 4096
        assert np.array_equal(probe.cpu().numpy(), _host(big.src, lo, 4096)), c


def _noise(n, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda", generator=g)


def test_update_rows_at_the_crossings_of_A(A, hooks_lib):
    row_bytes = 4101
    nrows = A.total // row_bytes
    rows = sorted(set(_crossing_rows(A, row_bytes)))
    rng = np.random.default_rng(51)
    while len(rows) < 64:  # (the others inside the superblocks already touched, and in a few more)
        r = int(rng.choice(rows)) + int(rng.integers(-40, 41))
        if 0 <= r < nrows and r not in rows:
            rows.append(r)
    rows = [int(r) for r in rng.permutation(rows)]
    assert len(rows) == 64 and nrows - 1 in rows
    _update_checked(A, row_bytes, rows, _noise(64 * row_bytes, 52), row_bytes, hooks_lib)


def test_update_source_rows_two_gib_apart(A, hooks_lib):
    """i * src_stride passes 2^32 at the third row"""
    row_bytes, stride = 4101, P31 + 8
    rows = [P32 // row_bytes, A.kf * SB // row_bytes, P31 // row_bytes]
    src_buf = torch.zeros(2 * stride + row_bytes, dtype=torch.uint8, device="cuda")
    for i in range(3):
        src_buf[i * stride:i * stride + row_bytes] = _noise(row_bytes, 53 + i)
    _update_checked(A, row_bytes, rows, src_buf, stride, hooks_lib)


def test_update_rows_behind_frame_offset_2_32_of_B(B, hooks_lib):
    row_bytes = 4101
    lo, hi = -(-P32 // row_bytes), (P32 + 8 * SB) // row_bytes  # the rows wholly inside the walk superblocks
    rng = np.random.default_rng(54)
    rows = [lo, hi - 1] + [int(r) for r in lo + 1 + rng.permutation(hi - lo - 2)[:10]] + [5, P31 // row_bytes]
    assert all(B.index[r * row_bytes // SB] > P32 for r in rows[:-2])
    _update_checked(B, row_bytes, rows, _noise(len(rows) * row_bytes, 55) & 0x0F, row_bytes, hooks_lib)  # (nibbles: the superblocks stay coded)


# ---- 6. batch ---------------------------------------------------------------------------------------------------------------

def test_batch_of_more_than_4_gib(A, hooks_lib):
    """A's source cut at superblock boundaries into 9 unequal items: the batch kernels address all of them through one prefix
    of blocks and superblocks, which passes 2^32 bytes inside the last item"""
    T = A.T
    counts = [3641, 3643, 3639, 3645, 3637, 3647, 3635, 3649]
    cuts = [0] + list(np.cumsum(counts)) + [A.nsb]
    bounds = [(int(a) * SB, min(int(b) * SB, A.total)) for a, b in zip(cuts, cuts[1:])]
    assert len(bounds) == 9 and bounds[-1][1] == A.total and len({b - a for a, b in bounds}) == 9
    holder = [k for k, (a, b) in enumerate(bounds) if a <= P32 - 1 < b]
    assert holder == [8] and bounds[8][0] > 0
    st = Stenos(1, lib=hooks_lib)
    try:
        srcs = [A.src[a:b] for a, b in bounds]
        dsts = [torch.empty(st.bound(b - a), dtype=torch.uint8, device="cuda") for a, b in bounds]
        res = st.compress_batch(srcs, T, dsts)
        single = torch.empty(max(d.numel() for d in dsts), dtype=torch.uint8, device="cuda")
        for k, (a, b) in enumerate(bounds):
            r = st.compress(srcs[k], T, single[:dsts[k].numel()])
            assert res[k] == r, (k, hex(res[k]), r)
            k0, k1 = a // SB, -(-b // SB)
            points = [A.index[k0 + 1] - A.index[k0] + 8, r - (A.index[k1] - A.index[k1 - 1])]  # the ends of its first and the start of its last superblock
            _same(dsts[k][:r], single[:r], points, f"item {k}: batch frame against the single call's")
            # (and both are the whole array's frame between the item's superblocks, behind the 8-byte header)
            _same(dsts[k][8:r], A.frame[A.index[k0]:A.index[k1]], [], f"item {k}: batch frame against A's frame")
        del single
        outs = [torch.zeros(b - a, dtype=torch.uint8, device="cuda") for a, b in bounds]
        back = st.decompress_batch(dsts, T, res, outs)
        for k, (a, b) in enumerate(bounds):
            assert back[k] == b - a, (k, hex(back[k]))
            _same(outs[k], srcs[k], [SB, (b - a) // SB * SB, P32 - a] if k == 8 else [SB], f"item {k}: decoded batch")
        # the item that holds the 2^32-th byte, on the host: its first and its last superblock, decoded and as frame bytes
        a, b = bounds[8]
        for lo, n in ((0, SB), ((b - a) // SB * SB, (b - a) % SB)):
            assert np.array_equal(_host(outs[8], lo, n), _host(A.src, a + lo, n)), lo
        k0, k1 = a // SB, A.nsb
        assert np.array_equal(_host(dsts[8], 8, A.index[k0 + 1] - A.index[k0]), _host(A.frame, A.index[k0], A.index[k0 + 1] - A.index[k0]))
        last = A.index[k1] - A.index[k1 - 1]
        assert np.array_equal(_host(dsts[8], res[8] - last, last), _host(A.frame, A.index[k1 - 1], last))
        del outs, dsts
    finally:
        st.close()


# ---- 7. the host ABI, once ----------------------------------------------------------------------------------------------------

def test_host_pointer_calls_once(A, hooks_lib):
    """the only array-sized PCIe traffic of the file: A to the host, through stenos_compress_generic and back"""
    t0 = time.perf_counter()
    data = A.src.cpu().numpy()
    frame = A.frame.cpu().numpy()
    t1 = time.perf_counter()
    st = Stenos(1, lib=hooks_lib)
    try:
        cap = st.bound(A.total)
        dst = np.empty(cap, dtype=np.uint8)
        r = st.lib.stenos_compress_generic(st.ctx, data.ctypes.data, A.T, A.total, dst.ctypes.data, cap)
        t2 = time.perf_counter()
        assert r == A.csize, (hex(r), A.csize)
        for o in range(0, r, GIB):
            assert np.array_equal(dst[o:o + GIB][:r - o], frame[o:o + GIB]), f"the host frame differs from the device frame in [{o}, {o + GIB})"
        back = np.empty(A.total, dtype=np.uint8)
        t3 = time.perf_counter()
        assert st.lib.stenos_decompress_generic(st.ctx, dst.ctypes.data, A.T, r, back.ctypes.data, A.total) == A.total
        t4 = time.perf_counter()
        for o in range(0, A.total, GIB):
            assert np.array_equal(back[o:o + GIB], data[o:o + GIB]), f"the decoded array differs in [{o}, {o + GIB})"
        for p in A.crossings:
            assert np.array_equal(back[p - WINDOW:p + WINDOW], _host(A.src, p - WINDOW, 2 * WINDOW)), p
        print(f"\nhost ABI on A: downloads {t1 - t0:.2f} s, stenos_compress_generic {t2 - t1:.2f} s, stenos_decompress_generic {t4 - t3:.2f} s")
    finally:
        st.close()


# ---- 8. many superblocks ------------------------------------------------------------------------------------------------------

def test_more_than_a_million_superblocks(room, hooks_lib):
    """stenos_set_block_size(ctx, 0): superblocks of one block, 1 KiB for 32-bit elements -- 2^20 + 1 of them in 1 GiB + 1003 bytes"""
    T, sb, total = 4, 1024, GIB + 1003
    src = generate_torch("rand12", T, total // T + 1, 31)[:total].clone()
    nsb = -(-total // sb)
    assert nsb > 1 << 20
    st, ref = Stenos(1, lib=hooks_lib), Stenos(1, lib=hooks_lib)
    try:
        for s in (st, ref):
            assert s.lib.stenos_set_block_size(s.ctx, 0) == 0
        cap = st.bound(total) + 4 * (nsb + 2) + 16  # (stenos_bound counts default superblocks)
        frame = torch.empty(cap, dtype=torch.uint8, device="cuda")
        csize = st.compress(src, T, frame)
        p, n = st.last_index()
        assert p and n == nsb
        index, index_dev = _index_of(p, nsb)
        print(f"\n{nsb} superblocks of {sb} bytes, frame {csize} bytes")
        _walks_agree(st, frame, T, csize, index)
        back = torch.zeros(total, dtype=torch.uint8, device="cuda")
        assert st.decompress(frame, T, csize, back) == total
        _same(back, src, [total - 1003], "decoded without an index")
        del back
        rng = np.random.default_rng(32)
        # ranges: 1000 pieces of up to 5000 bytes (up to six superblocks each), into one buffer with sentinels between them
        ranges = [(int(lo), int(min(total - lo, rng.integers(1, 5001)))) for lo in rng.integers(0, total, 998)] + [(total - 1, 1), (0, sb + 1)]
        c = Carved(ranges, src)
        for index_ptr in (index_dev.data_ptr(), None):
            buf, ptrs = c.fresh()
            assert st.decompress_ranges(frame, T, csize, ranges, ptrs, index_ptr) == sum(k for _, k in ranges)
            assert np.array_equal(buf.cpu().numpy(), c.want.cpu().numpy())
        # gather: 1000 rows of 300 bytes
        rb = 300
        rows = [int(r) for r in rng.integers(0, total // rb, 998)] + [total // rb - 1, 0]
        at = 256 + 5
        buf = torch.full((at + 1000 * rb + GUARD + 16,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
        assert st.gather_rows(frame, T, csize, rb, _rows_tensor(rows), buf.data_ptr() + at, index_dev.data_ptr()) == 1000 * rb
        want = np.full(buf.numel(), GUARD_BYTE, dtype=np.uint8)
        host = src.cpu().numpy()
        for i, r in enumerate(rows):
            want[at + i * rb:at + (i + 1) * rb] = host[r * rb:(r + 1) * rb]
        assert np.array_equal(buf.cpu().numpy(), want)
        # update: 16 rows against the compression of the updated array
        urows = [int(r) for r in rng.permutation(total // rb)[:14]] + [total // rb - 1, (total // 2) // rb]
        assert len(set(urows)) == 16
        new = _noise(16 * rb, 33)
        upd = src.clone()
        for i, r in enumerate(urows):
            upd[r * rb:(r + 1) * rb] = new[i * rb:(i + 1) * rb]
        want_frame = torch.empty(cap, dtype=torch.uint8, device="cuda")
        want_size = ref.compress(upd, T, want_frame)
        wp, wn = ref.last_index()
        want_index, _ = _index_of(wp, wn)
        obuf = torch.full((at + cap + GUARD + 16,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
        out = obuf[at:at + cap]
        r = st.update_rows(frame, T, csize, rb, _rows_tensor(urows), new, out, index_dev.data_ptr())
        assert r == want_size
        _same(out[:r], want_frame[:r], [want_index[x * rb // sb] for x in urows], "the updated frame")
        _all_guard(obuf[:at], "the bytes in front of d_out")
        _all_guard(obuf[at + r:], "the bytes behind the returned size")
        lp, ln = st.last_index()
        assert ln == nsb and _index_of(lp, ln)[0] == want_index
        back = torch.zeros(total, dtype=torch.uint8, device="cuda")
        assert st.decompress(out, T, r, back) == total
        _same(back, upd, [x * rb for x in urows], "the decoded update")
    finally:
        st.close()
        ref.close()
