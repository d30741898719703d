// range_codec.h -- decoding a byte window [lo, hi) of one BLOCK superblock (code 1) by one wavefront, for decode_ranges
// (range_decode_kernels.hip, stenos_hip_decompress_ranges).  Written in the wavevec.h vocabulary, so the host emulation
// in tests/emul_ranges runs the same code.
//
// The blocks of a payload form a chain: where a block ends is only known once it has been parsed, so the walk starts at
// block 0 whatever lo is.  Blocks are decoded into the LDS image (decode_block without a place in HBM), the part of the
// image that lies inside the window is stored with predicated stores, and the walk ends with the block that holds byte
// hi - 1: nothing behind it is read or checked.  A copied block wholly in front of lo is stepped over after its length check.
// Nothing in here branches on a lane-dependent value (wavevec.h, "Predicated memory accesses without a branch").
#pragma once
#include "superblock_codec.h"

namespace codec {

// Image bytes [a, b) (offsets from the image's start, a < b) -> g[0, b - a), any alignment of g: the image is read in its
// aligned 16-byte groups, the bytes in front of the first whole group and behind the last one go out as single bytes.
// Never writes outside [g, g + b - a).
WV_FN void store_image_window(uint8_t* g, Lds lds, uint32_t img, uint32_t a, uint32_t b)
{
	const U32 lane = lane_id();
	const uint32_t up = (a + 15u) & ~15u;
	const uint32_t a16 = up < b ? up : b; // end of the ragged head
	const uint32_t down = b & ~15u;
	const uint32_t b16 = down > a16 ? down : a16; // start of the ragged tail
	{
		Pred p = lane < U32(a16 - a);
		gst8(g, lane, lds_ld8(lds, U32(img + a) + sel(p, lane, U32(0u))), p);
	}
	const uint32_t groups = (b16 - a16) >> 4;
	uint8_t* mid = g + (a16 - a);
	for (uint32_t o = 0; o < groups; o += 64) {
		const U32 k = U32(o) + lane;
		Pred p = k < U32(groups);
		gst128_unaligned(mid, k * 16u, lds_ld128(lds, U32(img + a16) + sel(p, k, U32(0u)) * 16u), p);
	}
	{
		Pred p = lane < U32(b - b16);
		gst8(g + (b16 - a), lane, lds_ld8(lds, U32(img + b16) + sel(p, lane, U32(0u))), p);
	}
}

// Bytes [lo, hi) of the superblock whose payload is `csize` bytes at src and which decodes to dsize bytes
// (0 <= lo < hi <= dsize) -> dst[0, hi - lo).  Returns hi - lo, or DEC_ERROR under the conditions of decode_superblock
// (superblock_codec.h) for the blocks up to the one that holds byte hi - 1; the blocks behind it are not looked at.
WV_FN uint32_t decode_superblock_window(Lds lds, const DecLayout& L, uint32_t T, const uint8_t* src, uint32_t csize, uint32_t dsize, uint32_t lo, uint32_t hi,
					uint8_t* dst)
{
	const U32 lane = lane_id_plain();
	const uint32_t bs = 256 * T, hs = header_bytes(T);
	if (dsize == 0 || csize == 0)
		return 0;
	const uint32_t nblocks = dsize / bs;
	if (csize < hs + T && nblocks) // block_compress.h:1813-1815
		return DEC_ERROR;
	dec_write_lut(lds, L);
	const uint32_t wcap = window_bytes(T);
	const uint32_t mis = (uint32_t)((uintptr_t)src & 15u); // the window is filled from the 16-byte aligned address below src
	const uint8_t* abase = src - mis;
	uint32_t wstart = 0, wfill = 0, wend = 0; // window holds abase[wstart, wend), wend = wstart + wfill
	uint32_t consumed = 0;          // payload bytes consumed so far

	// (decode_superblock's: the window only moves forward; a block that was stepped over may lie behind its end, then nothing is kept)
	auto ensure = [&](uint32_t need) {
		uint32_t a = consumed + mis;
		if (a >= wstart && a + need <= wend)
			return;
		const uint32_t nstart = a & ~15u;
		const uint32_t endoff = csize + mis;
		const uint32_t nfill = endoff - nstart < wcap ? endoff - nstart : wcap;
		uint32_t keep = 0;
		if (wfill && nstart >= wstart && nstart < wstart + wfill && ((wstart + wfill) & 15u) == 0) {
			keep = wstart + wfill - nstart;
			const uint32_t d = nstart - wstart;
			for (uint32_t o = 0; o < keep; o += 1024) {
				U32 off = U32(o) + lane * 16u;
				Pred p = off < U32(keep);
				U128 v = lds_ld128(lds, U32(L.win + d) + sel(p, off, U32(0u)));
				wave_sync();
				lds_st128(lds, U32(L.win) + off, v, p);
				wave_sync();
			}
		}
		wstart = nstart;
		wfill = nfill;
		wend = nstart + nfill;
		if (nfill > keep)
			copy_g2l(lds, L.win + keep, abase + wstart + keep, nfill - keep);
		wave_sync();
	};

	const uint32_t last = (hi - 1u) / bs; // the block that holds byte hi - 1 (nblocks: the tail)
	for (uint32_t b = 0; b < nblocks && b <= last; ++b) {
		const uint32_t at = b * bs;
		const uint32_t left = csize - consumed;
		const uint32_t need = left < max_stream_block_bytes(T) ? left : max_stream_block_bytes(T);
		if (at + bs <= lo && left) { // wholly in front of the window: a copied block needs its length checked, not its bytes
			ensure(1);
			if (win_u8(lds + L.win, consumed + mis - wstart) == BLOCK_COPY) {
				if (left < 1 + bs)
					return DEC_ERROR;
				consumed += 1 + bs;
				continue;
			}
		}
		ensure(need);
		const uint32_t n = decode_block(lds, L, T, consumed + mis - wstart, need, 16, true);
		if (n == DEC_ERROR)
			return DEC_ERROR;
		if (at + bs > lo) { // (every predicated store is waited for, wavevec.h)
			const uint32_t a = (lo > at ? lo : at) - at, e = (hi < at + bs ? hi : at + bs) - at;
			store_image_window(dst + (at + a - lo), lds, L.img, a, e);
			wave_sync();
		}
		consumed += n;
	}
	const uint32_t tail = dsize - nblocks * bs, tb = nblocks * bs;
	if (tail && hi > tb) { // [254] + partial block, as in decode_superblock
		if (consumed == csize)
			return DEC_ERROR;
		const uint32_t left = csize - consumed;
		const uint32_t need = left < max_stream_tail_bytes(T) ? left : max_stream_tail_bytes(T);
		ensure(need);
		const uint32_t cur = consumed + mis - wstart;
		if (win_u8(lds + L.win, cur) != BLOCK_PARTIAL)
			return DEC_ERROR;
		const uint32_t lines = tail / (16 * T);
		uint32_t n = 0;
		if (lines) {
			n = decode_block(lds, L, T, cur + 1, need - 1, lines, false);
			if (n == DEC_ERROR)
				return DEC_ERROR;
		}
		const uint32_t rem = tail - lines * 16 * T;
		if (1 + n + rem > need)
			return DEC_ERROR;
		for (uint32_t o = 0; o < rem; o += 64) {
			Pred p = (U32(o) + lane) < U32(rem);
			U32 v = lds_ld8(lds + L.win, U32(cur + 1 + n + o) + sel(p, lane, U32(0u)));
			lds_st8(lds, U32(L.img + lines * 16 * T + o) + lane, v, p);
		}
		wave_sync();
		const uint32_t a = (lo > tb ? lo : tb) - tb;
		store_image_window(dst + (tb + a - lo), lds, L.img, a, hi - tb);
	}
	return hi - lo;
}

} // namespace codec
