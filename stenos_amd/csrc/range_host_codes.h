// range_host_codes.h -- internal to the host side: finishing pieces of superblocks that went through zstd (codes 2-5) one by
// one, for the calls that deliver parts of a frame (range_host.cpp, gather_host.cpp, update_host.cpp).  A piece is a RangeUnit {superblock,
// lo, hi, dst}; the superblock is fetched and inflated on the host, then the piece is copied out (code 2), cut out of the
// superblock as the byte kernels rebuild it (codes 3, 4), or decoded by a one-unit launch of decode_ranges over the inflated
// block stream (code 5).  Consecutive pieces of one superblock share the fetch and the inflation.  Slow.
// Behind it the tail both gather calls end with (gather_host.cpp, gather_batch_host.cpp): finish_flagged_pieces.
#pragma once
#include <algorithm>

#include "frame_access.h"
#include "range.h"

namespace stenos_host {

struct HostCodes {
	stenos_context_s* ctx;
	const uint8_t* d_frame;
	size_t size, T;
	const uint64_t* d_index;
	FrameInfo fi;
	hipStream_t stream;
	uint8_t* h_tab; // 128 bytes, page-locked: the words and the unit of a one-unit launch (code 5) ...
	uint8_t* d_tab; // ... and their place on the device
	// the superblock the buffers hold: inflated bytes at h_stage + 16 (codes 2 and 5), decoded bytes in rsb (codes 3 and 4)
	uint64_t have_sb = ~0ull;
	unsigned have_code = 0;
	size_t have_bytes = 0;

	// the one-unit tables: 128 bytes at o_one of rtab and its mirror, which the caller has made large enough
	HostCodes(stenos_context_s* c, const void* frame, size_t frame_size, size_t bytesoftype, const uint64_t* index, const FrameInfo& info, hipStream_t s, size_t o_one = 0)
		: ctx(c), d_frame((const uint8_t*)frame), size(frame_size), T(bytesoftype), d_index(index), fi(info), stream(s), h_tab(c->h_rtab.data() + o_one),
		  d_tab(c->rtab.as<uint8_t>() + o_one)
	{
	}
	bool copy(void* to, const void* from, size_t n, hipMemcpyKind kind) const
	{
		return hipMemcpyAsync(to, from, n, kind, stream) == hipSuccess && hipStreamSynchronize(stream) == hipSuccess;
	}
	// fetch and inflate superblock s; 0 or an error code
	size_t load(uint64_t s)
	{
		if (s == have_sb)
			return 0;
		have_sb = ~0ull;
		const size_t dsize = superblock_bytes(fi.total, fi.sb, s);
		uint64_t p = 0;
		uint8_t hd[4];
		if (!copy(&p, d_index + s, 8, hipMemcpyDeviceToHost))
			return STENOS_ERROR_UNDEFINED;
		if (p > size || size - p < 4)
			return STENOS_ERROR_SRC_OVERFLOW;
		if (!copy(hd, d_frame + p, 4, hipMemcpyDeviceToHost))
			return STENOS_ERROR_UNDEFINED;
		const unsigned code = hd[0];
		const size_t csize = (size_t)get_le(hd + 1, 3);
		if (code < 2 || code > 5 || size - p - 4 < csize)
			return STENOS_ERROR_INVALID_INPUT;
		if (!ctx->h_in.ensure(csize + 64) || !ctx->h_stage.ensure(fi.sb + 64 + 32) || !ctx->tmp1.ensure(fi.sb + 64 + 32) || !ctx->tmp2.ensure(fi.sb + 64) ||
		    !ctx->rsb.ensure(fi.sb + 64))
			return STENOS_ERROR_ALLOC;
		if (csize && !copy(ctx->h_in.data(), d_frame + p + 4, csize, hipMemcpyDeviceToHost))
			return STENOS_ERROR_UNDEFINED;
		uint8_t* const hs = ctx->h_stage.data();
		// code 5: zstd over the block stream, at most the superblock size (stenos.cpp:732)
		const size_t r = zstd().decompress(hs + 16, code == 5 ? fi.sb + 64 : dsize, ctx->h_in.data(), csize);
		if (zstd().is_error(r) || (code != 5 && code != 2 && r != dsize)) // stenos.cpp:696-698, 706-708, 718-720
			return STENOS_ERROR_INVALID_INPUT;
		if (code == 3 || code == 4) { // transposed (stenos.cpp:700-710) / transposed + byte delta (:711-725) -> rsb
			uint8_t* const t1 = ctx->tmp1.as<uint8_t>();
			uint8_t* const t2 = ctx->tmp2.as<uint8_t>();
			bool ok = hipMemcpyAsync(t1, hs + 16, dsize, hipMemcpyHostToDevice, stream) == hipSuccess;
			if (code == 4)
				ok = ok && stenos_k_launch_delta(t1, t2, dsize, true, stream) == hipSuccess;
			ok = ok && stenos_k_launch_shuffle(code == 4 ? t2 : t1, ctx->rsb.as<uint8_t>(), (uint32_t)T, dsize, true, stream) == hipSuccess;
			if (!ok || hipStreamSynchronize(stream) != hipSuccess)
				return STENOS_ERROR_UNDEFINED;
		}
		else if (code == 5) { // -> one BLOCK superblock for the block decoder (stenos.cpp:726-740), its payload 16-byte aligned
			write_superblock_header(hs + 12, 1, r);
			if (!copy(ctx->tmp1.as<uint8_t>() + 12, hs + 12, 4 + r, hipMemcpyHostToDevice))
				return STENOS_ERROR_UNDEFINED;
		}
		have_sb = s;
		have_code = code;
		have_bytes = r;
		return 0;
	}
	size_t finish(const RangeUnit& u)
	{
		if (size_t e = load(u.sb))
			return e;
		const size_t len = u.hi - u.lo;
		if (have_code == 2) { // plain zstd
			if (u.hi > have_bytes)
				return STENOS_ERROR_INVALID_INPUT;
			return copy(u.dst, ctx->h_stage.data() + 16 + u.lo, len, hipMemcpyHostToDevice) ? 0 : (size_t)STENOS_ERROR_UNDEFINED;
		}
		if (have_code != 5)
			return copy(u.dst, ctx->rsb.as<uint8_t>() + u.lo, len, hipMemcpyDeviceToDevice) ? 0 : (size_t)STENOS_ERROR_UNDEFINED;
		uint8_t* const h = h_tab;
		uint8_t* const d = d_tab;
		memset(h, 0, 128);
		*(RangeUnit*)(h + 64) = u;
		RangeArgs a = RangeArgs();
		a.frame = ctx->tmp1.as<uint8_t>();
		a.size = 16 + have_bytes;
		a.sb_off = nullptr;
		a.direct_off = 12;
		a.units = (const RangeUnit*)(d + 64);
		a.unit_status = (uint32_t*)(d + 8);
		a.status = (uint32_t*)d;
		a.total_bytes = fi.total;
		a.sb_bytes = (uint32_t)fi.sb;
		a.T = (uint32_t)T;
		a.nunits = 1;
		volatile uint32_t* back = &ctx->h_total->decode_status;
		if (hipMemcpyAsync(d, h, 128, hipMemcpyHostToDevice, stream) != hipSuccess || stenos_r_launch_decode(a, stream) != hipSuccess ||
		    !copy((void*)back, d, 4, hipMemcpyDeviceToHost))
			return STENOS_ERROR_UNDEFINED;
		return *back ? (size_t)STENOS_ERROR_INVALID_INPUT : 0;
	}
};

// The host tail of the gather calls, after a status word with DECODE_STATUS_HOST_CODES: the pairs and the flags of the
// superblocks come down into h_gtab (d_ids == NULL: every pair is of frame 0, and two copies instead of three; one wait), every
// row is cut again with the kernels' own cutting function, the pieces of flagged superblocks are kept, ordered by (frame,
// superblock) and finished, one HostCodes per frame that has any.  h_frames, h_first: the call's frame table and numbering (m
// frames, S superblocks); frame f's pointer, size and FrameInfo at [f]; its offsets start at d_index + h_first[f] + f.
// Returns 0 or an error code.  Slow.
inline size_t finish_flagged_pieces(stenos_context_s* ctx, const codec::GatherFrame* h_frames, const uint64_t* h_first, size_t m, uint64_t S, const void* const* d_frames,
				    const size_t* sizes, const FrameInfo* info, size_t T, const uint64_t* d_index, const uint64_t* d_ids, const uint64_t* d_rows,
				    const uint32_t* d_flags, size_t n, uint64_t P, size_t row_bytes, void* d_dst, size_t dst_stride, hipStream_t stream)
{
	if (!zstd().ok)
		return STENOS_ERROR_ZSTD_INTERNAL;
	const size_t o_hrows = d_ids ? align64(n * 8) : 0, o_hflags = o_hrows + align64(n * 8);
	if (!ctx->h_gtab.ensure(o_hflags + S * 4) || !ctx->rtab.ensure(128) || !ctx->h_rtab.ensure(128))
		return STENOS_ERROR_ALLOC;
	uint64_t* const h_ids = (uint64_t*)ctx->h_gtab.data();
	uint64_t* const h_rows = (uint64_t*)(ctx->h_gtab.data() + o_hrows);
	uint32_t* const h_flags = (uint32_t*)(ctx->h_gtab.data() + o_hflags);
	if ((d_ids && hipMemcpyAsync(h_ids, d_ids, n * 8, hipMemcpyDeviceToHost, stream) != hipSuccess) ||
	    hipMemcpyAsync(h_rows, d_rows, n * 8, hipMemcpyDeviceToHost, stream) != hipSuccess ||
	    hipMemcpyAsync(h_flags, d_flags, S * 4, hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) {
		(void)hipStreamSynchronize(stream);
		return STENOS_ERROR_UNDEFINED;
	}
	struct FrameUnit {
		uint64_t frame;
		RangeUnit u;
	};
	std::vector<FrameUnit> units;
	for (uint64_t i = 0; i < n; ++i)
		for (uint64_t j = 0; j < P; ++j) {
			uint64_t g;
			codec::GatherPiece p;
			FrameUnit x;
			x.frame = d_ids ? h_ids[i] : 0;
			if (codec::gather_cut_pair(h_frames, m, row_bytes, dst_stride, x.frame, h_rows[i], i, j, &g, &p) != codec::GATHER_PAIR_PIECE || !h_flags[g])
				continue;
			x.u.dst = (uint8_t*)d_dst + p.dst;
			x.u.sb = (uint32_t)(g - h_first[x.frame]);
			x.u.lo = p.lo;
			x.u.hi = p.hi;
			x.u.unused = 0;
			units.push_back(x);
		}
	std::stable_sort(units.begin(), units.end(), [](const FrameUnit& x, const FrameUnit& y) { return x.frame != y.frame ? x.frame < y.frame : x.u.sb < y.u.sb; });
	for (size_t k = 0; k < units.size();) {
		const uint64_t f = units[k].frame;
		HostCodes hc(ctx, d_frames[f], sizes[f], T, d_index + h_first[f] + f, info[f], stream);
		for (; k < units.size() && units[k].frame == f; ++k)
			if (size_t err = hc.finish(units[k].u))
				return err;
	}
	return 0;
}

} // namespace stenos_host
