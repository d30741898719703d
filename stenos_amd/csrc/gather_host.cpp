// gather_host.cpp -- rows of one frame in device memory by row numbers that live on the device (stenos_hip_gather_rows, gather.h).
#include <algorithm>

#include "host.h"
#include "gather.h"
#include "range_host_codes.h"

namespace stenos_host {

// The host knows the shape of the call and nothing about the rows: how many pieces a row has at most (P), the table sizes and
// the grid of every launch follow from n, P and the number of superblocks.  All of it is enqueued on `stream` -- the header
// fetch, the walk when no index is given, one memset (status word, counts, flags), gather_count, gather_scan, gather_fill,
// gather_decode, the status word back -- so launches and host round trips grow neither with n nor with the frame.  The tables
// have a buffer of their own (gtab): an index the caller passes may be the context's own (sboff) and stays as it is.
// Pieces in superblocks that went through zstd (codes 2-5) are rebuilt here from the row numbers, with the kernels' own
// cutting function, and finished one by one as the ranges call finishes its units (range_host_codes.h), which is slow.
size_t gather_rows(stenos_context_s* ctx, const void* d_src, size_t T, size_t size, size_t row_bytes, size_t n, const uint64_t* d_rows, void* d_dst,
		   size_t dst_stride, const uint64_t* d_index, hipStream_t stream)
{
	if (T == 0 || T > STENOS_K_LDS_MAX_T || row_bytes == 0 || dst_stride < row_bytes || (ctx->job_kind && ctx->job_async))
		return STENOS_ERROR_INVALID_PARAMETER;
	if (n > ~(size_t)0 / row_bytes || n - 1 > (~(size_t)0 - row_bytes) / dst_stride) // n * row_bytes, (n - 1) * dst_stride + row_bytes
		return STENOS_ERROR_INVALID_PARAMETER;
	uint8_t head[12] = { 0 };
	const size_t have = size < 12 ? size : 12;
	if (have && (hipMemcpyAsync(head, d_src, have, hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess))
		return STENOS_ERROR_UNDEFINED;
	FrameInfo fi;
	const size_t e = parse_frame(head, have, T, ~(size_t)0, fi);
	if (is_err(e))
		return e;
	if (fi.total == 0) // an array without rows: every row number is invalid
		return STENOS_ERROR_INVALID_PARAMETER;
	const uint64_t P = codec::gather_pieces_per_row(row_bytes, fi.sb);
	if (P > 0x7FFFFFFFull || (uint64_t)n > 0x7FFFFFFFull / P) // one thread per piece, 32-bit places in the piece table
		return STENOS_ERROR_INVALID_PARAMETER;
	const uint64_t npieces = (uint64_t)n * P, waves = stenos_g_decode_waves(fi.nsb, npieces);
	if (waves > 0x7FFFFFFFull) // one workgroup per wavefront: beyond the grid limit (parse_frame)
		return STENOS_ERROR_INVALID_PARAMETER;
	ctx->job_kind = 0;
	// gtab: [status, 64 bytes][count: nsb words][flags: nsb words] cleared by one memset, [ppre: nsb + 1][wpre: nsb + 1][pieces]
	const size_t o_count = 64, o_flags = o_count + align64(fi.nsb * 4), o_ppre = o_flags + align64(fi.nsb * 4), o_wpre = o_ppre + align64((fi.nsb + 1) * 4),
		     o_pieces = o_wpre + align64((fi.nsb + 1) * 4), tab_bytes = o_pieces + npieces * sizeof(codec::GatherPiece);
	if (!ctx->gtab.ensure(tab_bytes))
		return STENOS_ERROR_ALLOC;
	uint8_t* const d = ctx->gtab.as<uint8_t>();
	uint32_t* const d_status = (uint32_t*)d;
	auto fail = [&]() -> size_t {
		(void)hipStreamSynchronize(stream);
		return STENOS_ERROR_UNDEFINED;
	};
	if (hipMemsetAsync(d, 0, o_ppre, stream) != hipSuccess)
		return fail();
	if (!d_index) { // the chain is walked first, into the context's index
		if (!ctx->sboff.ensure((fi.nsb + 2) * 8) || !ctx->walk.ensure(stenos_k_walk_scratch_bytes()))
			return (void)hipStreamSynchronize(stream), STENOS_ERROR_ALLOC;
		d_index = ctx->sboff.as<uint64_t>();
		if (stenos_k_launch_walk((const uint8_t*)d_src, size, fi.header, fi.nsb, (uint32_t)fi.sb, ctx->sboff.as<uint64_t>(), d_status,
					 ctx->test_serial_walk ? nullptr : ctx->walk.p, stream) != hipSuccess)
			return fail();
	}
	GatherArgs a = GatherArgs();
	a.frame = (const uint8_t*)d_src;
	a.size = size;
	a.sb_off = d_index;
	a.rows = d_rows;
	a.dst = (uint8_t*)d_dst;
	a.n = n;
	a.valid_rows = codec::gather_valid_rows(fi.total, row_bytes);
	a.npieces = npieces;
	a.shape.row_bytes = row_bytes;
	a.shape.dst_stride = dst_stride;
	a.shape.total = fi.total;
	a.shape.sb = fi.sb;
	a.P = (uint32_t)P;
	a.nsb = (uint32_t)fi.nsb;
	a.T = (uint32_t)T;
	a.waves = (uint32_t)waves;
	a.status = d_status;
	a.count = (uint32_t*)(d + o_count);
	a.sb_flags = (uint32_t*)(d + o_flags);
	a.ppre = (uint32_t*)(d + o_ppre);
	a.wpre = (uint32_t*)(d + o_wpre);
	a.pieces = (codec::GatherPiece*)(d + o_pieces);
	volatile uint32_t* back = &ctx->h_total->decode_status; // (page-locked)
	if (stenos_g_launch_count(a, stream) != hipSuccess || stenos_g_launch_scan(a, stream) != hipSuccess || stenos_g_launch_fill(a, stream) != hipSuccess ||
	    stenos_g_launch_decode(a, stream) != hipSuccess || hipMemcpyAsync((void*)back, d_status, 4, hipMemcpyDeviceToHost, stream) != hipSuccess ||
	    hipStreamSynchronize(stream) != hipSuccess)
		return fail();
	ctx->warm = true;
	const uint32_t status = *back;
	if (status & DECODE_STATUS_BAD_ROW)
		return STENOS_ERROR_INVALID_PARAMETER;
	if (status & DECODE_STATUS_TRUNCATED)
		return STENOS_ERROR_SRC_OVERFLOW;
	if (status & DECODE_STATUS_INVALID)
		return STENOS_ERROR_INVALID_INPUT;
	if (status & DECODE_STATUS_HOST_CODES) {
		if (!zstd().ok)
			return STENOS_ERROR_ZSTD_INTERNAL;
		// the row numbers and the flags come down; the pieces of the flagged superblocks are cut again here
		const size_t o_hflags = align64(n * 8);
		if (!ctx->h_gtab.ensure(o_hflags + fi.nsb * 4) || !ctx->rtab.ensure(128) || !ctx->h_rtab.ensure(128))
			return STENOS_ERROR_ALLOC;
		const uint64_t* const h_rows = (const uint64_t*)ctx->h_gtab.data();
		const uint32_t* const h_flags = (const uint32_t*)(ctx->h_gtab.data() + o_hflags);
		if (hipMemcpyAsync((void*)h_rows, d_rows, n * 8, hipMemcpyDeviceToHost, stream) != hipSuccess ||
		    hipMemcpyAsync((void*)h_flags, a.sb_flags, fi.nsb * 4, hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess)
			return fail();
		std::vector<RangeUnit> units;
		for (uint64_t i = 0; i < n; ++i)
			for (uint64_t j = 0; j < P; ++j) {
				uint64_t s;
				codec::GatherPiece p;
				if (h_rows[i] >= a.valid_rows || !codec::gather_cut(a.shape, h_rows[i], i, j, &s, &p) || !h_flags[s])
					continue;
				RangeUnit u;
				u.dst = (uint8_t*)d_dst + p.dst;
				u.sb = (uint32_t)s;
				u.lo = p.lo;
				u.hi = p.hi;
				u.unused = 0;
				units.push_back(u);
			}
		std::stable_sort(units.begin(), units.end(), [](const RangeUnit& x, const RangeUnit& y) { return x.sb < y.sb; });
		HostCodes hc;
		hc.ctx = ctx;
		hc.d_frame = (const uint8_t*)d_src;
		hc.size = size;
		hc.T = T;
		hc.d_index = d_index;
		hc.fi = fi;
		hc.stream = stream;
		hc.h_tab = ctx->h_rtab.data();
		hc.d_tab = ctx->rtab.as<uint8_t>();
		hc.o_one = 0;
		for (const RangeUnit& u : units)
			if (size_t err = hc.finish(u))
				return err;
	}
	return n * row_bytes;
}

} // namespace stenos_host
