// gather_host.cpp -- rows of one frame in device memory by row numbers that live on the device (stenos_hip_gather_rows, gather.h).
#include <algorithm>

#include "range_host_codes.h"

namespace stenos_host {

// All of the call is enqueued on `stream` -- the header fetch, one memset (status word, counts, flags), the walk when no index is
// given, gather_count, gather_scan, gather_fill (the PiecePlan of frame_access.h, in a buffer of the call's own, gtab),
// gather_decode, the status word back -- so launches and host round trips grow neither with n nor with the frame.
// Pieces in superblocks that went through zstd (codes 2-5) are rebuilt here from the row numbers, with the kernels' own
// cutting function, and finished one by one as the ranges call finishes its units (range_host_codes.h), which is slow.
size_t gather_rows(stenos_context_s* ctx, const void* d_src, size_t T, size_t size, size_t row_bytes, size_t n, const uint64_t* d_rows, void* d_dst,
		   size_t dst_stride, const uint64_t* d_index, hipStream_t stream)
{
	if (T == 0 || T > STENOS_K_LDS_MAX_T || !PiecePlan::shape_ok(row_bytes, n, dst_stride) || (ctx->job_kind && ctx->job_async))
		return STENOS_ERROR_INVALID_PARAMETER;
	FrameInfo fi;
	if (const size_t e = fetch_frame_info(d_src, T, size, ~(size_t)0, stream, fi))
		return e;
	if (fi.total == 0) // an array without rows: every row number is invalid
		return STENOS_ERROR_INVALID_PARAMETER;
	PiecePlan plan;
	if (!plan.init(fi, row_bytes, n))
		return STENOS_ERROR_INVALID_PARAMETER;
	const uint64_t P = plan.P, waves = stenos_g_decode_waves(fi.nsb, plan.npieces);
	if (waves > 0x7FFFFFFFull) // one workgroup per wavefront: beyond the grid limit (parse_frame)
		return STENOS_ERROR_INVALID_PARAMETER;
	ctx->job_kind = 0;
	if (!ctx->gtab.ensure(plan.end))
		return STENOS_ERROR_ALLOC;
	uint8_t* const d = ctx->gtab.as<uint8_t>();
	uint32_t* const d_status = (uint32_t*)d;
	auto fail = [&](size_t code = STENOS_ERROR_UNDEFINED) -> size_t {
		(void)hipStreamSynchronize(stream);
		return code;
	};
	if (hipMemsetAsync(d, 0, plan.o_ppre, stream) != hipSuccess)
		return fail();
	if (const size_t e = frame_offsets(ctx, d_src, size, fi, &d_index, nullptr, d_status, stream))
		return fail(e);
	GatherArgs a = plan.args(d, d_src, size, d_index, fi, T, row_bytes, n, d_rows, dst_stride, d_status);
	a.dst = (uint8_t*)d_dst;
	a.waves = (uint32_t)waves;
	volatile uint32_t* back = &ctx->h_total->decode_status; // (page-locked)
	if (!PiecePlan::enqueue(a, stream) || stenos_g_launch_decode(a, stream) != hipSuccess || hipMemcpyAsync((void*)back, d_status, 4, hipMemcpyDeviceToHost, stream) != hipSuccess ||
	    hipStreamSynchronize(stream) != hipSuccess)
		return fail();
	ctx->warm = true;
	const uint32_t status = *back;
	if (const size_t e = status_error(status))
		return e;
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
		HostCodes hc(ctx, d_src, size, T, d_index, fi, stream);
		for (const RangeUnit& u : units)
			if (size_t err = hc.finish(u))
				return err;
	}
	return n * row_bytes;
}

} // namespace stenos_host
