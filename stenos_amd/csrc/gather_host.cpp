// gather_host.cpp -- rows of one frame in device memory by row numbers that live on the device (stenos_hip_gather_rows, gather.h).
#include "range_host_codes.h"

namespace stenos_host {

// All of the call is enqueued on `stream` -- the header fetch, one memset (status word, counts, flags), the walk when no index is
// given, gather_count, gather_scan, gather_fill (the PiecePlan of frame_access.h, in a buffer of the call's own, gtab),
// gather_decode, the status word back -- so launches and host round trips grow neither with n nor with the frame.
// Pieces in superblocks that went through zstd (codes 2-5) are rebuilt here from the row numbers, with the kernels' own
// cutting function, and finished one by one as the ranges call finishes its units (range_host_codes.h, finish_flagged_pieces),
// which is slow.
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
	if (status & DECODE_STATUS_HOST_CODES) { // (a batch of one frame, numbered from 0)
		const codec::GatherFrame frame = codec::gather_frame((const uint8_t*)d_src, size, fi.total, fi.sb, fi.nsb, 0, row_bytes);
		const uint64_t first = 0;
		if (const size_t e = finish_flagged_pieces(ctx, &frame, &first, 1, fi.nsb, &d_src, &size, &fi, T, d_index, nullptr, d_rows, a.sb_flags, n, P, row_bytes, d_dst,
							   dst_stride, stream))
			return e;
	}
	return n * row_bytes;
}

} // namespace stenos_host
