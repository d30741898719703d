// gather_batch_host.cpp -- rows of many frames in device memory by (frame number, row number) pairs that live on the device
// (stenos_hip_gather_rows_batch, stenos_hip_frames_index; gather_batch.h).  Both calls get from the frames' pointers and sizes to
// a walked index through the front end of the calls that read many frames (FrameBatch, frame_batch.h); the frame tables
// (BatchTables, fetch_frames, walk_frames), the limits and failing on the first refused frame are those of the calls that take
// pairs, which stenos_hip_update_rows_batch shares; the one status word is theirs.
// The tables of both calls lie in one device buffer of their own (gbtab) with a page-locked mirror (h_gbtab), so an index that
// lives in the context's index buffer survives any number of gather calls.
#include "frame_batch.h"
#include "gather_batch.h"
#include "range_host_codes.h"

namespace stenos_host {

const uint64_t* frames_index(stenos_context_s* ctx, size_t m, size_t T, const void* const* d_frames, const size_t* sizes, size_t* entries, hipStream_t stream)
{
	if (entries)
		*entries = 0;
	if (!ctx || !d_frames || !sizes || !ctx->device_ready() || batch_shape_refused(ctx, m, T))
		return nullptr;
	const BatchTables t(m);
	if (!ctx->gbtab.ensure(t.o_plan + 64) || !ctx->h_gbtab.ensure(t.o_plan + 64))
		return nullptr;
	FrameBatch b{ ctx, m, d_frames, sizes, stream };
	if (fetch_frames(b, t, T, 1, ctx->h_gbtab.data(), ctx->gbtab.as<uint8_t>()))
		return nullptr;
	ctx->job_kind = 0;
	uint32_t* const d_status = (uint32_t*)(ctx->gbtab.as<uint8_t>() + t.o_plan);
	volatile uint32_t* back = &ctx->h_total->decode_status; // (page-locked)
	if (hipMemsetAsync(d_status, 0, 4, stream) != hipSuccess || walk_frames(b, t, d_status, ctx->h_gbtab.data(), ctx->gbtab.as<uint8_t>()) ||
	    hipMemcpyAsync((void*)back, d_status, 4, hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) {
		(void)hipStreamSynchronize(stream);
		return nullptr;
	}
	if (*back) // a header or payload runs past the end of its frame
		return nullptr;
	ctx->last_frames = (size_t)(b.S + m);
	if (entries)
		*entries = (size_t)(b.S + m);
	return b.index;
}

// All of the call is enqueued on `stream`: the head fetch of all frames (one round trip), the tables and one memset, the walks
// when no index is given, gather_batch_count, gather_scan, gather_batch_fill, gather_batch_decode, the status word back -- so
// launches and host round trips grow neither with n nor with the superblocks, and with m only by the parallel walks of long
// chains.  Pieces in superblocks that went through zstd (codes 2-5) are rebuilt on the host from the pairs and finished frame by
// frame, by the tail gather_rows ends with (range_host_codes.h, finish_flagged_pieces), which is slow.
size_t gather_rows_batch(stenos_context_s* ctx, size_t m, size_t T, const void* const* d_frames, const size_t* sizes, size_t row_bytes, size_t n,
			 const uint64_t* d_frame_ids, const uint64_t* d_rows, void* d_dst, size_t dst_stride, const uint64_t* d_index, hipStream_t stream)
{
	if (batch_shape_refused(ctx, m, T) || !PiecePlan::shape_ok(row_bytes, n, dst_stride))
		return STENOS_ERROR_INVALID_PARAMETER;
	const BatchTables t(m);
	if (!ctx->gbtab.ensure(t.o_plan + 64) || !ctx->h_gbtab.ensure(t.o_plan + 64))
		return STENOS_ERROR_ALLOC;
	FrameBatch b{ ctx, m, d_frames, sizes, stream };
	if (const size_t e = fetch_frames(b, t, T, row_bytes, ctx->h_gbtab.data(), ctx->gbtab.as<uint8_t>()))
		return e;
	const uint64_t S = b.S;
	uint8_t* const h = ctx->h_gbtab.data();
	const codec::GatherFrame* const h_frames = (const codec::GatherFrame*)(h + t.o_frames);
	uint64_t P = 1; // the call's pieces per pair: the largest of the frames' (a frame with fewer leaves the rest empty)
	for (size_t f = 0; f < m; ++f)
		P = std::max<uint64_t>(P, h_frames[f].pieces);
	PiecePlan plan;
	if (!plan.init(S, P, n))
		return STENOS_ERROR_INVALID_PARAMETER;
	const uint64_t waves = stenos_g_decode_waves(S, plan.npieces);
	if (waves > 0x7FFFFFFFull) // one workgroup per wavefront: beyond the grid limit (parse_frame)
		return STENOS_ERROR_INVALID_PARAMETER;
	ctx->job_kind = 0;
	// (growing the buffer would lose nothing: the mirror holds the tables, and they go up again below)
	if (!ctx->gbtab.ensure(t.o_plan + plan.end))
		return STENOS_ERROR_ALLOC;
	uint8_t* const d = ctx->gbtab.as<uint8_t>();
	uint8_t* const dp = d + t.o_plan;
	uint32_t* const d_status = (uint32_t*)dp;
	auto fail = [&](size_t code = STENOS_ERROR_UNDEFINED) -> size_t {
		(void)hipStreamSynchronize(stream);
		return code;
	};
	if (hipMemsetAsync(dp, 0, plan.o_ppre, stream) != hipSuccess)
		return fail();
	if (d_index) {
		if (hipMemcpyAsync(d + t.o_frames, h + t.o_frames, t.o_dargs - t.o_frames, hipMemcpyHostToDevice, stream) != hipSuccess)
			return fail();
	}
	else if (const size_t e = walk_frames(b, t, d_status, h, d))
		return fail(e);
	else
		d_index = b.index;
	GatherBatchArgs a = GatherBatchArgs();
	a.frames = (const codec::GatherFrame*)(d + t.o_frames);
	a.first = (const uint64_t*)(d + t.o_first);
	a.sb_off = d_index;
	a.frame_ids = d_frame_ids;
	a.rows = d_rows;
	a.dst = (uint8_t*)d_dst;
	a.row_bytes = row_bytes;
	a.dst_stride = dst_stride;
	a.npieces = plan.npieces;
	a.m = (uint32_t)m;
	a.P = (uint32_t)P;
	a.S = (uint32_t)S;
	a.T = (uint32_t)T;
	a.waves = (uint32_t)waves;
	a.status = d_status;
	a.count = (uint32_t*)(dp + plan.o_count);
	a.sb_flags = (uint32_t*)(dp + plan.o_flags);
	a.ppre = (uint32_t*)(dp + plan.o_ppre);
	a.wpre = (uint32_t*)(dp + plan.o_wpre);
	a.pieces = (codec::GatherPiece*)(dp + plan.o_pieces);
	GatherArgs scan = GatherArgs(); // gather_scan reads the tables and their length, nothing else
	scan.nsb = a.S;
	scan.count = a.count;
	scan.ppre = a.ppre;
	scan.wpre = a.wpre;
	volatile uint32_t* back = &ctx->h_total->decode_status; // (page-locked)
	if (stenos_gb_launch_count(a, stream) != hipSuccess || stenos_g_launch_scan(scan, stream) != hipSuccess || stenos_gb_launch_fill(a, stream) != hipSuccess ||
	    stenos_gb_launch_decode(a, stream) != hipSuccess || hipMemcpyAsync((void*)back, d_status, 4, hipMemcpyDeviceToHost, stream) != hipSuccess ||
	    hipStreamSynchronize(stream) != hipSuccess)
		return fail();
	ctx->warm = true;
	const uint32_t status = *back;
	if (const size_t e = status_error(status))
		return e;
	if (status & DECODE_STATUS_HOST_CODES)
		if (const size_t e = finish_flagged_pieces(ctx, h_frames, b.first.data(), m, S, d_frames, sizes, b.info.data(), T, d_index, d_frame_ids, d_rows, a.sb_flags, n, P,
							   row_bytes, d_dst, dst_stride, stream))
			return e;
	return n * row_bytes;
}

} // namespace stenos_host
