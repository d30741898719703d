// frame_access.h -- internal to the host side: the front end the calls that read one frame in device memory share
// (decode_host.cpp, range_host.cpp, gather_host.cpp, update_host.cpp).  Each rule once: the header fetch, the index a call works
// with, the error code of a status word, the piece tables of the calls that take row numbers.  The calls that read many frames
// (batch_host.cpp, gather_batch_host.cpp) have theirs beside it, on top of this one: frame_batch.h.
#pragma once
#include "host.h"
#include "gather.h"

namespace stenos_host {

inline size_t align64(size_t v) { return (v + 63) & ~(size_t)63; }

// Superblocks up to which a chain of a call over many frames (frame_batch.h) is walked by one lane (walk_frames_batch) instead
// of the parallel walk of walk.h.
// Measured on MI355X (tools/batch_rate.py --walk, profiles/batch_rate.txt): a single call that walks 256 superblocks of int32
// serially decodes in 214 us, with the parallel walk in 240 us; at 1024 superblocks 428 against 239.  In a batch the serial
// walks of all items run side by side, while every parallel walk is a launch of its own.
constexpr uint64_t kBatchSerialWalkMax = 256;

// The first bytes of the frame come to the host (one round trip: the stream is waited for) and are checked: parse_frame's result.
inline size_t fetch_frame_info(const void* d_src, size_t T, size_t size, size_t dst_size, hipStream_t stream, FrameInfo& fi)
{
	uint8_t head[12] = { 0 };
	const size_t have = size < 12 ? size : 12;
	if (have && (hipMemcpyAsync(head, d_src, have, hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess))
		return STENOS_ERROR_UNDEFINED;
	return parse_frame(head, have, T, dst_size, fi);
}

// The index a call works with, in *index.  On entry the caller's d_index: where there is one it stays, as it is (it may be the
// context's own, sboff, from stenos_hip_last_index / stenos_hip_frame_index: nothing here touches that buffer then).  Where it
// is NULL the chain is walked on `stream` into `into` (room for nsb + 1 offsets; NULL: the context's index, made large enough
// here), which becomes *index; the walk sets DECODE_STATUS_TRUNCATED in *d_status where the chain leaves the frame.
// Returns 0, STENOS_ERROR_ALLOC or STENOS_ERROR_UNDEFINED; nothing is waited for.
inline size_t frame_offsets(stenos_context_s* ctx, const void* d_src, size_t size, const FrameInfo& fi, const uint64_t** index, uint64_t* into, uint32_t* d_status,
			    hipStream_t stream)
{
	if (*index)
		return 0;
	if ((!into && !ctx->sboff.ensure((fi.nsb + 2) * 8)) || !ctx->walk.ensure(stenos_k_walk_scratch_bytes()))
		return STENOS_ERROR_ALLOC;
	if (!into) {
		into = ctx->sboff.as<uint64_t>();
		ctx->last_frames = 0; // (the walk overwrites a many-frame index)
	}
	*index = into;
	// (only the test build can set test_serial_walk, stenos_hip_test_walk: one lane walks the chain)
	if (stenos_k_launch_walk((const uint8_t*)d_src, size, fi.header, fi.nsb, (uint32_t)fi.sb, into, d_status, ctx->test_serial_walk ? nullptr : ctx->walk.p, stream) !=
	    hipSuccess)
		return STENOS_ERROR_UNDEFINED;
	return 0;
}

// The error code of a call whose kernels left these DECODE_STATUS_* bits; 0: none (DECODE_STATUS_HOST_CODES is no error)
inline size_t status_error(uint32_t status)
{
	if (status & DECODE_STATUS_BAD_ROW)
		return STENOS_ERROR_INVALID_PARAMETER;
	if (status & DECODE_STATUS_DST_OVERFLOW)
		return STENOS_ERROR_DST_OVERFLOW;
	if (status & DECODE_STATUS_TRUNCATED)
		return STENOS_ERROR_SRC_OVERFLOW;
	if (status & DECODE_STATUS_INVALID)
		return STENOS_ERROR_INVALID_INPUT;
	return 0;
}

// The calls that take n row numbers on the device (gather, update) know the shape of the call and nothing about the rows: how
// many pieces a row has at most (P) and the sizes of the tables follow from n, P and the number of superblocks.  The tables lie
// in one device buffer of the call's:
//   [the call's words, 64 bytes][count: nsb words][flags: nsb words] | [ppre: nsb + 1][wpre: nsb + 1] | [pieces: npieces] | end
// zero on entry up to o_ppre (gather.h; a call that reads the prefixes without having filled them clears up to o_pieces), by one
// memset from the start of the buffer.  What else a call keeps in the buffer lies from `end` on.
struct PiecePlan {
	uint64_t P = 0, npieces = 0;
	size_t o_count = 0, o_flags = 0, o_ppre = 0, o_wpre = 0, o_pieces = 0, end = 0;

	// the shape of the call, checked before anything is fetched: n * row_bytes and (n - 1) * stride + row_bytes must be representable
	static bool shape_ok(size_t row_bytes, size_t n, size_t stride)
	{
		return row_bytes != 0 && stride >= row_bytes && (!n || (n <= ~(size_t)0 / row_bytes && n - 1 <= (~(size_t)0 - row_bytes) / stride));
	}
	// false: more pieces than one thread each and 32-bit places in the piece table allow (STENOS_ERROR_INVALID_PARAMETER)
	bool init(const FrameInfo& fi, size_t row_bytes, size_t n) { return init(fi.nsb, fi.total ? codec::gather_pieces_per_row(row_bytes, fi.sb) : 1, n); }
	// ... from the numbers themselves: nsb superblocks (of one frame, or of all frames of a batch), pieces_per_row pieces per row
	bool init(uint64_t nsb, uint64_t pieces_per_row, size_t n)
	{
		P = pieces_per_row;
		if (P == 0 || P > 0x7FFFFFFFull || (uint64_t)n > 0x7FFFFFFFull / P)
			return false;
		npieces = (uint64_t)n * P;
		o_count = 64;
		o_flags = o_count + align64(nsb * 4);
		o_ppre = o_flags + align64(nsb * 4);
		o_wpre = o_ppre + align64((nsb + 1) * 4);
		o_pieces = o_wpre + align64((nsb + 1) * 4);
		end = o_pieces + align64(npieces * sizeof(codec::GatherPiece));
		return true;
	}
	// the arguments of the piece kernels over the tables at d; stride: of the rows' other side (the destination's or the source's:
	// a piece's offset counts in it); dst and waves are gather_decode's alone
	GatherArgs args(uint8_t* d, const void* d_frame, size_t size, const uint64_t* index, const FrameInfo& fi, size_t T, size_t row_bytes, size_t n,
			const uint64_t* d_rows, size_t stride, uint32_t* d_status) const
	{
		GatherArgs a = GatherArgs();
		a.frame = (const uint8_t*)d_frame;
		a.size = size;
		a.sb_off = index;
		a.rows = d_rows;
		a.n = n;
		a.valid_rows = codec::gather_valid_rows(fi.total, row_bytes);
		a.npieces = npieces;
		a.shape.row_bytes = row_bytes;
		a.shape.dst_stride = stride;
		a.shape.total = fi.total;
		a.shape.sb = fi.sb;
		a.P = (uint32_t)P;
		a.nsb = (uint32_t)fi.nsb;
		a.T = (uint32_t)T;
		a.status = d_status;
		a.count = (uint32_t*)(d + o_count);
		a.sb_flags = (uint32_t*)(d + o_flags);
		a.ppre = (uint32_t*)(d + o_ppre);
		a.wpre = (uint32_t*)(d + o_wpre);
		a.pieces = (codec::GatherPiece*)(d + o_pieces);
		return a;
	}
	// gather_count, gather_scan, gather_fill: the pieces of all rows, ordered by superblock
	static bool enqueue(const GatherArgs& a, hipStream_t stream)
	{
		return stenos_g_launch_count(a, stream) == hipSuccess && stenos_g_launch_scan(a, stream) == hipSuccess && stenos_g_launch_fill(a, stream) == hipSuccess;
	}
};

} // namespace stenos_host
