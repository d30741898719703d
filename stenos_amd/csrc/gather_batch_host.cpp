// gather_batch_host.cpp -- rows of many frames in device memory by (frame number, row number) pairs that live on the device
// (stenos_hip_gather_rows_batch, stenos_hip_frames_index; gather_batch.h).
#include <algorithm>

#include "gather_batch.h"
#include "range_host_codes.h"

namespace stenos_host {

namespace {

// The tables of both calls lie in one device buffer of their own (gbtab) with a page-locked mirror (h_gbtab), so an index that
// lives in the context's index buffer survives any number of gather calls:
//   [frame pointers: m][frame sizes: m] up | [heads: 12 m] down |
//   [GatherFrame: m][first: m + 1] up, and for the walks [DecodeArgs: m][header sizes: m][walk choice: m] up | the PiecePlan (frame_access.h)
struct BatchTables {
	size_t m = 0, o_ptrs = 0, o_sizes = 0, o_heads = 0, o_frames = 0, o_first = 0, o_dargs = 0, o_header = 0, o_walk = 0, o_plan = 0;
	explicit BatchTables(size_t frames) : m(frames)
	{
		o_sizes = o_ptrs + align64(m * 8);
		o_heads = o_sizes + align64(m * 8);
		o_frames = o_heads + align64(m * 12);
		o_first = o_frames + align64(m * sizeof(codec::GatherFrame));
		o_dargs = o_first + align64((m + 1) * 8);
		o_header = o_dargs + align64(m * sizeof(DecodeArgs));
		o_walk = o_header + align64(m * 8);
		o_plan = o_walk + align64(m);
	}
};

// The first bytes of all frames come to the host in one round trip (decompress_batch's head fetch) and are checked as the single
// call checks them; the frame table follows from them.  Returns 0, or the error code of the first frame stenos_hip_decompress
// refuses, or STENOS_ERROR_INVALID_PARAMETER for more superblocks than one workgroup each allows.
size_t fetch_frames(stenos_context_s* ctx, const BatchTables& t, size_t T, const void* const* d_frames, const size_t* sizes, size_t row_bytes, hipStream_t stream,
		    std::vector<FrameInfo>& info, uint64_t& S)
{
	const size_t m = t.m;
	uint8_t* const h = ctx->h_gbtab.data();
	uint8_t* const d = ctx->gbtab.as<uint8_t>();
	for (size_t f = 0; f < m; ++f) {
		((const void**)(h + t.o_ptrs))[f] = d_frames[f];
		((uint64_t*)(h + t.o_sizes))[f] = sizes[f];
	}
	if (hipMemcpyAsync(d, h, t.o_heads, hipMemcpyHostToDevice, stream) != hipSuccess ||
	    stenos_b_launch_heads((const uint8_t* const*)(d + t.o_ptrs), (const uint64_t*)(d + t.o_sizes), (uint32_t)m, d + t.o_heads, stream) != hipSuccess ||
	    hipMemcpyAsync(h + t.o_heads, d + t.o_heads, m * 12, hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) {
		(void)hipStreamSynchronize(stream); // (nothing may still read the page-locked mirror)
		return STENOS_ERROR_UNDEFINED;
	}
	info.assign(m, FrameInfo());
	S = 0;
	for (size_t f = 0; f < m; ++f) {
		const size_t have = sizes[f] < 12 ? sizes[f] : 12;
		if (const size_t e = parse_frame(h + t.o_heads + 12 * f, have, T, ~(size_t)0, info[f]))
			return e;
		if (info[f].total == 0)
			info[f].nsb = 0;
		S += info[f].nsb;
		if (S > 0x7FFFFFFFull)
			return STENOS_ERROR_INVALID_PARAMETER;
	}
	codec::GatherFrame* const frames = (codec::GatherFrame*)(h + t.o_frames);
	uint64_t* const first = (uint64_t*)(h + t.o_first);
	uint64_t s0 = 0;
	for (size_t f = 0; f < m; ++f) {
		frames[f] = codec::gather_frame((const uint8_t*)d_frames[f], sizes[f], info[f].total, info[f].sb, info[f].nsb, s0, row_bytes);
		first[f] = s0;
		s0 += info[f].nsb;
	}
	first[m] = s0;
	return 0;
}

// Every chain is walked on `stream` into the context's index, in the layout of gather_batch.h, by the rule of decompress_batch:
// chains up to kBatchSerialWalkMax superblocks in one launch of the serial batched walk, longer ones by the parallel walk, one
// launch each.  A chain that leaves its frame sets DECODE_STATUS_TRUNCATED in *d_status.  The tables behind o_frames go up here.
// Returns 0, STENOS_ERROR_ALLOC or STENOS_ERROR_UNDEFINED; nothing is waited for.
size_t walk_frames(stenos_context_s* ctx, const BatchTables& t, const void* const* d_frames, const size_t* sizes, const std::vector<FrameInfo>& info, uint64_t S,
		   uint32_t* d_status, hipStream_t stream, const uint64_t** index)
{
	const size_t m = t.m;
	uint8_t* const h = ctx->h_gbtab.data();
	uint8_t* const d = ctx->gbtab.as<uint8_t>();
	if (!ctx->sboff.ensure((S + m + 1) * 8) || !ctx->walk.ensure(stenos_k_walk_scratch_bytes()))
		return STENOS_ERROR_ALLOC;
	ctx->last_nsb = 0; // (the index workspace holds the batch's superblock offsets from here on)
	ctx->last_batch = true;
	uint64_t* const into = ctx->sboff.as<uint64_t>();
	*index = into;
	DecodeArgs* const h_args = (DecodeArgs*)(h + t.o_dargs);
	uint64_t* const h_header = (uint64_t*)(h + t.o_header);
	uint8_t* const h_walk = h + t.o_walk;
	const uint64_t* const first = (const uint64_t*)(h + t.o_first);
	std::vector<uint32_t> parallel_walks;
	for (size_t f = 0; f < m; ++f) {
		DecodeArgs a = DecodeArgs();
		a.frame = (const uint8_t*)d_frames[f];
		a.size = sizes[f];
		a.sb_off = into + first[f] + f;
		a.nsb = info[f].nsb;
		a.sb_bytes = (uint32_t)info[f].sb;
		a.status = d_status;
		h_args[f] = a;
		h_header[f] = info[f].header;
		// (the frame of an empty array has one entry, its end: the serial walk writes it)
		h_walk[f] = info[f].nsb <= kBatchSerialWalkMax || ctx->test_serial_walk;
		if (!h_walk[f])
			parallel_walks.push_back((uint32_t)f);
	}
	if (hipMemcpyAsync(d + t.o_frames, h + t.o_frames, t.o_plan - t.o_frames, hipMemcpyHostToDevice, stream) != hipSuccess ||
	    (parallel_walks.size() < m &&
	     stenos_b_launch_walk((const DecodeArgs*)(d + t.o_dargs), (const uint64_t*)(d + t.o_header), d + t.o_walk, (uint32_t)m, stream) != hipSuccess))
		return STENOS_ERROR_UNDEFINED;
	for (uint32_t f : parallel_walks) {
		const uint64_t* none = nullptr;
		if (const size_t e = frame_offsets(ctx, d_frames[f], sizes[f], info[f], &none, into + first[f] + f, d_status, stream))
			return e;
	}
	return 0;
}

bool batch_shape_refused(stenos_context_s* ctx, size_t m, size_t T)
{
	return m == 0 || m > 0x7FFFFFFFull || T == 0 || T > STENOS_K_LDS_MAX_T || (ctx->job_kind && ctx->job_async);
}

} // namespace

const uint64_t* frames_index(stenos_context_s* ctx, size_t m, size_t T, const void* const* d_frames, const size_t* sizes, size_t* entries, hipStream_t stream)
{
	if (entries)
		*entries = 0;
	if (!ctx || !d_frames || !sizes || !ctx->device_ready() || batch_shape_refused(ctx, m, T))
		return nullptr;
	const BatchTables t(m);
	if (!ctx->gbtab.ensure(t.o_plan + 64) || !ctx->h_gbtab.ensure(t.o_plan + 64))
		return nullptr;
	std::vector<FrameInfo> info;
	uint64_t S = 0;
	if (fetch_frames(ctx, t, T, d_frames, sizes, 1, stream, info, S))
		return nullptr;
	ctx->job_kind = 0;
	uint32_t* const d_status = (uint32_t*)(ctx->gbtab.as<uint8_t>() + t.o_plan);
	volatile uint32_t* back = &ctx->h_total->decode_status; // (page-locked)
	const uint64_t* index = nullptr;
	if (hipMemsetAsync(d_status, 0, 4, stream) != hipSuccess || walk_frames(ctx, t, d_frames, sizes, info, S, d_status, stream, &index) ||
	    hipMemcpyAsync((void*)back, d_status, 4, hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) {
		(void)hipStreamSynchronize(stream);
		return nullptr;
	}
	if (*back) // a header or payload runs past the end of its frame
		return nullptr;
	if (entries)
		*entries = (size_t)(S + m);
	return index;
}

// All of the call is enqueued on `stream`: the head fetch of all frames (one round trip), the tables and one memset, the walks
// when no index is given, gather_batch_count, gather_scan, gather_batch_fill, gather_batch_decode, the status word back -- so
// launches and host round trips grow neither with n nor with the superblocks, and with m only by the parallel walks of long
// chains.  Pieces in superblocks that went through zstd (codes 2-5) are rebuilt here from the pairs, with the kernels' own
// cutting function, and finished frame by frame as gather_rows finishes them (range_host_codes.h), which is slow.
size_t gather_rows_batch(stenos_context_s* ctx, size_t m, size_t T, const void* const* d_frames, const size_t* sizes, size_t row_bytes, size_t n,
			 const uint64_t* d_frame_ids, const uint64_t* d_rows, void* d_dst, size_t dst_stride, const uint64_t* d_index, hipStream_t stream)
{
	if (batch_shape_refused(ctx, m, T) || !PiecePlan::shape_ok(row_bytes, n, dst_stride))
		return STENOS_ERROR_INVALID_PARAMETER;
	const BatchTables t(m);
	if (!ctx->gbtab.ensure(t.o_plan + 64) || !ctx->h_gbtab.ensure(t.o_plan + 64))
		return STENOS_ERROR_ALLOC;
	std::vector<FrameInfo> info;
	uint64_t S = 0;
	if (const size_t e = fetch_frames(ctx, t, T, d_frames, sizes, row_bytes, stream, info, S))
		return e;
	uint8_t* const h = ctx->h_gbtab.data();
	const codec::GatherFrame* const h_frames = (const codec::GatherFrame*)(h + t.o_frames);
	const uint64_t* const h_first = (const uint64_t*)(h + t.o_first);
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
	else if (const size_t e = walk_frames(ctx, t, d_frames, sizes, info, S, d_status, stream, &d_index))
		return fail(e);
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
	if (status & DECODE_STATUS_HOST_CODES) {
		if (!zstd().ok)
			return STENOS_ERROR_ZSTD_INTERNAL;
		// the pairs and the flags come down; the pieces of the flagged superblocks are cut again here and grouped by frame
		const size_t o_hrows = align64(n * 8), o_hflags = o_hrows + align64(n * 8);
		if (!ctx->h_gtab.ensure(o_hflags + S * 4) || !ctx->rtab.ensure(128) || !ctx->h_rtab.ensure(128))
			return STENOS_ERROR_ALLOC;
		const uint64_t* const h_ids = (const uint64_t*)ctx->h_gtab.data();
		const uint64_t* const h_rows = (const uint64_t*)(ctx->h_gtab.data() + o_hrows);
		const uint32_t* const h_flags = (const uint32_t*)(ctx->h_gtab.data() + o_hflags);
		if (hipMemcpyAsync((void*)h_ids, d_frame_ids, n * 8, hipMemcpyDeviceToHost, stream) != hipSuccess ||
		    hipMemcpyAsync((void*)h_rows, d_rows, n * 8, hipMemcpyDeviceToHost, stream) != hipSuccess ||
		    hipMemcpyAsync((void*)h_flags, a.sb_flags, S * 4, hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess)
			return fail();
		struct FrameUnit {
			uint64_t frame;
			RangeUnit u;
		};
		std::vector<FrameUnit> units;
		for (uint64_t i = 0; i < n; ++i)
			for (uint64_t j = 0; j < P; ++j) {
				uint64_t g;
				codec::GatherPiece p;
				if (codec::gather_cut_pair(h_frames, m, row_bytes, dst_stride, h_ids[i], h_rows[i], i, j, &g, &p) != codec::GATHER_PAIR_PIECE || !h_flags[g])
					continue;
				FrameUnit x;
				x.frame = h_ids[i];
				x.u.dst = (uint8_t*)d_dst + p.dst;
				x.u.sb = (uint32_t)(g - h_first[x.frame]);
				x.u.lo = p.lo;
				x.u.hi = p.hi;
				x.u.unused = 0;
				units.push_back(x);
			}
		std::stable_sort(units.begin(), units.end(), [](const FrameUnit& x, const FrameUnit& y) { return x.frame != y.frame ? x.frame < y.frame : x.u.sb < y.u.sb; });
		for (size_t k = 0; k < units.size();) { // one HostCodes per frame that has flagged superblocks
			const uint64_t f = units[k].frame;
			HostCodes hc(ctx, d_frames[f], sizes[f], T, d_index + h_first[f] + f, info[f], stream);
			for (; k < units.size() && units[k].frame == f; ++k)
				if (size_t err = hc.finish(units[k].u))
					return err;
		}
	}
	return n * row_bytes;
}

} // namespace stenos_host
