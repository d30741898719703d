// frame_batch.h -- internal to the host side: the front end the calls that read many frames in device memory share
// (decompress_batch in batch_host.cpp; gather_rows_batch and frames_index in gather_batch_host.cpp), beside the front end of
// the calls that read one (frame_access.h).  Each rule once: how the first bytes of all frames reach the host, how the
// superblocks of a batch are numbered and where a frame's offsets lie in the index, which walk a chain takes.
//
// The tables are the caller's: it says where in its buffer and in the page-locked mirror of it they lie, and it uploads them.
// The steps of a call, in the order in which they reach the stream:
//   fetch_heads   pointers and sizes up, frame_heads_batch, the heads down, one wait; parse_frame's result per frame
//   number        (host) first[], S
//   plan_walks    (host) the index is made large enough; per frame the walk fields of its DecodeArgs, its header size, its walk
//   ...           the caller's one upload of its tables
//   launch_walks  walk_frames_batch if a frame takes it, then one parallel walk per long chain
// Errors are the caller's to judge: decompress_batch turns a frame's into that item's result and carries on, the gather calls
// fail on the first.
#pragma once
#include "batch.h"
#include "frame_access.h"

namespace stenos_host {

struct FrameBatch { // { ctx, m, d_frames, sizes, stream }: the call's frames, frame f at d_frames[f][0, sizes[f])
	stenos_context_s* ctx;
	size_t m;
	const void* const* d_frames;
	const size_t* sizes;
	hipStream_t stream;
	std::vector<FrameInfo> info;          // fetch_heads: parse_frame's, per frame ...
	std::vector<size_t> error;            // ... and its result (0: the frame takes part)
	std::vector<uint64_t> first;          // number: m + 1 entries, the batch's number of frame f's superblock 0; first[m] = S
	uint64_t S = 0;                       // superblocks of all frames that take part
	uint64_t* index = nullptr;            // plan_walks: the context's index; frame f's nsb_f + 1 offsets start at entry first[f] + f
	std::vector<uint32_t> parallel_walks; // plan_walks: the frames whose chain takes the parallel walk of walk.h
	bool serial_walks = false;            // plan_walks: some frame takes the serial batched walk

	// superblocks of frame f in the batch: none for a frame that was refused or holds an empty array
	uint64_t nsb(size_t f) const { return !error[f] && info[f].total ? info[f].nsb : 0; }

	// The first bytes of all frames come to the host in one round trip and are checked as the single call checks them, against
	// dst_sizes[f] (NULL: no bound).  h, d: the caller's mirror and buffer, [pointers: m][sizes: m] from o_ptrs on (o_sizes
	// behind them), [heads: 12 m] at o_heads.  Returns 0, or STENOS_ERROR_UNDEFINED with nothing left on the stream.
	size_t fetch_heads(size_t T, uint8_t* h, uint8_t* d, size_t o_ptrs, size_t o_sizes, size_t o_heads, const size_t* dst_sizes)
	{
		for (size_t f = 0; f < m; ++f) {
			((const void**)(h + o_ptrs))[f] = d_frames[f];
			((uint64_t*)(h + o_sizes))[f] = sizes[f];
		}
		if (hipMemcpyAsync(d + o_ptrs, h + o_ptrs, o_heads - o_ptrs, hipMemcpyHostToDevice, stream) != hipSuccess ||
		    stenos_b_launch_heads((const uint8_t* const*)(d + o_ptrs), (const uint64_t*)(d + o_sizes), (uint32_t)m, d + o_heads, stream) != hipSuccess ||
		    hipMemcpyAsync(h + o_heads, d + o_heads, m * 12, hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) {
			(void)hipStreamSynchronize(stream); // (nothing may still read the page-locked mirror)
			return STENOS_ERROR_UNDEFINED;
		}
		info.assign(m, FrameInfo());
		error.assign(m, 0);
		for (size_t f = 0; f < m; ++f)
			error[f] = parse_frame(h + o_heads + 12 * f, sizes[f] < 12 ? sizes[f] : 12, T, dst_sizes ? dst_sizes[f] : ~(size_t)0, info[f]);
		return 0;
	}

	// The superblocks of the batch are numbered through, frame by frame.
	void number()
	{
		first.assign(m + 1, 0);
		for (size_t f = 0; f < m; ++f)
			first[f + 1] = first[f] + nsb(f);
		S = first[m];
	}

	// The context's index gets room for S + m offsets and holds a batch's from here on.  Per frame: the walk fields of
	// h_args[f] (frame, size, sb_off, nsb, sb_bytes, status; the rest zero), its header size and whether the serial batched walk
	// takes it: chains up to kBatchSerialWalkMax superblocks do, longer ones take the parallel walk.  A refused frame takes
	// neither; the frame of an empty array has one entry, its end, which the serial walk writes if walk_empty says so.
	// d_status: the word a chain that leaves its frame sets DECODE_STATUS_TRUNCATED in, frame f's at d_status + f * status_step.
	// into: a buffer of the caller's with room for S + m offsets, which takes the walks instead (the context's index is left as
	// it is).  Returns 0 or STENOS_ERROR_ALLOC; nothing reaches the stream.
	size_t plan_walks(DecodeArgs* h_args, uint64_t* h_header, uint8_t* h_walk, uint32_t* d_status, size_t status_step, bool walk_empty, uint64_t* into = nullptr)
	{
		if (!into) {
			ctx->last_nsb = 0; // (the index workspace holds the batch's superblock offsets from here on)
			ctx->last_batch = true;
			ctx->last_frames = 0;
			if (!ctx->sboff.ensure((S + m + 1) * 8))
				return STENOS_ERROR_ALLOC;
		}
		if (!ctx->walk.ensure(stenos_k_walk_scratch_bytes()))
			return STENOS_ERROR_ALLOC;
		index = into ? into : ctx->sboff.as<uint64_t>();
		for (size_t f = 0; f < m; ++f) {
			DecodeArgs a = DecodeArgs();
			a.frame = (const uint8_t*)d_frames[f];
			a.size = sizes[f];
			a.sb_off = index + first[f] + f;
			a.nsb = nsb(f);
			a.sb_bytes = (uint32_t)info[f].sb;
			a.status = d_status + f * status_step;
			h_args[f] = a;
			h_header[f] = info[f].header;
			const bool walked = !error[f] && (info[f].total || walk_empty);
			// (only the test build can set test_serial_walk, stenos_hip_test_walk: one lane walks every chain)
			h_walk[f] = walked && (a.nsb <= kBatchSerialWalkMax || ctx->test_serial_walk);
			serial_walks |= h_walk[f] != 0;
			if (walked && !h_walk[f])
				parallel_walks.push_back((uint32_t)f);
		}
		return 0;
	}

	// The walks, over the tables plan_walks filled and the caller has uploaded.  Returns 0, STENOS_ERROR_ALLOC or
	// STENOS_ERROR_UNDEFINED; nothing is waited for.
	size_t launch_walks(const DecodeArgs* h_args, const DecodeArgs* d_args, const uint64_t* d_header, const uint8_t* d_walk)
	{
		if (serial_walks && stenos_b_launch_walk(d_args, d_header, d_walk, (uint32_t)m, stream) != hipSuccess)
			return STENOS_ERROR_UNDEFINED;
		for (uint32_t f : parallel_walks) { // (one launch per long chain, into the frame's part of the index)
			const uint64_t* none = nullptr;
			if (const size_t e = frame_offsets(ctx, d_frames[f], sizes[f], info[f], &none, (uint64_t*)h_args[f].sb_off, h_args[f].status, stream))
				return e;
		}
		return 0;
	}
};

// ---- the calls that take (frame number, row number) pairs (gather_batch_host.cpp, update_batch_host.cpp) ----
// Their frame tables lie at the start of one device buffer of the call's (d) with a page-locked mirror (h):
//   [frame pointers: m][frame sizes: m] up | [heads: 12 m] down |
//   [GatherFrame: m][first: m + 1] up, and for the walks [DecodeArgs: m][header sizes: m][walk choice: m] up | o_plan: the call's own
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

// The heads of all frames, their numbering, and the frame table that follows from them, in the mirror.  Returns 0, or the error
// code of the first frame stenos_hip_decompress refuses, or STENOS_ERROR_INVALID_PARAMETER for more superblocks than one
// workgroup each allows.
inline size_t fetch_frames(FrameBatch& b, const BatchTables& t, size_t T, size_t row_bytes, uint8_t* h, uint8_t* d)
{
	if (const size_t e = b.fetch_heads(T, h, d, t.o_ptrs, t.o_sizes, t.o_heads, nullptr))
		return e;
	b.number();
	codec::GatherFrame* const frames = (codec::GatherFrame*)(h + t.o_frames);
	for (size_t f = 0; f < b.m; ++f) {
		if (b.error[f])
			return b.error[f];
		if (b.first[f + 1] > 0x7FFFFFFFull)
			return STENOS_ERROR_INVALID_PARAMETER;
		frames[f] = codec::gather_frame((const uint8_t*)b.d_frames[f], b.sizes[f], b.info[f].total, b.info[f].sb, b.info[f].nsb, b.first[f], row_bytes);
	}
	memcpy(h + t.o_first, b.first.data(), (b.m + 1) * 8);
	return 0;
}

// Every chain is walked on the stream into the context's index (into: a buffer of the caller's instead, plan_walks), in the layout
// of gather_batch.h (the frame of an empty array has one entry, which the serial walk writes).  A chain that leaves its frame sets
// DECODE_STATUS_TRUNCATED in *d_status.  The tables from o_frames up to `up_end` (at least o_plan) go up here.  Returns 0,
// STENOS_ERROR_ALLOC or STENOS_ERROR_UNDEFINED; nothing is waited for.
inline size_t walk_frames(FrameBatch& b, const BatchTables& t, uint32_t* d_status, uint8_t* h, uint8_t* d, uint64_t* into = nullptr, size_t up_end = 0)
{
	DecodeArgs* const h_args = (DecodeArgs*)(h + t.o_dargs);
	if (const size_t e = b.plan_walks(h_args, (uint64_t*)(h + t.o_header), h + t.o_walk, d_status, 0, true, into))
		return e;
	if (hipMemcpyAsync(d + t.o_frames, h + t.o_frames, (up_end > t.o_plan ? up_end : t.o_plan) - t.o_frames, hipMemcpyHostToDevice, b.stream) != hipSuccess)
		return STENOS_ERROR_UNDEFINED;
	return b.launch_walks(h_args, (const DecodeArgs*)(d + t.o_dargs), (const uint64_t*)(d + t.o_header), d + t.o_walk);
}

inline bool batch_shape_refused(stenos_context_s* ctx, size_t m, size_t T)
{
	return m == 0 || m > 0x7FFFFFFFull || T == 0 || T > STENOS_K_LDS_MAX_T || (ctx->job_kind && ctx->job_async);
}

} // namespace stenos_host
