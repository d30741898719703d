// batch_host.cpp -- many independent items in one pass of kernels (batch.h).
#include "frame_batch.h"

namespace stenos_host {

// The item tables go up in one copy from the page-locked mirror h_btab, the per-item results come back in one; the number
// of launches and host round trips does not grow with the number of items (the tiny last superblocks add one round trip,
// items that take the parallel walk or carry zstd-coded superblocks add work of their own).
// decompress_batch gets from the frames' pointers and sizes to a walked index through the front end of the calls that read many
// frames (FrameBatch, frame_batch.h: the head fetch, the numbering, the choice of walk); the item tables, the per-item status
// words and what becomes of a refused item are its own.

static size_t batch_refused(stenos_context_s* ctx, size_t T)
{
	if (T == 0 || T > STENOS_K_LDS_MAX_T || (ctx->job_kind && ctx->job_async))
		return STENOS_ERROR_INVALID_PARAMETER;
	return 0;
}

size_t compress_batch(stenos_context_s* ctx, size_t n, size_t T, const void* const* d_srcs, const size_t* bytes, void* const* d_dsts, const size_t* dst_sizes,
		      size_t* results, hipStream_t stream)
{
	const int level = ctx->level;
	if (size_t e = batch_refused(ctx, T))
		return e;
	if (level >= 2 || level < 0 || (level == 1 && T == 1) || ctx->max_nanoseconds) // the strategy layer and the time limit
		return STENOS_ERROR_INVALID_PARAMETER;
	if (n >= 0x7FFFFFFFull)
		return STENOS_ERROR_INVALID_PARAMETER;
	ctx->job_kind = 0;
	const uint32_t stride = stenos_k_slot_stride((uint32_t)T);
	std::vector<size_t> res(n, 0);
	std::vector<uint8_t> run(n, 0);
	std::vector<FramePlan> plan(n);
	std::vector<uint32_t> tiny;
	uint64_t B = 0, S = 0;
	uint32_t bps = 0;
	for (size_t i = 0; i < n; ++i) {
		FramePlan& f = plan[i];
		size_t e = plan_frame(ctx, T, bytes[i], level, f);
		if (!is_err(e) && dst_sizes[i] < f.header) // stenos.cpp:862-863, 870-871
			e = STENOS_ERROR_DST_OVERFLOW;
		const uint64_t last_bytes = bytes[i] ? bytes[i] - (f.nsb - 1) * f.sb : 0;
		const bool is_tiny = bytes[i] && level >= 1 && last_bytes < 128;
		if (!is_err(e) && is_tiny && !zstd().ok)
			e = STENOS_ERROR_ZSTD_INTERNAL;
		if (is_err(e)) {
			res[i] = e;
			continue;
		}
		run[i] = 1;
		bps = f.bps; // (the same for every item: no shift at levels 0 and 1)
		if (bytes[i]) {
			B += f.nfull + (f.tail ? 1 : 0);
			S += f.nsb;
			if (is_tiny)
				tiny.push_back((uint32_t)i);
		}
	}
	if (S * codec::PACK_WAVES >= 0x7FFFFFFFull || B >= 0x7FFFFFFFull) // one workgroup per unit of work
		return STENOS_ERROR_INVALID_PARAMETER;
	const size_t ntiny = tiny.size();
	ctx->last_nsb = 0; // (the workspace below holds the batch's superblock offsets from here on)
	ctx->last_batch = true;
	ctx->last_frames = 0;
	// table layout (device and its host mirror): jobs, block and superblock prefix sums, per-item words, tiny list, tiny records
	const size_t o_jobs = 0, o_bpre = align64(n * sizeof(codec::FrameJob)), o_spre = o_bpre + align64((n + 1) * 8), o_state = o_spre + align64((n + 1) * 8),
		     o_tiny = o_state + align64(n * sizeof(BatchItemState)), o_tin = o_tiny + align64(ntiny * 4 + 4), o_tout = o_tin + align64(ntiny * sizeof(BatchTinyIn)),
		     tab_bytes = o_tout + align64(ntiny * sizeof(BatchTinyOut));
	if (!ctx->btab.ensure(tab_bytes) || !ctx->h_btab.ensure(tab_bytes) || !ctx->slots.ensure((level >= 1 ? B : 0) * stride + 64) || !ensure_workspace(ctx, B, S, n))
		return STENOS_ERROR_ALLOC;
	uint8_t* const h = ctx->h_btab.data();
	uint8_t* const d = ctx->btab.as<uint8_t>();
	codec::FrameJob* h_jobs = (codec::FrameJob*)(h + o_jobs);
	uint64_t* h_bpre = (uint64_t*)(h + o_bpre);
	uint64_t* h_spre = (uint64_t*)(h + o_spre);
	BatchItemState* h_state = (BatchItemState*)(h + o_state);
	const codec::FrameJob* d_jobs = (const codec::FrameJob*)(d + o_jobs);
	BatchItemState* d_state = (BatchItemState*)(d + o_state);
	BatchTinyOut* d_tout = (BatchTinyOut*)(d + o_tout);
	uint64_t b0 = 0, s0 = 0;
	size_t k_tiny = 0;
	for (size_t i = 0; i < n; ++i) {
		const FramePlan& f = plan[i];
		const bool go = run[i] && bytes[i];
		const uint64_t nb = go ? f.nfull + (f.tail ? 1 : 0) : 0, ns = go ? f.nsb : 0;
		h_bpre[i] = b0;
		h_spre[i] = s0;
		h_state[i] = { 0, 0, 0xFFFFFFFFu };
		codec::FrameJob j;
		if (!frame_job(ctx, f, T, go ? bytes[i] : 0, b0, s0, i, j))
			return STENOS_ERROR_ALLOC;
		if (!go)
			j.nfull = j.nsb = j.tail_bytes = 0;
		j.src = (const uint8_t*)d_srcs[i];
		j.dst = (uint8_t*)d_dsts[i];
		j.dst_size = dst_sizes[i];
		j.slots = ctx->slots.as<uint8_t>() + (level >= 1 ? b0 * stride : 0);
		j.total = &d_state[i].total;
		j.status = &d_state[i].status;
		j.first_flagged = &d_state[i].first_flagged;
		const bool is_tiny = k_tiny < ntiny && tiny[k_tiny] == i;
		j.override_payload = is_tiny ? d_tout[k_tiny].payload : nullptr;
		k_tiny += is_tiny ? 1 : 0;
		j.shift_byte = run[i] ? f.shift : 0xFFFFFFFFu; // (a refused item: no header, no superblocks -- the kernels leave it alone)
		j.header_bytes = (uint32_t)f.header;
		j.force_copy = level == 0 ? 1u : 0u;
		j.tiny_last = is_tiny ? 1u : 0u;
		j.check_total = 1;
		h_jobs[i] = j;
		b0 += nb;
		s0 += ns;
	}
	h_bpre[n] = b0;
	h_spre[n] = s0;
	memcpy(h + o_tiny, tiny.data(), ntiny * 4);
	const uint64_t* d_bpre = (const uint64_t*)(d + o_bpre);
	const uint64_t* d_spre = (const uint64_t*)(d + o_spre);
	const uint32_t* d_tiny = (const uint32_t*)(d + o_tiny);
	const uint32_t un = (uint32_t)n;
	auto fail = [&]() -> size_t {
		(void)hipStreamSynchronize(stream); // (nothing may still read the page-locked mirror)
		return STENOS_ERROR_UNDEFINED;
	};
	if (hipMemcpyAsync(d, h, o_tin, hipMemcpyHostToDevice, stream) != hipSuccess)
		return fail();
	if ((level >= 1 && stenos_b_launch_encode(d_jobs, d_bpre, un, B, (uint32_t)T, stream) != hipSuccess) || stenos_b_launch_plan(d_jobs, d_spre, un, S, stream) != hipSuccess ||
	    stenos_b_launch_scan(d_jobs, un, stream) != hipSuccess || (S && stenos_b_launch_resolve(d_jobs, un, (uint32_t)T, stream) != hipSuccess))
		return fail();
	if (ntiny) {
		// The reference hands zstd the rest of the caller's buffer as capacity (stenos.cpp:666, 895), so the last superblock's
		// final offset must be known first: one round trip for all of them (enqueue_compress does the same per frame)
		BatchTinyIn* h_tin = (BatchTinyIn*)(h + o_tin);
		BatchTinyOut* h_tout = (BatchTinyOut*)(h + o_tout);
		if (stenos_b_launch_tiny_gather(d_jobs, d_tiny, (uint32_t)ntiny, (BatchTinyIn*)(d + o_tin), stream) != hipSuccess ||
		    hipMemcpyAsync(h_tin, d + o_tin, ntiny * sizeof(BatchTinyIn), hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess)
			return fail();
		for (size_t k = 0; k < ntiny; ++k) {
			const size_t i = tiny[k];
			const FramePlan& f = plan[i];
			const BatchTinyIn& in = h_tin[k];
			BatchTinyOut& out = h_tout[k];
			memset(&out, 0, sizeof(out));
			const size_t last_bytes = superblock_bytes(bytes[i], f.sb, f.nsb - 1);
			if (in.status || dst_sizes[i] < in.off_last + 4) // an earlier superblock did not fit / no room for this header (stenos.cpp:427-429)
				continue;
			const size_t room = dst_sizes[i] - (size_t)in.off_last - 4;
			uint8_t comp[kTinyCapacity];
			out.code = tiny_superblock(in.raw, last_bytes, room, comp, tiny_capacity(room), &out.csize);
			if (!out.code)
				continue;
			memcpy(out.payload, comp, out.csize);
			out.end = in.off_last + 4 + out.csize;
		}
		if (hipMemcpyAsync(d + o_tout, h_tout, ntiny * sizeof(BatchTinyOut), hipMemcpyHostToDevice, stream) != hipSuccess ||
		    stenos_b_launch_tiny_apply(d_jobs, d_tiny, (uint32_t)ntiny, (const BatchTinyOut*)(d + o_tout), stream) != hipSuccess)
			return fail();
	}
	if (stenos_b_launch_pack(d_jobs, d_spre, un, S, bps, stream) != hipSuccess ||
	    hipMemcpyAsync(h_state, d_state, n * sizeof(BatchItemState), hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess)
		return fail();
	for (size_t i = 0; i < n; ++i)
		results[i] = !run[i] ? res[i] : (h_state[i].status || h_state[i].total > dst_sizes[i]) ? (size_t)STENOS_ERROR_DST_OVERFLOW : (size_t)h_state[i].total;
	ctx->warm = true;
	return 0;
}

size_t decompress_batch(stenos_context_s* ctx, size_t n, size_t T, const void* const* d_srcs, const size_t* src_sizes, void* const* d_dsts, const size_t* dst_sizes,
			size_t* results, hipStream_t stream)
{
	if (size_t e = batch_refused(ctx, T))
		return e;
	if (n >= 0x7FFFFFFFull)
		return STENOS_ERROR_INVALID_PARAMETER;
	ctx->job_kind = 0;
	// 1. the first bytes of every frame, for the header checks of the single call (FrameBatch::fetch_heads)
	const size_t o_frames = 0, o_sizes = align64(n * 8), o_heads = o_sizes + align64(n * 8), head_bytes = o_heads + align64(n * 12);
	// 2. the items' decode arguments, superblock prefix sums, walk start and choice, status words
	const size_t o_args = head_bytes, o_spre = o_args + align64(n * sizeof(DecodeArgs)), o_first = o_spre + align64((n + 1) * 8), o_walk = o_first + align64(n * 8),
		     o_status = o_walk + align64(n), tab_bytes = o_status + align64(n * 4);
	if (!ctx->btab.ensure(tab_bytes) || !ctx->h_btab.ensure(tab_bytes))
		return STENOS_ERROR_ALLOC;
	uint8_t* const h = ctx->h_btab.data();
	uint8_t* const d = ctx->btab.as<uint8_t>();
	auto fail = [&]() -> size_t {
		(void)hipStreamSynchronize(stream);
		return STENOS_ERROR_UNDEFINED;
	};
	FrameBatch b{ ctx, n, d_srcs, src_sizes, stream };
	if (const size_t e = b.fetch_heads(T, h, d, o_frames, o_sizes, o_heads, dst_sizes))
		return e;
	const std::vector<FrameInfo>& info = b.info;
	std::vector<size_t> res = b.error; // (a refused item keeps its error code; the others go on)
	b.number();
	const uint64_t S = b.S;
	if (S >= 0x7FFFFFFFull)
		return STENOS_ERROR_INVALID_PARAMETER;
	DecodeArgs* h_args = (DecodeArgs*)(h + o_args);
	uint32_t* h_status = (uint32_t*)(h + o_status);
	const DecodeArgs* d_args = (const DecodeArgs*)(d + o_args);
	// (an empty array has nothing to decode and no chain to walk)
	if (const size_t e = b.plan_walks(h_args, (uint64_t*)(h + o_first), h + o_walk, (uint32_t*)(d + o_status), 1, false))
		return e;
	for (size_t i = 0; i < n; ++i) {
		const bool go = !is_err(res[i]) && info[i].total;
		if (!decode_args(ctx, d_srcs[i], src_sizes[i], h_args[i].sb_off, d_dsts[i], go ? info[i].total : 0, b.nsb(i), info[i].sb, T, h_args[i].status, h_args[i]))
			return STENOS_ERROR_ALLOC;
		h_status[i] = 0;
	}
	memcpy(h + o_spre, b.first.data(), (n + 1) * 8);
	if (hipMemcpyAsync(d + o_args, h + o_args, tab_bytes - o_args, hipMemcpyHostToDevice, stream) != hipSuccess ||
	    b.launch_walks(h_args, d_args, (const uint64_t*)(d + o_first), d + o_walk))
		return fail();
	if (stenos_b_launch_decode(d_args, (const uint64_t*)(d + o_spre), (uint32_t)n, S, (uint32_t)T, stream) != hipSuccess ||
	    hipMemcpyAsync(h_status, d + o_status, n * 4, hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess)
		return fail();
	ctx->warm = true;
	std::vector<uint64_t> idx;
	for (size_t i = 0; i < n; ++i) {
		if (is_err(res[i]) || !info[i].total)
			continue;
		const uint32_t status = h_status[i];
		if (const size_t e = status_error(status))
			res[i] = e;
		else if (status & DECODE_STATUS_HOST_CODES) { // zstd-based superblocks: finished on the host, item by item
			idx.resize(info[i].nsb + 1);
			if (hipMemcpy(idx.data(), h_args[i].sb_off, (info[i].nsb + 1) * 8, hipMemcpyDeviceToHost) != hipSuccess)
				return STENOS_ERROR_UNDEFINED;
			const size_t e = finish_host_codes(ctx, (const uint8_t*)d_srcs[i], nullptr, src_sizes[i], T, idx.data(), info[i], (uint8_t*)d_dsts[i], stream);
			res[i] = is_err(e) ? e : (size_t)info[i].total;
		}
		else
			res[i] = (size_t)info[i].total;
	}
	for (size_t i = 0; i < n; ++i)
		results[i] = res[i];
	return 0;
}

} // namespace stenos_host
