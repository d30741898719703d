// encode_host.cpp -- levels 0 and 1 on device memory: frame geometry, the workspace and the FrameJob of the encode
// pipeline, the kernel sequence of one frame, the device-pointer call and the end of a pending job.
#include "frame_access.h"

namespace stenos_host {

// ctx->prepare + frame geometry (stenos.cpp:115-185, 853-874).  Returns 0 or an error code.
size_t plan_frame(const stenos_context_s* ctx, size_t T, size_t bytes, int level, FramePlan& f)
{
	if (T == 0 || T >= STENOS_MAX_BYTESOFTYPE)
		return STENOS_ERROR_INVALID_BYTESOFTYPE;
	const size_t bs = T * 256;
	if (ctx->custom_shift != STENOS_NO_BLOCK_SHIFT) {
		f.sb = bs << ctx->custom_shift;
		f.shift = 255;
		f.header = 12;
	}
	else {
		f.sb = base_superblock(bs);
		f.shift = 0;
		if (bytes > f.sb) {
			f.shift = level ? (uint32_t)(level - 1) / 2 : 0;
			f.sb <<= f.shift;
		}
		f.header = 8;
	}
	if (f.sb < bs || f.sb >= STENOS_MAX_BLOCK_BYTES)
		return STENOS_ERROR_INVALID_PARAMETER;
	f.nsb = bytes / f.sb + (bytes % f.sb ? 1 : 0);
	f.nfull = bytes / bs;
	f.tail = (uint32_t)(bytes % bs);
	f.bps = (uint32_t)(f.sb / bs);
	return 0;
}

// What this build cannot do is refused loudly instead of being routed to a CPU path (nothing at present: every level and
// every bytesoftype the reference accepts has a device path).
size_t check_supported(const stenos_context_s* ctx, size_t T, int level)
{
	(void)ctx;
	(void)level;
	return T > kMaxT ? STENOS_ERROR_INVALID_BYTESOFTYPE : 0;
}
// bytesoftype above 64: scratch for the workgroups of kernels_wide.hip, at most 1 GiB (at least one workgroup's worth)
uint64_t wide_scratch_bytes(size_t T, uint64_t units)
{
	if (T <= STENOS_K_LDS_MAX_T)
		return 0;
	const uint64_t stride = stenos_kw_scratch_stride((uint32_t)T);
	uint64_t groups = ((uint64_t)1 << 30) / stride;
	groups = groups > units ? units : groups;
	groups = groups > 2048 ? 2048 : (groups < 1 ? 1 : groups);
	return groups * stride;
}
bool wide_scratch(stenos_context_s* ctx, size_t T, uint64_t units, uint8_t** p, uint64_t* bytes)
{
	*bytes = wide_scratch_bytes(T, units);
	*p = nullptr;
	if (*bytes && !ctx->wide.ensure((size_t)*bytes))
		return false;
	if (*bytes)
		*p = ctx->wide.as<uint8_t>();
	return true;
}

// The tables of the encode pipeline for `blocks` blocks and `sbs` superblocks in `frames` frames (a frame's superblock
// offsets have one entry more than it has superblocks), and the device words.
bool ensure_workspace(stenos_context_s* ctx, uint64_t blocks, uint64_t sbs, uint64_t frames)
{
	return ctx->bsize.ensure((blocks + 1) * 4) && ctx->binfo.ensure((blocks + 1) * 4) && ctx->bneed.ensure((blocks + 1) * 4) && ctx->boff.ensure((blocks + 1) * 4) &&
	       ctx->sbcsize.ensure((sbs + 1) * 4) && ctx->sbneed.ensure((sbs + 1) * 4) && ctx->sbcode.ensure(sbs + 4) && ctx->sboff.ensure((sbs + frames + 7) * 8) &&
	       ctx->misc.ensure(4096);
}
// The job of frame number `frame` whose tables start at block b0 / superblock s0 of that workspace: geometry, tables, the
// device words and the wide kernels' scratch; everything else is zero.  What is a caller's own comes after the call: source,
// destination and capacity, the slot base, shift_byte, header_bytes, force_copy, tiny_last, check_total, fixed_capacity, qprod.
bool frame_job(stenos_context_s* ctx, const FramePlan& f, size_t T, size_t bytes, uint64_t b0, uint64_t s0, uint64_t frame, codec::FrameJob& j)
{
	memset(&j, 0, sizeof(j));
	DeviceWords* w = ctx->words();
	j.slots = ctx->slots.as<uint8_t>();
	j.bsize = ctx->bsize.as<uint32_t>() + b0;
	j.binfo = ctx->binfo.as<uint32_t>() + b0;
	j.bneed = ctx->bneed.as<uint32_t>() + b0;
	j.boff = ctx->boff.as<uint32_t>() + b0;
	j.sb_csize = ctx->sbcsize.as<uint32_t>() + s0;
	j.sb_code = ctx->sbcode.as<uint8_t>() + s0;
	j.sb_need = ctx->sbneed.as<uint32_t>() + s0;
	j.sb_off = ctx->sboff.as<uint64_t>() + s0 + frame;
	j.total = &w->total;
	j.status = &w->encode_status;
	j.first_flagged = &w->first_flagged;
	j.override_payload = w->override_payload;
	j.nfull = f.nfull;
	j.nsb = f.nsb;
	j.total_bytes = bytes;
	j.tail_bytes = f.tail;
	j.bps = f.bps;
	j.sb_bytes = (uint32_t)f.sb;
	j.slot_stride = stenos_k_slot_stride((uint32_t)T);
	j.T = (uint32_t)T;
	return wide_scratch(ctx, T, f.nfull + (f.tail ? 1 : 0), &j.wide_scratch, &j.wide_scratch_bytes);
}

// A last superblock shorter than 128 bytes (stenos.cpp:435-437): zstd level 1 (zstd_wrapper.h:49-56) into `out`, else a
// copy (stenos.cpp:668-669, 366-367).  The reference hands zstd the rest of the caller's buffer as capacity (stenos.cpp:666,
// 895) and zstd's result depends on it: `capacity` is what zstd is given, `room` the bytes left behind the superblock's
// header; `out` holds capacity bytes and at least n.  Returns the superblock's code (2 or 6), or 0: it does not fit.
uint32_t tiny_superblock(const uint8_t* raw, size_t n, size_t room, uint8_t* out, size_t capacity, uint32_t* csize)
{
	const size_t r = zstd().compress(out, capacity, raw, n, 1);
	if (!zstd().is_error(r) && r <= n) {
		*csize = (uint32_t)r;
		return 2;
	}
	if (room < n)
		return 0;
	memcpy(out, raw, n);
	*csize = (uint32_t)n;
	return 6;
}

// Enqueue the compression of `bytes` device bytes into a frame (or, with frame_header == false, into
// the bare superblock stream used by the private API).  Nothing is waited for except, for a final
// superblock shorter than 128 bytes, the copy of those bytes to the host.
size_t enqueue_compress(stenos_context_s* ctx, const uint8_t* d_src, size_t T, size_t bytes, uint8_t* d_dst, size_t dst_size, int level,
			const FramePlan& f, bool frame_header, hipStream_t stream)
{
	const uint64_t nblocks = f.nfull + (f.tail ? 1 : 0);
	const uint32_t stride = stenos_k_slot_stride((uint32_t)T);
	if (!ensure_workspace(ctx, nblocks, f.nsb, 1))
		return STENOS_ERROR_ALLOC;

	const size_t last_bytes = superblock_bytes(bytes, f.sb, f.nsb - 1);
	const bool tiny_last = level >= 1 && last_bytes < 128; // small input: direct zstd (stenos.cpp:435-437)
	if (tiny_last && !zstd().ok)
		return STENOS_ERROR_ZSTD_INTERNAL;

	DeviceWords* w = ctx->words();
	codec::FrameJob j;
	if (!frame_job(ctx, f, T, bytes, 0, 0, 0, j))
		return STENOS_ERROR_ALLOC;
	j.src = d_src;
	j.dst = d_dst;
	j.dst_size = dst_size;
	j.shift_byte = frame_header ? f.shift : 0xFFFFFFFFu;
	j.header_bytes = frame_header ? (uint32_t)f.header : 0u;
	j.force_copy = level == 0 ? 1u : 0u;
	j.tiny_last = tiny_last ? 1u : 0u;
	const uint64_t header = j.header_bytes;

	// Superblocks whose capacity is certainly large enough for any encoding ("safe zone", normally all but the
	// last one or two) need no capacity replay and no overflow check; they are processed in chunks, the
	// pack of a chunk overlapping the encoding of the next one on a second stream.  The remaining tail zone
	// goes through plan / scan / resolve / pack in order.
	uint64_t s_tight = codec::safe_superblocks(dst_size, header, f.bps, (uint32_t)T, f.sb, f.nsb);
	if (tiny_last && s_tight > f.nsb - 1)
		s_tight = f.nsb - 1;
	auto first_block = [&](uint64_t sb_index) { // first block of a superblock (nblocks for sb_index == nsb)
		const uint64_t b = sb_index * f.bps;
		return sb_index >= f.nsb ? nblocks : (b < f.nfull ? b : f.nfull);
	};

	uint64_t* d_carry = &w->scan_carry;
	// Safe superblocks that consist of full blocks go through the fused kernel (encode + offsets + store in one launch).
	// (offset 0 means "not published yet" to the fused kernel, so frames without a header stay on the other path)
	uint64_t s_fused = 0;
	if (level >= 1 && header > 0 && stenos_k_fused_supported((uint32_t)T) && !ctx->no_fused)
		s_fused = f.nfull / f.bps < s_tight ? f.nfull / f.bps : s_tight;
	// One arena serves both: the staging streams of the fused superblocks, then (the fused kernel is done by
	// then) the 16-byte aligned slots of the remaining blocks, addressed by their absolute block number.
	const uint64_t b_unfused = first_block(s_fused);
	// Which fused kernel.  Bytesoftype 4 takes encode_superblocks_nt (non-temporal input and frame, fewer workgroups: the
	// staged streams stay in the caches) unless the context's last fused call stored more than half its superblocks
	// as copies: incompressible input reads its source twice (a measuring pass, then the copy or a second pass), and there the
	// policy costs instead (full entropy +30 %).  Like the guess of a workgroup inside the kernel, history decides.
	bool fused_nt = stenos_k_fused_nt_supported((uint32_t)T) && !ctx->fused_copy_heavy;
	if (ctx->test_fused_variant)
		fused_nt = ctx->test_fused_variant == 2 && stenos_k_fused_nt_supported((uint32_t)T);
	if (level >= 1) {
		// (the arena fits either kernel's staging buffers, so that a change of kernel between calls allocates nothing)
		const size_t stage_bytes = s_fused ? fused_stage_bytes_any((uint32_t)T, f.bps, s_fused) : 0;
		const size_t slot_bytes = (size_t)(nblocks - b_unfused + 1) * stride;
		if (!ctx->slots.ensure(stage_bytes > slot_bytes ? stage_bytes : slot_bytes))
			return STENOS_ERROR_ALLOC;
		j.slots = ctx->slots.as<uint8_t>() - b_unfused * (uint64_t)stride;
	}
	if (s_fused) {
		if (!ctx->chain.ensure((s_fused + 2) * 8))
			return STENOS_ERROR_ALLOC;
		uint64_t* desc = ctx->chain.as<uint64_t>() + 1; // word 0: ticket counter
		if (stenos_k_launch_init((uint8_t*)w, header, ctx->chain.as<uint64_t>(), s_fused + 2, j.sb_off, s_fused + 8, stream) != hipSuccess)
			return STENOS_ERROR_UNDEFINED;
		ctx->mark(0, stream);
		if (stenos_k_launch_encode_fused(j, s_fused, ctx->slots.as<uint8_t>(), desc, ctx->chain.as<uint32_t>(), d_carry, &w->fused_copies, fused_nt, stream) !=
		    hipSuccess)
			return STENOS_ERROR_UNDEFINED;
		ctx->mark(1, stream);
	}
	else if (stenos_k_launch_init((uint8_t*)w, header, nullptr, 0, nullptr, 0, stream) != hipSuccess)
		return STENOS_ERROR_UNDEFINED;
	if (s_tight > s_fused) {
		// safe superblocks the fused kernel does not take (bytesoftype too large for its LDS budget, frames without a header):
		// one encode / plan / scan / pack sequence.  (Overlapping the pack of one chunk with the encoding of the next on a
		// second stream was measured on MI355X and gains nothing.)
		if (s_fused == 0)
			ctx->mark(0, stream); // kernel timing: the encode_blocks launch of the safe zone
		if (level >= 1 && stenos_k_launch_encode(j, first_block(s_fused), first_block(s_tight), stream) != hipSuccess)
			return STENOS_ERROR_UNDEFINED;
		if (s_fused == 0)
			ctx->mark(1, stream);
		if (stenos_k_launch_plan(j, s_fused, s_tight, stream) != hipSuccess || stenos_k_launch_scan(j, s_fused, s_tight, d_carry, stream) != hipSuccess ||
		    stenos_k_launch_pack(j, s_fused, s_tight, stream) != hipSuccess)
			return STENOS_ERROR_UNDEFINED;
	}
	// tail zone
	j.check_total = 1;
	if (s_tight < f.nsb) {
		if (s_tight == 0)
			ctx->mark(0, stream);
		if (level >= 1 && stenos_k_launch_encode(j, first_block(s_tight), nblocks, stream) != hipSuccess)
			return STENOS_ERROR_UNDEFINED;
		if (s_tight == 0)
			ctx->mark(1, stream);
		if (stenos_k_launch_plan(j, s_tight, f.nsb, stream) != hipSuccess || stenos_k_launch_scan(j, s_tight, f.nsb, d_carry, stream) != hipSuccess ||
		    stenos_k_launch_resolve(j, stream) != hipSuccess)
			return STENOS_ERROR_UNDEFINED;
	}

	if (tiny_last) {
		// zstd is given the room the caller's buffer has left (tiny_superblock), so the final offset of this last
		// superblock must be known first.
		uint64_t off_last = 0;
		uint32_t status = 0, csize = 0;
		uint8_t raw[128], comp[kTinyCapacity];
		if (hipMemcpyAsync(&off_last, j.sb_off + (f.nsb - 1), 8, hipMemcpyDeviceToHost, stream) != hipSuccess ||
		    hipMemcpyAsync(&status, j.status, 4, hipMemcpyDeviceToHost, stream) != hipSuccess ||
		    hipMemcpyAsync(raw, d_src + (bytes - last_bytes), last_bytes, hipMemcpyDeviceToHost, stream) != hipSuccess ||
		    hipStreamSynchronize(stream) != hipSuccess)
			return STENOS_ERROR_UNDEFINED;
		if (status || dst_size < off_last + 4) // an earlier superblock did not fit / no room for this header (stenos.cpp:427-429)
			return STENOS_ERROR_DST_OVERFLOW;
		const size_t room = dst_size - (size_t)off_last - 4;
		const uint32_t code = tiny_superblock(raw, last_bytes, room, comp, tiny_capacity(room), &csize);
		if (!code)
			return STENOS_ERROR_DST_OVERFLOW;
		const uint64_t end = off_last + 4 + csize;
		const uint8_t code8 = (uint8_t)code;
		if (hipMemcpyAsync(w->override_payload, comp, csize, hipMemcpyHostToDevice, stream) != hipSuccess ||
		    hipMemcpyAsync(j.sb_code + (f.nsb - 1), &code8, 1, hipMemcpyHostToDevice, stream) != hipSuccess ||
		    hipMemcpyAsync(j.sb_csize + (f.nsb - 1), &csize, 4, hipMemcpyHostToDevice, stream) != hipSuccess ||
		    hipMemcpyAsync(j.sb_off + f.nsb, &end, 8, hipMemcpyHostToDevice, stream) != hipSuccess ||
		    hipMemcpyAsync(j.total, &end, 8, hipMemcpyHostToDevice, stream) != hipSuccess ||
		    hipStreamSynchronize(stream) != hipSuccess) // the sources live on this stack frame
			return STENOS_ERROR_UNDEFINED;
		j.override_code = code;
	}
	if (stenos_k_launch_pack(j, s_tight, f.nsb, stream) != hipSuccess)
		return STENOS_ERROR_UNDEFINED;
	// total, the encode status and the fused kernel's copy count travel together: the words in front of scan_carry
	if (hipMemcpyAsync(ctx->h_total, w, offsetof(DeviceWords, scan_carry), hipMemcpyDeviceToHost, stream) != hipSuccess)
		return STENOS_ERROR_UNDEFINED;
	ctx->job_fused_nsb = s_fused;
	ctx->last_nsb = f.nsb;
	ctx->last_batch = false;
	ctx->last_frames = 0;
	return 0;
}

size_t compress_device(stenos_context_s* ctx, const void* d_src, size_t T, size_t bytes, void* d_dst, size_t dst_size, hipStream_t stream, bool wait)
{
	if (!ctx->device_ready())
		return STENOS_ERROR_INVALID_INSTRUCTION_SET;
	const int level = ctx->level;
	if (ctx->max_nanoseconds) // the time limit is a feature of the host-pointer ABI (compress_timed); these entry points take none
		return STENOS_ERROR_INVALID_PARAMETER;
	FramePlan f;
	size_t e = plan_frame(ctx, T, bytes, level, f);
	if (is_err(e))
		return e;
	e = check_supported(ctx, T, level);
	if (is_err(e))
		return e;
	if (dst_size < f.header) // stenos.cpp:862-863, 870-871
		return STENOS_ERROR_DST_OVERFLOW;
	ctx->job_kind = 0;
	auto host_made = [&](size_t total) { // a frame the host finished: no device-side index, nothing to read back but its size
		ctx->last_nsb = 0;
		ctx->last_batch = false;
		ctx->last_frames = 0;
		ctx->h_total->total = total;
		ctx->h_total->encode_status = 0;
		ctx->set_job(1, stream, !wait, dst_size);
	};
	if (bytes && needs_strategy(T, level)) {
		// the strategy layer needs the input on the host (estimator, zstd): fetch it, assemble the frame there
		const size_t roomy = f.header + f.nsb * 4 + bytes + f.sb / 128 + 4096; // beyond the largest frame (all copies) + ZSTD_compressBound's margin the capacity no longer matters
		const size_t cap = dst_size < roomy ? dst_size : roomy;
		HostBuf& h_out = ctx->h_out;
		if (!h_out.ensure(cap + 64))
			return STENOS_ERROR_ALLOC;
		// (no host copy of the input: the strategy layer fetches what it looks at)
		size_t r = compress_strategy(ctx, nullptr, (const uint8_t*)d_src, T, bytes, h_out.data(), cap, level, f, stream, (uint8_t*)d_dst);
		if (is_err(r))
			return r;
		host_made(r);
		return wait ? finish_job(ctx) : 0;
	}
	if (bytes == 0) { // stenos.cpp:876-878
		uint8_t h[12];
		write_frame_header(h, f.shift, 0, f.sb);
		if (hipMemcpyAsync(d_dst, h, f.header, hipMemcpyHostToDevice, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess)
			return STENOS_ERROR_UNDEFINED;
		host_made(f.header);
		return f.header;
	}
	e = enqueue_compress(ctx, (const uint8_t*)d_src, T, bytes, (uint8_t*)d_dst, dst_size, level, f, true, stream);
	if (is_err(e))
		return e;
	ctx->set_job(1, stream, !wait, dst_size);
	ctx->job_src = d_src;
	ctx->job_dst = d_dst;
	ctx->job_T = T;
	ctx->job_bytes = bytes;
	return wait ? finish_job(ctx) : 0;
}

size_t finish_job(stenos_context_s* ctx)
{
	ctx->job_host_codes = false;
	if (!ctx->job_kind)
		return STENOS_ERROR_INVALID_PARAMETER;
	if (hipStreamSynchronize(ctx->job_stream) != hipSuccess)
		return STENOS_ERROR_UNDEFINED;
	ctx->warm = true;
	const int kind = ctx->job_kind;
	ctx->job_kind = 0;
	if (kind == 1) {
		if (ctx->job_fused_nsb) { // history for the next call's choice of fused kernel (enqueue_compress)
			const uint32_t copies = ctx->h_total->fused_copies;
			ctx->fused_copy_heavy = 2ull * copies > ctx->job_fused_nsb;
			ctx->job_fused_nsb = 0;
		}
		const uint64_t total = ctx->h_total->total;
		uint32_t estatus = ctx->h_total->encode_status;
		if (ctx->inject_chain_timeout > 0 && ctx->job_src && !ctx->no_fused) {
			--ctx->inject_chain_timeout;
			estatus |= codec::ENCODE_STATUS_CHAIN_TIMEOUT;
		}
		if (estatus & codec::ENCODE_STATUS_CHAIN_TIMEOUT) {
			// The fused kernel gave up waiting for a frame offset (its waits are bounded so that a scheduling accident cannot
			// hang the device; never seen in practice).  The frame is then produced once more by the kernels that need no
			// such wait (encode_blocks / plan / scan / pack); only when that fails too is the call an error.
			if (ctx->no_fused || !ctx->job_src)
				return STENOS_ERROR_UNDEFINED;
			ctx->no_fused = true;
			++ctx->fused_fallbacks;
			const void* src = ctx->job_src;
			ctx->job_src = nullptr;
			const size_t r = compress_device(ctx, src, ctx->job_T, ctx->job_bytes, ctx->job_dst, ctx->job_dst_size, ctx->job_stream, true);
			ctx->no_fused = false;
			return r;
		}
		ctx->job_src = nullptr;
		return (estatus || total > ctx->job_dst_size) ? STENOS_ERROR_DST_OVERFLOW : (size_t)total;
	}
	const uint32_t status = ctx->h_total->decode_status;
	if (const size_t e = status_error(status))
		return e;
	ctx->job_host_codes = (status & DECODE_STATUS_HOST_CODES) != 0;
	return ctx->job_expected;
}

} // namespace stenos_host
