// append_host.cpp -- bytes in device memory appended to the array of one frame in device memory, in place
// (stenos_hip_append, append.h).
#include "range_host_codes.h"
#include "append.h"

namespace stenos_host {

// The frame of A||B starts with the frame of A up to A's last whole superblock (superblocks are encoded independently), so only
// the stream from the header of superblock keep = floor(|A| / sb) on is made anew: it encodes (last r = |A| mod sb bytes of
// A)||B.  The host knows the sizes and, after the second round trip, where that stream starts (p).  On `stream`, in this order
// (the front end: frame_access.h):
//   the header fetch                                                                                       (round trip 1)
//   one memset (the words), the old index into the append's own buffer (a copy of d_index, or the walk), append_plan, the
//   words back                                                                                             (round trip 2)
//   [r > 0: append_decode of superblock keep into the stitch buffer (a zstd-based code: HostCodes), the first min(|B|, sb - r)
//   bytes of B behind it (one device copy)], one upload of the encoder's item tables, the batch encoder's kernels over the
//   stitched superblock and the rest of B (read where the caller has it) as two items without a frame header
//   [a tiny new last superblock: one more round trip, as in compress_batch], append_commit_plan; the words and the
//   encoder's states back                                                                                  (round trip 3)
//   append_commit (the only writes to d_frame), the new index into the context's, the wait for completion.
// Launches and round trips depend neither on the sizes nor on the number of superblocks.  The index is copied first because a
// caller's index may be the context's own (sboff), which the encoder writes the offsets of its streams into.
// Device memory, kept by the context between calls (k new superblocks):
//   atab  64 (words) + about 1 KB (the encoder's item tables) + 8 per superblock of the new frame (the index)
//   araw  one superblock: the stitch buffer
//   aenc  k * (sb + 4) + one superblock's worst case per stream: the encodings
// and the batch encoder's workspace for k superblocks (ensure_workspace, slots): proportional to r + |B|, never to the array,
// but for the 8 bytes of index per superblock here and in the context's index.
size_t append(stenos_context_s* ctx, void* d_frame, size_t T, size_t size, size_t capacity, const void* d_src, size_t src_bytes, const uint64_t* d_index,
	      hipStream_t stream)
{
	const int level = ctx->level;
	constexpr uint64_t kMaxArray = ((uint64_t)1 << 56) - 1; // the header's size field
	if (capacity < size || T == 0 || T > STENOS_K_LDS_MAX_T || (uint64_t)src_bytes > kMaxArray || (ctx->job_kind && ctx->job_async))
		return STENOS_ERROR_INVALID_PARAMETER;
	if (needs_strategy(T, level) || level < 0 || ctx->max_nanoseconds) // what stenos_hip_compress_batch refuses to compress
		return STENOS_ERROR_INVALID_PARAMETER;
	FrameInfo fi;
	if (const size_t e = fetch_frame_info(d_frame, T, size, ~(size_t)0, stream, fi))
		return e;
	if (fi.total > kMaxArray - src_bytes)
		return STENOS_ERROR_INVALID_PARAMETER;
	if (fi.total == 0) {
		// the frame of an empty array carries no geometry: B is compressed under the context's settings
		if (src_bytes == 0)
			return fi.header;
		return compress_device(ctx, d_src, T, src_bytes, d_frame, capacity, stream, true);
	}
	const size_t bs = T * 256, sb = fi.sb;
	if (sb % bs)
		return STENOS_ERROR_INVALID_INPUT;
	const uint64_t new_bytes = fi.total + src_bytes, keep = fi.total / sb, nsb_new = new_bytes / sb + (new_bytes % sb ? 1 : 0);
	const size_t r = (size_t)(fi.total % sb);
	if (nsb_new > 0x7FFFFFFFull)
		return STENOS_ERROR_INVALID_PARAMETER;
	const uint64_t k = nsb_new - keep;
	ctx->job_kind = 0;
	// atab and its page-locked mirror: [words: 64] | [FrameJob: 2][bpre: 3][spre: 3][states: 2][tiny list] up, states down |
	// [tiny in] down [tiny out] up | the index, device only
	const size_t o_jobs = 64, o_bpre = o_jobs + align64(2 * sizeof(codec::FrameJob)), o_spre = o_bpre + 64, o_state = o_spre + 64,
		     o_tiny = o_state + align64(2 * sizeof(BatchItemState)), o_tin = o_tiny + 64, o_tout = o_tin + align64(2 * sizeof(BatchTinyIn)),
		     o_idx = o_tout + align64(2 * sizeof(BatchTinyOut)), tab_bytes = o_idx + align64((nsb_new + 2) * 8);
	if (!ctx->atab.ensure(tab_bytes) || !ctx->h_atab.ensure(o_idx))
		return STENOS_ERROR_ALLOC;
	uint8_t* const d = ctx->atab.as<uint8_t>();
	uint8_t* const h = ctx->h_atab.data();
	uint32_t* const d_words = (uint32_t*)d;
	volatile uint32_t* const h_words = (volatile uint32_t*)h;
	uint64_t* const d_idx = (uint64_t*)(d + o_idx);
	auto fail = [&](size_t code = STENOS_ERROR_UNDEFINED) -> size_t {
		(void)hipStreamSynchronize(stream); // (nothing may still read the page-locked mirror)
		return code;
	};
	auto word64 = [&](uint32_t w) { return (uint64_t)h_words[w] | ((uint64_t)h_words[w + 1] << 32); };
	if (hipMemsetAsync(d, 0, 64, stream) != hipSuccess)
		return fail();
	if (d_index) {
		if (hipMemcpyAsync(d_idx, d_index, (fi.nsb + 1) * 8, hipMemcpyDeviceToDevice, stream) != hipSuccess)
			return fail();
	}
	else if (const size_t e = frame_offsets(ctx, d_frame, size, fi, &d_index, d_idx, d_words + APPEND_W_STATUS, stream))
		return fail(e);
	// the context's index takes the new frame's at the end, and the encoder's offsets in between: if it has to grow, the copy
	// above (whose source it may be) is waited for first
	const size_t index_bytes = (nsb_new + 16) * 8;
	ctx->last_nsb = 0;
	ctx->last_batch = false;
	ctx->last_frames = 0;
	if (index_bytes > ctx->sboff.cap && hipStreamSynchronize(stream) != hipSuccess)
		return STENOS_ERROR_UNDEFINED;
	if (!ctx->sboff.ensure(index_bytes) || !ctx->misc.ensure(4096))
		return fail(STENOS_ERROR_ALLOC);

	AppendArgs a = AppendArgs();
	a.frame = (uint8_t*)d_frame;
	a.size = size;
	a.idx = d_idx;
	a.new_bytes = new_bytes;
	a.keep = (uint32_t)keep;
	a.r = (uint32_t)r;
	a.k = (uint32_t)k;
	a.k0 = r ? 1u : 0u;
	a.header = (uint32_t)fi.header;
	a.words = d_words;
	uint64_t chain_end = 0; // (src_bytes == 0: what the call returns)
	if (stenos_a_launch_plan(a, stream) != hipSuccess || hipMemcpyAsync(h, d_words, 64, hipMemcpyDeviceToHost, stream) != hipSuccess ||
	    (src_bytes == 0 && hipMemcpyAsync(&chain_end, d_idx + fi.nsb, 8, hipMemcpyDeviceToHost, stream) != hipSuccess) || hipStreamSynchronize(stream) != hipSuccess)
		return fail();
	ctx->warm = true;
	uint32_t status = h_words[APPEND_W_STATUS];
	if (const size_t e = status_error(status))
		return e;
	if (src_bytes == 0)
		return (size_t)chain_end;

	// the streams: [0] the stitched superblock (r > 0), [1] the rest of B
	const size_t n0 = r ? (src_bytes < sb - r ? src_bytes : sb - r) : 0;
	struct Item {
		const uint8_t* src;
		size_t bytes;
	} items[2];
	size_t m = 0;
	if (r) {
		if (!ctx->araw.ensure(sb + 64))
			return STENOS_ERROR_ALLOC;
		uint8_t* const raw = ctx->araw.as<uint8_t>();
		if (stenos_a_launch_decode(a, raw, fi.total, (uint32_t)sb, (uint32_t)T, stream) != hipSuccess)
			return fail();
		if (status & DECODE_STATUS_HOST_CODES) {
			if (!zstd().ok)
				return fail(STENOS_ERROR_ZSTD_INTERNAL);
			if (!ctx->rtab.ensure(128) || !ctx->h_rtab.ensure(128))
				return fail(STENOS_ERROR_ALLOC);
			HostCodes hc(ctx, d_frame, size, T, d_idx, fi, stream);
			RangeUnit u;
			u.dst = raw;
			u.sb = (uint32_t)keep;
			u.lo = 0;
			u.hi = (uint32_t)r;
			u.unused = 0;
			if (size_t err = hc.finish(u))
				return fail(err);
		}
		if (hipMemcpyAsync(raw + r, d_src, n0, hipMemcpyDeviceToDevice, stream) != hipSuccess)
			return fail();
		items[m++] = { raw, r + n0 };
	}
	if (src_bytes > n0)
		items[m++] = { (const uint8_t*)d_src + n0, src_bytes - n0 };

	const uint32_t bps = (uint32_t)(sb / bs), stride = stenos_k_slot_stride((uint32_t)T);
	// roomy: every superblock lies in the zone where no capacity rule applies (pipeline.h, safe_superblocks)
	const size_t pad = ((size_t)(bps + 1) * (bs + (T + 1) / 2) + 288 * T + 4096 + 63) & ~(size_t)63;
	FramePlan fp[2];
	size_t cap[2] = { 0, 0 };
	uint64_t B = 0, K = 0, e_all = 0;
	uint32_t tiny[2];
	size_t ntiny = 0;
	for (size_t f = 0; f < m; ++f) {
		FramePlan& p = fp[f];
		p.sb = sb;
		p.shift = 0;
		p.header = 0;
		p.bps = bps;
		p.nsb = items[f].bytes / sb + (items[f].bytes % sb ? 1 : 0);
		p.nfull = items[f].bytes / bs;
		p.tail = (uint32_t)(items[f].bytes % bs);
		cap[f] = (size_t)p.nsb * (sb + 4) + pad;
		if (level >= 1 && superblock_bytes(items[f].bytes, sb, p.nsb - 1) < 128)
			tiny[ntiny++] = (uint32_t)f;
		B += p.nfull + (p.tail ? 1 : 0);
		K += p.nsb;
		e_all += cap[f];
	}
	if (K != k)
		return fail(STENOS_ERROR_UNDEFINED);
	if (K * codec::PACK_WAVES >= 0x7FFFFFFFull || B >= 0x7FFFFFFFull) // one workgroup per unit of work
		return fail(STENOS_ERROR_INVALID_PARAMETER);
	if (ntiny && !zstd().ok)
		return fail(STENOS_ERROR_ZSTD_INTERNAL);
	if (!ctx->aenc.ensure((size_t)e_all + 64) || !ctx->slots.ensure((level >= 1 ? B : 0) * stride + 64) || !ensure_workspace(ctx, B, K, m))
		return fail(STENOS_ERROR_ALLOC);
	a.enc = ctx->aenc.as<uint8_t>();
	a.enc_off = ctx->sboff.as<uint64_t>();
	a.enc_base1 = m == 2 ? cap[0] : 0;

	// the encoder's item tables (compress_batch's, batch_host.cpp)
	codec::FrameJob* const h_jobs = (codec::FrameJob*)(h + o_jobs);
	uint64_t* const h_bpre = (uint64_t*)(h + o_bpre);
	uint64_t* const h_spre = (uint64_t*)(h + o_spre);
	BatchItemState* const h_state = (BatchItemState*)(h + o_state);
	const codec::FrameJob* const d_jobs = (const codec::FrameJob*)(d + o_jobs);
	BatchItemState* const d_state = (BatchItemState*)(d + o_state);
	BatchTinyOut* const d_tout = (BatchTinyOut*)(d + o_tout);
	uint64_t b0 = 0, c0 = 0, e0 = 0;
	size_t k_tiny = 0;
	for (size_t f = 0; f < m; ++f) {
		const FramePlan& p = fp[f];
		h_bpre[f] = b0;
		h_spre[f] = c0;
		h_state[f] = { 0, 0, 0xFFFFFFFFu };
		codec::FrameJob j;
		if (!frame_job(ctx, p, T, items[f].bytes, b0, c0, f, j))
			return fail(STENOS_ERROR_ALLOC);
		j.src = items[f].src;
		j.dst = ctx->aenc.as<uint8_t>() + e0;
		j.dst_size = cap[f];
		j.slots = ctx->slots.as<uint8_t>() + (level >= 1 ? b0 * stride : 0);
		j.total = &d_state[f].total;
		j.status = &d_state[f].status;
		j.first_flagged = &d_state[f].first_flagged;
		const bool is_tiny = k_tiny < ntiny && tiny[k_tiny] == f;
		j.override_payload = is_tiny ? d_tout[k_tiny].payload : nullptr;
		k_tiny += is_tiny ? 1 : 0;
		j.shift_byte = 0xFFFFFFFFu; // (no frame header)
		j.header_bytes = 0;
		j.force_copy = level == 0 ? 1u : 0u;
		j.tiny_last = is_tiny ? 1u : 0u;
		j.check_total = 1;
		h_jobs[f] = j;
		b0 += p.nfull + (p.tail ? 1 : 0);
		c0 += p.nsb;
		e0 += cap[f];
	}
	h_bpre[m] = b0;
	h_spre[m] = c0;
	memcpy(h + o_tiny, tiny, ntiny * 4);
	const uint64_t* const d_bpre = (const uint64_t*)(d + o_bpre);
	const uint64_t* const d_spre = (const uint64_t*)(d + o_spre);
	const uint32_t* const d_tiny = (const uint32_t*)(d + o_tiny);
	const uint32_t um = (uint32_t)m;
	if (hipMemcpyAsync(d + o_jobs, h + o_jobs, o_tin - o_jobs, hipMemcpyHostToDevice, stream) != hipSuccess)
		return fail();
	if ((level >= 1 && stenos_b_launch_encode(d_jobs, d_bpre, um, B, (uint32_t)T, stream) != hipSuccess) || stenos_b_launch_plan(d_jobs, d_spre, um, K, stream) != hipSuccess ||
	    stenos_b_launch_scan(d_jobs, um, stream) != hipSuccess || stenos_b_launch_resolve(d_jobs, um, (uint32_t)T, stream) != hipSuccess)
		return fail();
	if (ntiny) { // (compress_batch's round trip: zstd is given the room behind the superblock's header, which is ample here)
		BatchTinyIn* const h_tin = (BatchTinyIn*)(h + o_tin);
		BatchTinyOut* const h_tout = (BatchTinyOut*)(h + o_tout);
		if (stenos_b_launch_tiny_gather(d_jobs, d_tiny, (uint32_t)ntiny, (BatchTinyIn*)(d + o_tin), stream) != hipSuccess ||
		    hipMemcpyAsync(h_tin, d + o_tin, ntiny * sizeof(BatchTinyIn), hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess)
			return fail();
		for (size_t t = 0; t < ntiny; ++t) {
			const size_t f = tiny[t];
			const BatchTinyIn& in = h_tin[t];
			BatchTinyOut& out = h_tout[t];
			memset(&out, 0, sizeof(out));
			const size_t last_bytes = superblock_bytes(items[f].bytes, sb, fp[f].nsb - 1);
			if (in.status || cap[f] < in.off_last + 4) // (neither happens in a roomy stream; the item then reports an overflow)
				continue;
			const size_t room = cap[f] - (size_t)in.off_last - 4;
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
	if (stenos_b_launch_pack(d_jobs, d_spre, um, K, bps, stream) != hipSuccess || stenos_a_launch_commit_plan(a, stream) != hipSuccess ||
	    hipMemcpyAsync(h_state, d_state, m * sizeof(BatchItemState), hipMemcpyDeviceToHost, stream) != hipSuccess ||
	    hipMemcpyAsync(h, d_words, 64, hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess)
		return fail();
	status = h_words[APPEND_W_STATUS];
	if (const size_t e = status_error(status))
		return e;
	for (size_t f = 0; f < m; ++f)
		if (h_state[f].status || h_state[f].total > cap[f]) // (the roomy streams cannot overflow)
			return STENOS_ERROR_UNDEFINED;
	const uint64_t new_total = word64(APPEND_W_TOTAL), len0 = word64(APPEND_W_LEN0), len1 = word64(APPEND_W_LEN1);
	if (len0 + len1 > e_all || new_total != word64(APPEND_W_P) + len0 + len1)
		return STENOS_ERROR_UNDEFINED;
	if (new_total > capacity)
		return STENOS_ERROR_DST_OVERFLOW;
	if (stenos_a_launch_commit(a, len0, len1, stream) != hipSuccess)
		return fail();
	if (hipMemcpyAsync(ctx->sboff.p, d_idx, (nsb_new + 1) * 8, hipMemcpyDeviceToDevice, stream) != hipSuccess)
		return fail();
	if (hipStreamSynchronize(stream) != hipSuccess)
		return STENOS_ERROR_UNDEFINED;
	ctx->last_nsb = nsb_new;
	ctx->last_batch = false;
	ctx->last_frames = 0;
	return (size_t)new_total;
}

} // namespace stenos_host
