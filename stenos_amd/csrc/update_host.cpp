// update_host.cpp -- rows of one frame in device memory replaced by row numbers that live on the device, the updated frame
// written to a second buffer (stenos_hip_update_rows, update.h).
#include "range_host_codes.h"
#include "update.h"

namespace stenos_host {

// The host knows the shape of the call and, after the first round trip, how many superblocks the rows touch (k); it never reads
// the row numbers.  On `stream`, in this order (the front end: frame_access.h):
//   the header fetch                                                                     (round trip 1)
//   one memset (words, counts, flags, prefixes), the old index into the update's own buffer (a copy of d_index, or the walk),
//   gather_count, gather_scan, gather_fill (gather.h: the pieces by superblock), update_plan, the words back   (round trip 2)
//   update_decode, [zstd-based codes of touched superblocks: HostCodes, one whole superblock each], update_apply,
//   enqueue_compress of the k slots as k superblocks without a frame header, update_splice_plan, the words back (round trip 3)
//   update_splice (the only writes to d_out), the new index into the context's, the wait for completion.
// Launches and round trips depend neither on n nor on the number of superblocks.  The index is copied first because a
// caller's index may be the context's own (sboff), which the encoder writes the k offsets of its stream into.
// Device memory, kept by the context between calls:
//   utab  the PiecePlan's tables (64 + 8 nsb + 8 (nsb + 1) + 16 * pieces) + 8 nsb (slot, touched) + 16 (nsb + 1) (old and new
//         index), each part rounded up to 64 bytes
//   uraw  k * sb                                       the touched superblocks, decoded
//   uenc  k * (sb + 4) + one superblock's worst case   their encodings
// and the encoder's workspace for k superblocks (ensure_workspace, slots): proportional to k, never to the array.
size_t update_rows(stenos_context_s* ctx, const void* d_frame, size_t T, size_t size, size_t row_bytes, size_t n, const uint64_t* d_rows, const void* d_src,
		   size_t src_stride, void* d_out, size_t out_size, const uint64_t* d_index, hipStream_t stream)
{
	const int level = ctx->level;
	if (T == 0 || T > STENOS_K_LDS_MAX_T || !PiecePlan::shape_ok(row_bytes, n, src_stride) || (ctx->job_kind && ctx->job_async))
		return STENOS_ERROR_INVALID_PARAMETER;
	if (needs_strategy(T, level) || level < 0 || ctx->max_nanoseconds) // what stenos_hip_compress_batch refuses to compress
		return STENOS_ERROR_INVALID_PARAMETER;
	FrameInfo fi;
	if (const size_t e = fetch_frame_info(d_frame, T, size, ~(size_t)0, stream, fi))
		return e;
	if (fi.total == 0 && n) // an array without rows: every row number is invalid
		return STENOS_ERROR_INVALID_PARAMETER;
	PiecePlan plan;
	if (!plan.init(fi, row_bytes, n))
		return STENOS_ERROR_INVALID_PARAMETER;
	ctx->job_kind = 0;
	// utab: the plan's tables, cleared by one memset up to the pieces, then [slot: nsb][touched: nsb][old index: nsb + 1][new index: nsb + 1]
	const size_t o_slot = plan.end, o_touched = o_slot + align64(fi.nsb * 4), o_idx = o_touched + align64(fi.nsb * 4), o_new = o_idx + align64((fi.nsb + 1) * 8),
		     tab_bytes = o_new + align64((fi.nsb + 1) * 8);
	if (!ctx->utab.ensure(tab_bytes))
		return STENOS_ERROR_ALLOC;
	uint8_t* const d = ctx->utab.as<uint8_t>();
	uint32_t* const d_words = (uint32_t*)d;
	uint64_t* const d_idx = (uint64_t*)(d + o_idx);
	uint64_t* const d_new = (uint64_t*)(d + o_new);
	auto fail = [&](size_t code = STENOS_ERROR_UNDEFINED) -> size_t {
		(void)hipStreamSynchronize(stream);
		return code;
	};
	if (hipMemsetAsync(d, 0, plan.o_pieces, stream) != hipSuccess)
		return fail();
	if (fi.nsb) {
		if (d_index) {
			if (hipMemcpyAsync(d_idx, d_index, (fi.nsb + 1) * 8, hipMemcpyDeviceToDevice, stream) != hipSuccess)
				return fail();
		}
		else if (const size_t e = frame_offsets(ctx, d_frame, size, fi, &d_index, d_idx, d_words + UPDATE_W_STATUS, stream))
			return fail(e);
	}
	// the context's index takes the new frame's at the end, and the encoder's offsets in between: if it has to grow, the copy
	// above (whose source it may be) is waited for first
	const size_t index_bytes = (fi.nsb + 8) * 8;
	ctx->last_frames = 0; // (a many-frame index in there does not survive this call)
	if (index_bytes > ctx->sboff.cap && hipStreamSynchronize(stream) != hipSuccess)
		return STENOS_ERROR_UNDEFINED;
	if (!ctx->sboff.ensure(index_bytes) || !ctx->misc.ensure(4096))
		return fail(STENOS_ERROR_ALLOC);

	UpdateArgs a = UpdateArgs();
	a.frame = (const uint8_t*)d_frame;
	a.size = size;
	a.idx = d_idx;
	a.new_idx = d_new;
	a.src = (const uint8_t*)d_src;
	a.out = (uint8_t*)d_out;
	a.total = fi.total;
	a.sb = (uint32_t)fi.sb;
	a.nsb = (uint32_t)fi.nsb;
	a.T = (uint32_t)T;
	a.header = (uint32_t)fi.header;
	a.words = d_words;
	a.ppre = (const uint32_t*)(d + plan.o_ppre);
	a.slot = (uint32_t*)(d + o_slot);
	a.touched = (uint32_t*)(d + o_touched);
	a.flags = (uint32_t*)(d + plan.o_flags);
	a.pieces = (const codec::GatherPiece*)(d + plan.o_pieces);
	volatile uint32_t* back = &ctx->h_total->decode_status; // (page-locked; 24 bytes from here on are the status words' of the decode paths)
	static_assert(offsetof(PinnedWords, decode_status) + 24 <= 64, "h_total");
	uint64_t new_total = fi.header;
	if (fi.nsb) {
		// (a piece's offset counts from the source rows)
		if (plan.npieces && !PiecePlan::enqueue(plan.args(d, d_frame, size, d_idx, fi, T, row_bytes, n, d_rows, src_stride, d_words + UPDATE_W_STATUS), stream))
			return fail();
		if (stenos_u_launch_plan(a, stream) != hipSuccess || hipMemcpyAsync((void*)back, d_words, 12, hipMemcpyDeviceToHost, stream) != hipSuccess ||
		    hipStreamSynchronize(stream) != hipSuccess)
			return fail();
		ctx->warm = true;
		uint32_t status = back[UPDATE_W_STATUS];
		if (const size_t e = status_error(status))
			return e;
		const uint64_t k = back[UPDATE_W_K], last = back[UPDATE_W_LAST];
		size_t enc_cap = 0;
		if (k) {
			if (k > fi.nsb || last >= fi.nsb)
				return STENOS_ERROR_UNDEFINED;
			const size_t bs = T * 256, raw_bytes = (size_t)(k - 1) * fi.sb + superblock_bytes(fi.total, fi.sb, last);
			FramePlan f;
			f.sb = fi.sb;
			f.shift = 0;
			f.header = 0;
			f.nsb = k;
			f.nfull = raw_bytes / bs;
			f.tail = (uint32_t)(raw_bytes % bs);
			f.bps = (uint32_t)(fi.sb / bs);
			// roomy: every superblock lies in the zone where no capacity rule applies (pipeline.h, safe_superblocks)
			enc_cap = (size_t)k * (fi.sb + 4) + (size_t)(f.bps + 1) * (bs + (T + 1) / 2) + 288 * T + 4096;
			if (!ctx->uraw.ensure((size_t)k * fi.sb + 64) || !ctx->uenc.ensure(enc_cap + 64))
				return STENOS_ERROR_ALLOC;
			a.k = (uint32_t)k;
			a.raw = ctx->uraw.as<uint8_t>();
			a.enc = ctx->uenc.as<uint8_t>();
			a.enc_off = ctx->sboff.as<uint64_t>();
			if (stenos_u_launch_decode(a, stream) != hipSuccess)
				return fail();
			if (status & DECODE_STATUS_HOST_CODES) {
				if (!zstd().ok)
					return fail(STENOS_ERROR_ZSTD_INTERNAL);
				// the compact list and the flags come down; every flagged superblock is decoded whole into its slot
				const size_t o_hflags = align64(k * 4);
				if (!ctx->h_utab.ensure(o_hflags + fi.nsb * 4) || !ctx->rtab.ensure(128) || !ctx->h_rtab.ensure(128))
					return fail(STENOS_ERROR_ALLOC);
				const uint32_t* const h_touched = (const uint32_t*)ctx->h_utab.data();
				const uint32_t* const h_flags = (const uint32_t*)(ctx->h_utab.data() + o_hflags);
				if (hipMemcpyAsync((void*)h_touched, a.touched, k * 4, hipMemcpyDeviceToHost, stream) != hipSuccess ||
				    hipMemcpyAsync((void*)h_flags, a.flags, fi.nsb * 4, hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess)
					return fail();
				HostCodes hc(ctx, d_frame, size, T, d_idx, fi, stream);
				for (uint64_t c = 0; c < k; ++c) {
					const uint32_t s = h_touched[c];
					if (s >= fi.nsb || !h_flags[s])
						continue;
					RangeUnit u;
					u.dst = a.raw + c * fi.sb;
					u.sb = s;
					u.lo = 0;
					u.hi = (uint32_t)superblock_bytes(fi.total, fi.sb, s);
					u.unused = 0;
					if (size_t err = hc.finish(u))
						return fail(err);
				}
			}
			if (stenos_u_launch_apply(a, stream) != hipSuccess)
				return fail();
			const size_t r = enqueue_compress(ctx, a.raw, T, raw_bytes, ctx->uenc.as<uint8_t>(), enc_cap, level, f, false, stream);
			ctx->last_nsb = 0; // (the context's index holds the encoder's offsets until the new frame's is in place)
			if (is_err(r))
				return fail(r);
		}
		if (stenos_u_launch_splice_plan(a, stream) != hipSuccess || hipMemcpyAsync((void*)back, d_words, 24, hipMemcpyDeviceToHost, stream) != hipSuccess ||
		    hipStreamSynchronize(stream) != hipSuccess)
			return fail();
		status = back[UPDATE_W_STATUS];
		if (const size_t e = status_error(status))
			return e;
		if (k && (ctx->h_total->encode_status || ctx->h_total->total > enc_cap)) // (the roomy stream cannot overflow)
			return STENOS_ERROR_UNDEFINED;
		new_total = (uint64_t)back[UPDATE_W_TOTAL] | ((uint64_t)back[UPDATE_W_TOTAL + 1] << 32);
	}
	if (new_total > out_size)
		return STENOS_ERROR_DST_OVERFLOW;
	if (stenos_u_launch_splice(a, stream) != hipSuccess)
		return fail();
	if (fi.nsb && hipMemcpyAsync(ctx->sboff.p, d_new, (fi.nsb + 1) * 8, hipMemcpyDeviceToDevice, stream) != hipSuccess)
		return fail();
	if (hipStreamSynchronize(stream) != hipSuccess)
		return STENOS_ERROR_UNDEFINED;
	ctx->warm = true;
	ctx->last_nsb = fi.nsb;
	ctx->last_batch = false;
	ctx->last_frames = 0;
	return (size_t)new_total;
}

} // namespace stenos_host
