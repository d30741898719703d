// update_batch_host.cpp -- rows of many frames in device memory replaced by (frame number, row number) pairs that live on the
// device, every updated frame written to a buffer of its own (stenos_hip_update_rows_batch, update_batch.h).  The frames' heads,
// the numbering and the walks come from the front end of the calls over many frames (frame_batch.h), the pieces from the batched
// gather's kernels, the encoding from the batch encoder's (batch.h); the planning, apply and splice rules are update_codec.h's.
#include <algorithm>

#include "frame_batch.h"
#include "range_host_codes.h"
#include "update_batch.h"

namespace stenos_host {

// The host knows the shape of the call and, after the second round trip, how many superblocks of each frame the pairs touch
// (k_f); it never reads the pairs.  On `stream`, in this order:
//   FrameBatch: the heads of all frames                                                                         (round trip 1)
//   one memset (k_f, words, counts, flags, prefixes), one upload of the frame tables, the old index into the call's own buffer
//   (a copy of d_index, or the walks), gather_batch_count, gather_scan, gather_batch_fill, update_batch_plan; the words and the
//   m pairs (k_f, last_f) back                                                                                  (round trip 2)
//   update_batch_decode, [zstd-based codes of touched superblocks: HostCodes, one whole superblock each], update_batch_apply,
//   one upload of the encoder's item tables, the batch encoder's kernels over one item without a frame header per touched frame
//   [a tiny last superblock: one more round trip, as in compress_batch], update_batch_splice_plan; the status, the m new sizes
//   and the encoder's states back                                                                               (round trip 3)
//   update_batch_splice (the only writes to the outputs), the new index into the context's, the wait for completion.
// Launches and round trips depend neither on n nor on the superblocks, and on m only through the parallel walks of long chains
// and the tiny and zstd host paths; host work and uploads are O(m).  The index is copied first because a caller's index may be
// the context's own (sboff), which the encoder writes its offsets into.
// Device memory, kept by the context between calls (S superblocks in all frames, K of them touched):
//   ubtab  O(m) tables (about 0.8 KB per frame: frame tables, walk arguments, the encoder's items) + the PiecePlan's tables
//          (64 + 8 S + 8 (S + 1) + 16 * pieces) + 8 S (slot, touched) + 16 (S + m) (old and new index) + 8 (S + 1) (sums),
//          each part rounded up to 64 bytes
//   uraw   K * sb                                                       the touched superblocks, decoded
//   uenc   K * (sb + 4) + one superblock's worst case per touched frame  their encodings
// and the batch encoder's workspace for K superblocks (ensure_workspace, slots): proportional to K, never to the arrays.
size_t update_rows_batch(stenos_context_s* ctx, size_t m, size_t T, const void* const* d_frames, const size_t* sizes, size_t row_bytes, size_t n,
			 const uint64_t* d_frame_ids, const uint64_t* d_rows, const void* d_src, size_t src_stride, void* const* d_outs, const size_t* out_sizes,
			 size_t* results, const uint64_t* d_index, hipStream_t stream)
{
	const int level = ctx->level;
	if (batch_shape_refused(ctx, m, T) || !PiecePlan::shape_ok(row_bytes, n, src_stride))
		return STENOS_ERROR_INVALID_PARAMETER;
	if (needs_strategy(T, level) || level < 0 || ctx->max_nanoseconds) // what stenos_hip_compress_batch refuses to compress
		return STENOS_ERROR_INVALID_PARAMETER;
	// the tables of O(m), mirrored on the host:
	//   BatchTables | [outs: m] up | [new sizes: m] down | [enc_base: m][FrameJob: m][bpre: m + 1][spre: m + 1][states: m][tiny list] up,
	//   states down | [tiny in] down [tiny out] up | [(k_f, last_f): m] down | o_plan: the tables of O(S) and O(pieces), device only
	const BatchTables t(m);
	const size_t o_outs = t.o_plan, o_totals = o_outs + align64(m * 8), o_ebase = o_totals + align64(m * 8), o_jobs = o_ebase + align64(m * 8),
		     o_bpre = o_jobs + align64(m * sizeof(codec::FrameJob)), o_spre = o_bpre + align64((m + 1) * 8), o_state = o_spre + align64((m + 1) * 8),
		     o_tiny = o_state + align64(m * sizeof(BatchItemState)), o_tin = o_tiny + align64(m * 4 + 4), o_tout = o_tin + align64(m * sizeof(BatchTinyIn)),
		     o_kf = o_tout + align64(m * sizeof(BatchTinyOut)), o_plan = o_kf + align64(m * 8);
	if (!ctx->ubtab.ensure(o_plan + 64) || !ctx->h_ubtab.ensure(o_plan + 64))
		return STENOS_ERROR_ALLOC;
	uint8_t* const h = ctx->h_ubtab.data();
	FrameBatch b{ ctx, m, d_frames, sizes, stream };
	if (const size_t e = fetch_frames(b, t, T, row_bytes, h, ctx->ubtab.as<uint8_t>()))
		return e;
	const uint64_t S = b.S;
	const codec::GatherFrame* const h_frames = (const codec::GatherFrame*)(h + t.o_frames);
	// one geometry: the touched superblocks of all frames are encoded in one pass
	size_t sb = 0;
	uint64_t P = 1;
	for (size_t f = 0; f < m; ++f) {
		if (!b.info[f].total)
			continue;
		if (sb && b.info[f].sb != sb)
			return STENOS_ERROR_INVALID_PARAMETER;
		sb = b.info[f].sb;
		P = std::max<uint64_t>(P, h_frames[f].pieces);
	}
	PiecePlan plan;
	if (S + m > 0x7FFFFFFFull || !plan.init(S, P, n)) // one workgroup per superblock and frame, one thread per piece
		return STENOS_ERROR_INVALID_PARAMETER;
	ctx->job_kind = 0;
	const size_t o_slot = o_plan + plan.end, o_touched = o_slot + align64(S * 4), o_idx = o_touched + align64(S * 4), o_new = o_idx + align64((S + m) * 8),
		     o_gpre = o_new + align64((S + m) * 8), tab_bytes = o_gpre + align64((S + 1) * 8);
	// (growing the buffer loses nothing: the mirror holds the tables, and they go up below)
	if (!ctx->ubtab.ensure(tab_bytes))
		return STENOS_ERROR_ALLOC;
	uint8_t* const d = ctx->ubtab.as<uint8_t>();
	uint8_t* const dp = d + o_plan;
	uint32_t* const d_words = (uint32_t*)dp;
	uint64_t* const d_idx = (uint64_t*)(d + o_idx);
	uint64_t* const d_new = (uint64_t*)(d + o_new);
	auto fail = [&](size_t code = STENOS_ERROR_UNDEFINED) -> size_t {
		(void)hipStreamSynchronize(stream); // (nothing may still read the page-locked mirror)
		return code;
	};
	for (size_t f = 0; f < m; ++f) {
		((uint64_t*)(h + t.o_header))[f] = b.info[f].header;
		((void**)(h + o_outs))[f] = d_outs[f];
	}
	if (hipMemsetAsync(d + o_kf, 0, o_plan - o_kf + plan.o_pieces, stream) != hipSuccess)
		return fail();
	if (d_index) {
		if (hipMemcpyAsync(d + t.o_frames, h + t.o_frames, o_totals - t.o_frames, hipMemcpyHostToDevice, stream) != hipSuccess ||
		    hipMemcpyAsync(d_idx, d_index, (S + m) * 8, hipMemcpyDeviceToDevice, stream) != hipSuccess)
			return fail();
	}
	else if (const size_t e = walk_frames(b, t, d_words + UPDATE_W_STATUS, h, d, d_idx, o_totals))
		return fail(e);
	// the context's index takes the new frames' at the end, and the encoder's offsets in between: if it has to grow, the copy
	// above (whose source it may be) is waited for first
	const size_t index_bytes = (S + m + 8) * 8;
	ctx->last_nsb = 0;
	ctx->last_batch = true;
	ctx->last_frames = 0;
	if (index_bytes > ctx->sboff.cap && hipStreamSynchronize(stream) != hipSuccess)
		return STENOS_ERROR_UNDEFINED;
	if (!ctx->sboff.ensure(index_bytes) || !ctx->misc.ensure(4096))
		return fail(STENOS_ERROR_ALLOC);

	UpdateBatchArgs a = UpdateBatchArgs();
	a.frames = (const codec::GatherFrame*)(d + t.o_frames);
	a.first = (const uint64_t*)(d + t.o_first);
	a.header = (const uint64_t*)(d + t.o_header);
	a.outs = (uint8_t* const*)(d + o_outs);
	a.idx = d_idx;
	a.new_idx = d_new;
	a.gpre = (uint64_t*)(d + o_gpre);
	a.totals = (uint64_t*)(d + o_totals);
	a.enc_base = (const uint64_t*)(d + o_ebase);
	a.src = (const uint8_t*)d_src;
	a.sb = (uint32_t)sb;
	a.m = (uint32_t)m;
	a.S = (uint32_t)S;
	a.T = (uint32_t)T;
	a.words = d_words;
	a.ppre = (const uint32_t*)(dp + plan.o_ppre);
	a.slot = (uint32_t*)(d + o_slot);
	a.touched = (uint32_t*)(d + o_touched);
	a.flags = (uint32_t*)(dp + plan.o_flags);
	a.kf = (uint32_t*)(d + o_kf);
	a.pieces = (const codec::GatherPiece*)(dp + plan.o_pieces);
	if (plan.npieces) { // (a piece's offset counts from the source rows)
		GatherBatchArgs g = GatherBatchArgs();
		g.frames = a.frames;
		g.first = a.first;
		g.sb_off = d_idx;
		g.frame_ids = d_frame_ids;
		g.rows = d_rows;
		g.row_bytes = row_bytes;
		g.dst_stride = src_stride;
		g.npieces = plan.npieces;
		g.m = a.m;
		g.P = (uint32_t)P;
		g.S = a.S;
		g.T = a.T;
		g.status = d_words + UPDATE_W_STATUS;
		g.count = (uint32_t*)(dp + plan.o_count);
		g.sb_flags = a.flags;
		g.ppre = (uint32_t*)(dp + plan.o_ppre);
		g.wpre = (uint32_t*)(dp + plan.o_wpre);
		g.pieces = (codec::GatherPiece*)(dp + plan.o_pieces);
		GatherArgs scan = GatherArgs(); // gather_scan reads the tables and their length, nothing else
		scan.nsb = g.S;
		scan.count = g.count;
		scan.ppre = g.ppre;
		scan.wpre = g.wpre;
		if (stenos_gb_launch_count(g, stream) != hipSuccess || stenos_g_launch_scan(scan, stream) != hipSuccess || stenos_gb_launch_fill(g, stream) != hipSuccess)
			return fail();
	}
	volatile uint32_t* back = &ctx->h_total->decode_status; // (page-locked; 24 bytes from here on are the status words' of the decode paths)
	const uint32_t* const h_kf = (const uint32_t*)(h + o_kf);
	if (stenos_ub_launch_plan(a, stream) != hipSuccess || hipMemcpyAsync((void*)back, d_words, 12, hipMemcpyDeviceToHost, stream) != hipSuccess ||
	    hipMemcpyAsync(h + o_kf, d + o_kf, m * 8, hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess)
		return fail();
	ctx->warm = true;
	uint32_t status = back[UPDATE_W_STATUS];
	if (const size_t e = status_error(status))
		return e;
	const uint64_t K = back[UPDATE_W_K];
	BatchItemState* const h_state = (BatchItemState*)(h + o_state);
	std::vector<size_t> cap(m, 0); // capacity of frame f's encoded stream
	if (K) {
		// one item without a frame header per touched frame: its k_f slots are one run of the compact list
		const size_t bs = T * 256;
		const uint32_t bps = (uint32_t)(sb / bs), stride = stenos_k_slot_stride((uint32_t)T);
		// roomy: every superblock lies in the zone where no capacity rule applies (pipeline.h, safe_superblocks)
		const size_t pad = ((size_t)(bps + 1) * (bs + (T + 1) / 2) + 288 * T + 4096 + 63) & ~(size_t)63;
		uint64_t c0 = 0, b0 = 0, e0 = 0;
		std::vector<uint32_t> tiny;
		std::vector<FramePlan> fp(m);
		for (size_t f = 0; f < m; ++f) {
			const uint64_t k = h_kf[2 * f], last = h_kf[2 * f + 1];
			if (k > b.nsb(f) || (k && last >= b.nsb(f)) || c0 + k > K)
				return STENOS_ERROR_UNDEFINED;
			FramePlan& p = fp[f];
			p.sb = sb;
			p.shift = 0;
			p.header = 0;
			p.bps = bps;
			if (k) {
				const size_t last_bytes = superblock_bytes(b.info[f].total, sb, last), raw_bytes = (size_t)(k - 1) * sb + last_bytes;
				p.nsb = k;
				p.nfull = raw_bytes / bs;
				p.tail = (uint32_t)(raw_bytes % bs);
				cap[f] = (size_t)k * (sb + 4) + pad;
				if (level >= 1 && last_bytes < 128)
					tiny.push_back((uint32_t)f);
			}
			c0 += k;
			b0 += p.nfull + (p.tail ? 1 : 0);
			e0 += cap[f];
		}
		const uint64_t B = b0;
		if (c0 != K || K * codec::PACK_WAVES >= 0x7FFFFFFFull || B >= 0x7FFFFFFFull) // one workgroup per unit of work
			return STENOS_ERROR_INVALID_PARAMETER;
		const size_t ntiny = tiny.size();
		if (ntiny && !zstd().ok)
			return STENOS_ERROR_ZSTD_INTERNAL;
		if (!ctx->uraw.ensure((size_t)K * sb + 64) || !ctx->uenc.ensure((size_t)e0 + 64) || !ctx->slots.ensure((level >= 1 ? B : 0) * stride + 64) ||
		    !ensure_workspace(ctx, B, K, m))
			return STENOS_ERROR_ALLOC;
		a.K = (uint32_t)K;
		a.raw = ctx->uraw.as<uint8_t>();
		a.enc = ctx->uenc.as<uint8_t>();
		a.enc_off = ctx->sboff.as<uint64_t>();
		if (stenos_ub_launch_decode(a, stream) != hipSuccess)
			return fail();
		if (status & DECODE_STATUS_HOST_CODES) {
			if (!zstd().ok)
				return fail(STENOS_ERROR_ZSTD_INTERNAL);
			// the compact list and the flags come down; every flagged superblock is decoded whole into its slot
			const size_t o_hflags = align64(K * 4);
			if (!ctx->h_utab.ensure(o_hflags + S * 4) || !ctx->rtab.ensure(128) || !ctx->h_rtab.ensure(128))
				return fail(STENOS_ERROR_ALLOC);
			const uint32_t* const h_touched = (const uint32_t*)ctx->h_utab.data();
			const uint32_t* const h_flags = (const uint32_t*)(ctx->h_utab.data() + o_hflags);
			if (hipMemcpyAsync((void*)h_touched, a.touched, K * 4, hipMemcpyDeviceToHost, stream) != hipSuccess ||
			    hipMemcpyAsync((void*)h_flags, a.flags, S * 4, hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess)
				return fail();
			for (uint64_t c = 0; c < K; ++c) {
				const uint32_t g = h_touched[c];
				if (g >= S || !h_flags[g])
					continue;
				const size_t f = (size_t)(std::upper_bound(b.first.begin(), b.first.end(), (uint64_t)g) - b.first.begin()) - 1;
				HostCodes hc(ctx, d_frames[f], sizes[f], T, d_idx + b.first[f] + f, b.info[f], stream);
				RangeUnit u;
				u.dst = a.raw + c * sb;
				u.sb = (uint32_t)(g - b.first[f]);
				u.lo = 0;
				u.hi = (uint32_t)superblock_bytes(b.info[f].total, sb, u.sb);
				u.unused = 0;
				if (size_t err = hc.finish(u))
					return fail(err);
			}
		}
		if (stenos_ub_launch_apply(a, stream) != hipSuccess)
			return fail();
		// the encoder's item tables (compress_batch's, batch_host.cpp): frame f's item reads its run of slots and writes its own
		// stream; a frame that no pair names is an item without superblocks, which the kernels leave alone
		codec::FrameJob* const h_jobs = (codec::FrameJob*)(h + o_jobs);
		uint64_t* const h_bpre = (uint64_t*)(h + o_bpre);
		uint64_t* const h_spre = (uint64_t*)(h + o_spre);
		uint64_t* const h_ebase = (uint64_t*)(h + o_ebase);
		const codec::FrameJob* const d_jobs = (const codec::FrameJob*)(d + o_jobs);
		BatchItemState* const d_state = (BatchItemState*)(d + o_state);
		BatchTinyOut* const d_tout = (BatchTinyOut*)(d + o_tout);
		c0 = b0 = e0 = 0;
		size_t k_tiny = 0;
		for (size_t f = 0; f < m; ++f) {
			const FramePlan& p = fp[f];
			const uint64_t nb = p.nfull + (p.tail ? 1 : 0);
			const size_t raw_bytes = (size_t)p.nfull * bs + p.tail;
			h_bpre[f] = b0;
			h_spre[f] = c0;
			h_ebase[f] = e0;
			h_state[f] = { 0, 0, 0xFFFFFFFFu };
			codec::FrameJob j;
			if (!frame_job(ctx, p, T, raw_bytes, b0, c0, f, j))
				return fail(STENOS_ERROR_ALLOC);
			j.src = a.raw + c0 * sb;
			j.dst = ctx->uenc.as<uint8_t>() + e0;
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
			b0 += nb;
			c0 += p.nsb;
			e0 += cap[f];
		}
		h_bpre[m] = b0;
		h_spre[m] = c0;
		memcpy(h + o_tiny, tiny.data(), ntiny * 4);
		const uint64_t* const d_bpre = (const uint64_t*)(d + o_bpre);
		const uint64_t* const d_spre = (const uint64_t*)(d + o_spre);
		const uint32_t* const d_tiny = (const uint32_t*)(d + o_tiny);
		const uint32_t um = (uint32_t)m;
		if (hipMemcpyAsync(d + o_ebase, h + o_ebase, o_tin - o_ebase, hipMemcpyHostToDevice, stream) != hipSuccess)
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
			for (size_t k = 0; k < ntiny; ++k) {
				const size_t f = tiny[k];
				const BatchTinyIn& in = h_tin[k];
				BatchTinyOut& out = h_tout[k];
				memset(&out, 0, sizeof(out));
				const size_t last_bytes = ((size_t)fp[f].nfull * bs + fp[f].tail) - (size_t)(fp[f].nsb - 1) * sb;
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
		if (stenos_b_launch_pack(d_jobs, d_spre, um, K, bps, stream) != hipSuccess ||
		    hipMemcpyAsync(h_state, d_state, m * sizeof(BatchItemState), hipMemcpyDeviceToHost, stream) != hipSuccess)
			return fail();
	}
	uint64_t* const h_totals = (uint64_t*)(h + o_totals);
	if (stenos_ub_launch_splice_plan(a, stream) != hipSuccess || hipMemcpyAsync((void*)back, d_words, 4, hipMemcpyDeviceToHost, stream) != hipSuccess ||
	    hipMemcpyAsync(h_totals, d + o_totals, m * 8, hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess)
		return fail();
	status = back[UPDATE_W_STATUS];
	if (const size_t e = status_error(status))
		return e;
	for (size_t f = 0; K && f < m; ++f)
		if (cap[f] && (h_state[f].status || h_state[f].total > cap[f])) // (the roomy streams cannot overflow)
			return STENOS_ERROR_UNDEFINED;
	for (size_t f = 0; f < m; ++f)
		if (h_totals[f] > out_sizes[f])
			return STENOS_ERROR_DST_OVERFLOW;
	if (stenos_ub_launch_splice(a, stream) != hipSuccess)
		return fail();
	if (hipMemcpyAsync(ctx->sboff.p, d_new, (S + m) * 8, hipMemcpyDeviceToDevice, stream) != hipSuccess)
		return fail();
	if (hipStreamSynchronize(stream) != hipSuccess)
		return STENOS_ERROR_UNDEFINED;
	for (size_t f = 0; f < m; ++f)
		results[f] = (size_t)h_totals[f];
	ctx->last_nsb = 0;
	ctx->last_batch = true;
	ctx->last_frames = (size_t)(S + m);
	return 0;
}

} // namespace stenos_host
