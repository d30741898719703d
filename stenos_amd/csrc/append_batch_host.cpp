// append_batch_host.cpp -- bytes in device memory appended to the arrays of many frames in device memory, in place, in one call
// (stenos_hip_append_batch, append_batch.h).  The frames' heads, the numbering and the walks come from the front end of the
// calls over many frames (frame_batch.h), the encoding from the batch encoder's kernels (batch.h); the rules are
// append_codec.h's, applied frame by frame (append_batch_codec.h).
#include <algorithm>

#include "frame_batch.h"
#include "range_host_codes.h"
#include "append_batch.h"

namespace stenos_host {

// The in-place commit would race with itself: no two frame buffers [d_frames[f], + capacities[f]) may overlap, and no source
// [d_srcs[f], + src_sizes[f]) may overlap a frame buffer (sources may overlap each other: they are only read).
bool append_batch_overlap(size_t m, void* const* d_frames, const size_t* capacities, const void* const* d_srcs, const size_t* src_sizes)
{
	struct Interval {
		uintptr_t lo, hi;
		bool frame;
	};
	std::vector<Interval> v;
	v.reserve(2 * m);
	for (size_t f = 0; f < m; ++f) {
		const uintptr_t p = (uintptr_t)d_frames[f];
		if (capacities[f] > ~(uintptr_t)0 - p || (src_sizes[f] && src_sizes[f] > ~(uintptr_t)0 - (uintptr_t)d_srcs[f]))
			return true; // (a buffer that wraps around the address space)
		if (capacities[f])
			v.push_back({ p, p + capacities[f], true });
		if (src_sizes[f])
			v.push_back({ (uintptr_t)d_srcs[f], (uintptr_t)d_srcs[f] + src_sizes[f], false });
	}
	std::sort(v.begin(), v.end(), [](const Interval& x, const Interval& y) { return x.lo < y.lo; });
	uintptr_t frames_end = 0, srcs_end = 0; // the largest ends so far
	for (const Interval& x : v) {
		if (x.lo < frames_end || (x.frame && x.lo < srcs_end))
			return true;
		(x.frame ? frames_end : srcs_end) = std::max(x.frame ? frames_end : srcs_end, x.hi);
	}
	return false;
}

// The host knows the sizes of everything but the encodings.  On `stream`, in this order:
//   FrameBatch: the heads of all frames                                                                         (round trip 1)
//   one memset (words, flags, lengths), one upload of the frame tables, the old index into the call's own buffer (a copy of
//   d_index, or the walks), append_batch_plan; the status, the flags and the ends of untouched chains back      (round trip 2)
//   append_batch_decode [zstd-based codes: HostCodes, one frame at a time], append_batch_stitch, one upload of the encoder's item
//   tables, the batch encoder's kernels over up to 2 m items (the stitched superblock of a frame, the rest of its B_f read where
//   the caller has it; both without a frame header, the one item of the frame of an empty array with one) [tiny new last
//   superblocks: one more round trip for all of them, as in compress_batch], append_batch_commit_plan, append_batch_index; the
//   status, the streams' bytes, the m totals and the encoder's states back                                       (round trip 3)
//   one upload (the commit's chunk table), append_batch_commit (the only writes to the frames), the new index into the
//   context's, the wait for completion.
// Launches and round trips depend neither on the bytes nor on the superblocks, and on m only through the parallel walks of long
// chains and the tiny and zstd host paths; host work and uploads are O(m).  The index is copied first because a caller's index
// may be the context's own (sboff), which the encoder writes its offsets into.
// Device memory, kept by the context between calls (S old and S' new superblocks in all frames, k_i new superblocks in item i):
//   abtab  O(m) tables (about 1.3 KB per frame: frame tables, walk arguments, the encoder's items, the words) + 8 (S + m) +
//          8 (S' + m) (old and new index)
//   abraw  r_f + n0_f per frame with a partial last superblock, rounded up to 64: the stitch slots
//   abenc  k_i * (sb + 4) + one superblock's worst case PER ITEM (the roomy pad: capacity rules would change output bytes)
// and the batch encoder's workspace for all new superblocks (ensure_workspace, slots).
size_t append_batch(stenos_context_s* ctx, size_t m, size_t T, void* const* d_frames, const size_t* sizes, const size_t* capacities, const void* const* d_srcs,
		    const size_t* src_sizes, size_t* results, const uint64_t* d_index, hipStream_t stream)
{
	const int level = ctx->level;
	constexpr uint64_t kMaxArray = ((uint64_t)1 << 56) - 1; // the header's size field
	if (batch_shape_refused(ctx, m, T))
		return STENOS_ERROR_INVALID_PARAMETER;
	if (needs_strategy(T, level) || level < 0 || ctx->max_nanoseconds) // what stenos_hip_compress_batch refuses to compress
		return STENOS_ERROR_INVALID_PARAMETER;
	for (size_t f = 0; f < m; ++f)
		if (!d_frames[f] || capacities[f] < sizes[f] || (uint64_t)src_sizes[f] > kMaxArray || (src_sizes[f] && !d_srcs[f]))
			return STENOS_ERROR_INVALID_PARAMETER;
	if (append_batch_overlap(m, d_frames, capacities, d_srcs, src_sizes))
		return STENOS_ERROR_INVALID_PARAMETER;

	// the tables of O(m), mirrored on the host:
	//   BatchTables | [AppendBatchFrame: m][kpre: m + 1][mpre: m + 1][spre: m + 1][dec: m] up | [cpre: 2 m + 1] up |
	//   [FrameJob: 2 m][bpre: 2 m + 1][ipre: 2 m + 1][states: 2 m][tiny list] up, states down | [tiny in] down [tiny out] up |
	//   o_zero: [ends: m][flags: m] down [totals: m][lens: 2 m] down [words: 16 (m + 1)] | o_idx: both indices, device only
	const BatchTables t(m);
	const size_t M2 = 2 * m;
	const size_t o_af = t.o_plan, o_kpre = o_af + align64(m * sizeof(AppendBatchFrame)), o_mpre = o_kpre + align64((m + 1) * 8), o_spre = o_mpre + align64((m + 1) * 8),
		     o_dec = o_spre + align64((m + 1) * 8), o_cpre = o_dec + align64(m * 4), o_jobs = o_cpre + align64((M2 + 1) * 8),
		     o_bpre = o_jobs + align64(M2 * sizeof(codec::FrameJob)), o_ipre = o_bpre + align64((M2 + 1) * 8), o_state = o_ipre + align64((M2 + 1) * 8),
		     o_tiny = o_state + align64(M2 * sizeof(BatchItemState)), o_tin = o_tiny + align64(M2 * 4 + 4), o_tout = o_tin + align64(M2 * sizeof(BatchTinyIn)),
		     o_zero = o_tout + align64(M2 * sizeof(BatchTinyOut)), o_ends = o_zero, o_flags = o_ends + align64(m * 8), o_totals = o_flags + align64(m * 4),
		     o_lens = o_totals + align64(m * 8), o_words = o_lens + align64(M2 * 8), o_idx = o_words + align64((m + 1) * APPEND_WORDS * 4);
	if (!ctx->abtab.ensure(o_idx + 64) || !ctx->h_abtab.ensure(o_idx + 64))
		return STENOS_ERROR_ALLOC;
	uint8_t* const h = ctx->h_abtab.data();
	FrameBatch b{ ctx, m, (const void* const*)d_frames, sizes, stream };
	if (const size_t e = fetch_frames(b, t, T, 1, h, ctx->abtab.as<uint8_t>()))
		return e;
	const uint64_t S = b.S;

	// one geometry: the new superblocks of all frames are encoded in one pass
	const size_t bs = T * 256;
	size_t sb = 0;
	for (size_t f = 0; f < m; ++f) {
		const FrameInfo& fi = b.info[f];
		if (fi.total > kMaxArray - src_sizes[f])
			return STENOS_ERROR_INVALID_PARAMETER;
		if (!fi.total)
			continue;
		if (fi.sb % bs)
			return STENOS_ERROR_INVALID_INPUT;
		if (sb && fi.sb != sb)
			return STENOS_ERROR_INVALID_PARAMETER;
		sb = fi.sb;
	}
	// per frame: keep, r, k, n0; the new numbering; the encoder's items
	struct Item {
		const uint8_t* src; // (a stitched superblock: set once the stitch buffer is there)
		size_t bytes, frame;
		bool stitched, header;
		FramePlan plan;
	};
	std::vector<Item> items;
	AppendBatchFrame* const h_af = (AppendBatchFrame*)(h + o_af);
	uint64_t* const h_kpre = (uint64_t*)(h + o_kpre);
	uint64_t* const h_mpre = (uint64_t*)(h + o_mpre);
	uint64_t* const h_spre = (uint64_t*)(h + o_spre);
	uint32_t* const h_dec = (uint32_t*)(h + o_dec);
	uint64_t first_new = 0, K = 0, moved = 0, stitch_chunks = 0, raw_bytes = 0;
	uint32_t ndec = 0;
	for (size_t f = 0; f < m; ++f) {
		const FrameInfo& fi = b.info[f];
		const size_t nb = src_sizes[f];
		AppendBatchFrame& af = h_af[f];
		memset(&af, 0, sizeof(af));
		af.frame = (uint8_t*)d_frames[f];
		af.size = sizes[f];
		af.src = (const uint8_t*)d_srcs[f];
		af.total = fi.total;
		af.new_bytes = fi.total + nb;
		af.first = b.first[f];
		af.first_new = first_new;
		af.header = (uint32_t)fi.header;
		h_kpre[f] = K;
		h_mpre[f] = moved;
		h_spre[f] = stitch_chunks;
		uint64_t nsb_new = fi.total ? fi.nsb : 0;
		if (!fi.total && nb) {
			// the frame of an empty array carries no geometry: B_f is compressed under the context's settings, with a frame header
			Item it = { (const uint8_t*)d_srcs[f], nb, f, false, true, FramePlan() };
			if (const size_t e = plan_frame(ctx, T, nb, level, it.plan))
				return e;
			if (sb && it.plan.sb != sb)
				return STENOS_ERROR_INVALID_PARAMETER;
			sb = it.plan.sb;
			nsb_new = it.plan.nsb;
			af.k = (uint32_t)nsb_new;
			af.start = (uint32_t)it.plan.header;
			if (nsb_new > 0x7FFFFFFFull)
				return STENOS_ERROR_INVALID_PARAMETER;
			items.push_back(it);
		}
		else if (fi.total) {
			const uint64_t keep = fi.total / sb;
			const size_t r = (size_t)(fi.total % sb);
			nsb_new = af.new_bytes / sb + (af.new_bytes % sb ? 1 : 0);
			if (nsb_new > 0x7FFFFFFFull)
				return STENOS_ERROR_INVALID_PARAMETER;
			af.keep = (uint32_t)keep;
			af.r = (uint32_t)r;
			if (nb) {
				const size_t n0 = r ? (nb < sb - r ? nb : sb - r) : 0;
				af.k = (uint32_t)(nsb_new - keep);
				af.k0 = r ? 1u : 0u;
				af.n0 = (uint32_t)n0;
				FramePlan p;
				p.sb = sb;
				p.shift = 0;
				p.header = 0;
				p.bps = (uint32_t)(sb / bs);
				if (r) {
					af.stitch = raw_bytes;
					raw_bytes += align64(r + n0);
					h_dec[ndec++] = (uint32_t)f;
					stitch_chunks += (n0 + APPEND_COMMIT_CHUNK - 1) / APPEND_COMMIT_CHUNK;
					items.push_back({ nullptr, r + n0, f, true, false, p });
				}
				if (nb > n0)
					items.push_back({ (const uint8_t*)d_srcs[f] + n0, nb - n0, f, false, false, p });
			}
		}
		K += af.k;
		moved += af.k ? af.keep : (fi.total ? fi.nsb + 1 : 0);
		first_new += nsb_new;
	}
	h_kpre[m] = K;
	h_mpre[m] = moved;
	h_spre[m] = stitch_chunks;
	const uint64_t S_new = first_new;
	if (S_new + m > 0x7FFFFFFFull || S + m > 0x7FFFFFFFull) // one thread per entry
		return STENOS_ERROR_INVALID_PARAMETER;
	const size_t n_items = items.size();

	// the encoder's geometry per item, its capacity and place in the encodings
	const uint32_t bps = sb ? (uint32_t)(sb / bs) : 0, stride = stenos_k_slot_stride((uint32_t)T);
	// roomy: every superblock lies in the zone where no capacity rule applies (pipeline.h, safe_superblocks)
	const size_t pad = ((size_t)(bps + 1) * (bs + (T + 1) / 2) + 288 * T + 4096 + 63) & ~(size_t)63;
	std::vector<size_t> cap(n_items, 0);
	std::vector<uint64_t> ebase(n_items, 0);
	std::vector<uint32_t> tiny;
	uint64_t B = 0, K_items = 0, e_all = 0;
	for (size_t i = 0; i < n_items; ++i) {
		Item& it = items[i];
		FramePlan& p = it.plan;
		p.nsb = it.bytes / sb + (it.bytes % sb ? 1 : 0);
		p.nfull = it.bytes / bs;
		p.tail = (uint32_t)(it.bytes % bs);
		cap[i] = (size_t)p.nsb * (sb + 4) + pad + (it.header ? 64 : 0);
		ebase[i] = e_all;
		if (level >= 1 && superblock_bytes(it.bytes, sb, p.nsb - 1) < 128)
			tiny.push_back((uint32_t)i);
		AppendBatchFrame& af = h_af[it.frame];
		const bool first_of_frame = i == 0 || items[i - 1].frame != it.frame;
		if (first_of_frame) {
			af.enc_base0 = af.enc_base1 = e_all;
			af.enc_first = K_items + i;
		}
		else
			af.enc_base1 = e_all;
		B += p.nfull + (p.tail ? 1 : 0);
		K_items += p.nsb;
		e_all += cap[i];
	}
	if (K_items != K)
		return STENOS_ERROR_UNDEFINED;
	if (K * codec::PACK_WAVES >= 0x7FFFFFFFull || B >= 0x7FFFFFFFull) // one workgroup per unit of work
		return STENOS_ERROR_INVALID_PARAMETER;
	const size_t ntiny = tiny.size();
	if (ntiny && !zstd().ok)
		return STENOS_ERROR_ZSTD_INTERNAL;

	ctx->job_kind = 0;
	const size_t o_new = o_idx + align64((S + m) * 8), tab_bytes = o_new + align64((S_new + m) * 8);
	// (growing the buffer loses nothing: the mirror holds the tables, and they go up below)
	if (!ctx->abtab.ensure(tab_bytes))
		return STENOS_ERROR_ALLOC;
	uint8_t* const d = ctx->abtab.as<uint8_t>();
	uint32_t* const d_words = (uint32_t*)(d + o_words);
	uint64_t* const d_idx = (uint64_t*)(d + o_idx);
	uint64_t* const d_new = (uint64_t*)(d + o_new);
	auto fail = [&](size_t code = STENOS_ERROR_UNDEFINED) -> size_t {
		(void)hipStreamSynchronize(stream); // (nothing may still read the page-locked mirror)
		return code;
	};
	for (size_t f = 0; f < m; ++f)
		((uint64_t*)(h + t.o_header))[f] = b.info[f].header;
	if (hipMemsetAsync(d + o_zero, 0, o_idx - o_zero, stream) != hipSuccess)
		return fail();
	if (d_index) {
		if (hipMemcpyAsync(d + t.o_frames, h + t.o_frames, o_cpre - t.o_frames, hipMemcpyHostToDevice, stream) != hipSuccess ||
		    hipMemcpyAsync(d_idx, d_index, (S + m) * 8, hipMemcpyDeviceToDevice, stream) != hipSuccess)
			return fail();
	}
	else if (const size_t e = walk_frames(b, t, d_words + APPEND_W_STATUS, h, d, d_idx, o_cpre))
		return fail(e);
	// the context's index takes the new frames' at the end, and the encoder's offsets in between: if it has to grow, the copy
	// above (whose source it may be) is waited for first
	const size_t index_bytes = (std::max<uint64_t>(S_new + m, K + n_items) + 16) * 8;
	ctx->last_nsb = 0;
	ctx->last_batch = true;
	ctx->last_frames = 0;
	if (index_bytes > ctx->sboff.cap && hipStreamSynchronize(stream) != hipSuccess)
		return STENOS_ERROR_UNDEFINED;
	if (!ctx->sboff.ensure(index_bytes) || !ctx->misc.ensure(4096))
		return fail(STENOS_ERROR_ALLOC);

	AppendBatchArgs a = AppendBatchArgs();
	a.frames = (const AppendBatchFrame*)(d + o_af);
	a.kpre = (const uint64_t*)(d + o_kpre);
	a.mpre = (const uint64_t*)(d + o_mpre);
	a.spre = (const uint64_t*)(d + o_spre);
	a.cpre = (const uint64_t*)(d + o_cpre);
	a.dec = (const uint32_t*)(d + o_dec);
	a.idx = d_idx;
	a.new_idx = d_new;
	a.words = d_words;
	a.flags = (uint32_t*)(d + o_flags);
	a.ends = (uint64_t*)(d + o_ends);
	a.lens = (uint64_t*)(d + o_lens);
	a.totals = (uint64_t*)(d + o_totals);
	a.m = (uint32_t)m;
	a.ndec = ndec;
	a.sb = (uint32_t)sb;
	a.T = (uint32_t)T;
	volatile uint32_t* back = &ctx->h_total->decode_status; // (page-locked)
	const uint64_t* const h_ends = (const uint64_t*)(h + o_ends);
	const uint32_t* const h_flags = (const uint32_t*)(h + o_flags);
	if (stenos_ab_launch_plan(a, stream) != hipSuccess || hipMemcpyAsync((void*)back, d_words, 4, hipMemcpyDeviceToHost, stream) != hipSuccess ||
	    hipMemcpyAsync(h + o_ends, d + o_ends, o_totals - o_ends, hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess)
		return fail();
	ctx->warm = true;
	uint32_t status = back[0];
	if (const size_t e = status_error(status))
		return e;

	const uint64_t* const h_totals = (const uint64_t*)(h + o_totals);
	if (K) {
		if (!ctx->abraw.ensure((size_t)raw_bytes + 64) || !ctx->abenc.ensure((size_t)e_all + 64) || !ctx->slots.ensure((level >= 1 ? B : 0) * stride + 64) ||
		    !ensure_workspace(ctx, B, K, n_items))
			return STENOS_ERROR_ALLOC;
		a.raw = ctx->abraw.as<uint8_t>();
		a.enc = ctx->abenc.as<uint8_t>();
		a.enc_off = ctx->sboff.as<uint64_t>();
		if (stenos_ab_launch_decode(a, stream) != hipSuccess)
			return fail();
		if (status & DECODE_STATUS_HOST_CODES) { // flagged frames: the partial last superblock is decoded on the host, one frame at a time
			if (!zstd().ok)
				return fail(STENOS_ERROR_ZSTD_INTERNAL);
			if (!ctx->rtab.ensure(128) || !ctx->h_rtab.ensure(128))
				return fail(STENOS_ERROR_ALLOC);
			for (uint32_t c = 0; c < ndec; ++c) {
				const size_t f = h_dec[c];
				if (!h_flags[f])
					continue;
				HostCodes hc(ctx, d_frames[f], sizes[f], T, d_idx + b.first[f] + f, b.info[f], stream);
				RangeUnit u;
				u.dst = a.raw + h_af[f].stitch;
				u.sb = h_af[f].keep;
				u.lo = 0;
				u.hi = h_af[f].r;
				u.unused = 0;
				if (size_t err = hc.finish(u))
					return fail(err);
			}
		}
		if (stenos_ab_launch_stitch(a, stitch_chunks, stream) != hipSuccess)
			return fail();

		// the encoder's item tables (compress_batch's, batch_host.cpp)
		codec::FrameJob* const h_jobs = (codec::FrameJob*)(h + o_jobs);
		uint64_t* const h_bpre = (uint64_t*)(h + o_bpre);
		uint64_t* const h_ipre = (uint64_t*)(h + o_ipre);
		BatchItemState* const h_state = (BatchItemState*)(h + o_state);
		const codec::FrameJob* const d_jobs = (const codec::FrameJob*)(d + o_jobs);
		BatchItemState* const d_state = (BatchItemState*)(d + o_state);
		BatchTinyOut* const d_tout = (BatchTinyOut*)(d + o_tout);
		uint64_t b0 = 0, c0 = 0;
		size_t k_tiny = 0;
		for (size_t i = 0; i < n_items; ++i) {
			const Item& it = items[i];
			const FramePlan& p = it.plan;
			h_bpre[i] = b0;
			h_ipre[i] = c0;
			h_state[i] = { 0, 0, 0xFFFFFFFFu };
			codec::FrameJob j;
			if (!frame_job(ctx, p, T, it.bytes, b0, c0, i, j))
				return fail(STENOS_ERROR_ALLOC);
			j.src = it.stitched ? a.raw + h_af[it.frame].stitch : it.src;
			j.dst = ctx->abenc.as<uint8_t>() + ebase[i];
			j.dst_size = cap[i];
			j.slots = ctx->slots.as<uint8_t>() + (level >= 1 ? b0 * stride : 0);
			j.total = &d_state[i].total;
			j.status = &d_state[i].status;
			j.first_flagged = &d_state[i].first_flagged;
			const bool is_tiny = k_tiny < ntiny && tiny[k_tiny] == i;
			j.override_payload = is_tiny ? d_tout[k_tiny].payload : nullptr;
			k_tiny += is_tiny ? 1 : 0;
			j.shift_byte = it.header ? p.shift : 0xFFFFFFFFu; // (0xFFFFFFFF: no frame header)
			j.header_bytes = it.header ? (uint32_t)p.header : 0;
			j.force_copy = level == 0 ? 1u : 0u;
			j.tiny_last = is_tiny ? 1u : 0u;
			j.check_total = 1;
			h_jobs[i] = j;
			b0 += p.nfull + (p.tail ? 1 : 0);
			c0 += p.nsb;
		}
		h_bpre[n_items] = b0;
		h_ipre[n_items] = c0;
		memcpy(h + o_tiny, tiny.data(), ntiny * 4);
		const uint64_t* const d_bpre = (const uint64_t*)(d + o_bpre);
		const uint64_t* const d_ipre = (const uint64_t*)(d + o_ipre);
		const uint32_t* const d_tiny = (const uint32_t*)(d + o_tiny);
		const uint32_t un = (uint32_t)n_items;
		if (hipMemcpyAsync(d + o_jobs, h + o_jobs, o_tin - o_jobs, hipMemcpyHostToDevice, stream) != hipSuccess)
			return fail();
		if ((level >= 1 && stenos_b_launch_encode(d_jobs, d_bpre, un, B, (uint32_t)T, stream) != hipSuccess) || stenos_b_launch_plan(d_jobs, d_ipre, un, K, stream) != hipSuccess ||
		    stenos_b_launch_scan(d_jobs, un, stream) != hipSuccess || stenos_b_launch_resolve(d_jobs, un, (uint32_t)T, stream) != hipSuccess)
			return fail();
		if (ntiny) { // (compress_batch's round trip: zstd is given the room behind the superblock's header, which is ample here)
			BatchTinyIn* const h_tin = (BatchTinyIn*)(h + o_tin);
			BatchTinyOut* const h_tout = (BatchTinyOut*)(h + o_tout);
			if (stenos_b_launch_tiny_gather(d_jobs, d_tiny, (uint32_t)ntiny, (BatchTinyIn*)(d + o_tin), stream) != hipSuccess ||
			    hipMemcpyAsync(h_tin, d + o_tin, ntiny * sizeof(BatchTinyIn), hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess)
				return fail();
			for (size_t k = 0; k < ntiny; ++k) {
				const size_t i = tiny[k];
				const BatchTinyIn& in = h_tin[k];
				BatchTinyOut& out = h_tout[k];
				memset(&out, 0, sizeof(out));
				const size_t last_bytes = superblock_bytes(items[i].bytes, sb, items[i].plan.nsb - 1);
				if (in.status || cap[i] < in.off_last + 4) // (neither happens in a roomy stream; the item then reports an overflow)
					continue;
				const size_t room = cap[i] - (size_t)in.off_last - 4;
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
		if (stenos_b_launch_pack(d_jobs, d_ipre, un, K, bps, stream) != hipSuccess || stenos_ab_launch_commit_plan(a, K, stream) != hipSuccess ||
		    hipMemcpyAsync(h_state, d_state, n_items * sizeof(BatchItemState), hipMemcpyDeviceToHost, stream) != hipSuccess)
			return fail();
	}
	if (stenos_ab_launch_index(a, moved, stream) != hipSuccess)
		return fail();
	if (K) {
		const uint64_t* const h_lens = (const uint64_t*)(h + o_lens);
		const BatchItemState* const h_state = (const BatchItemState*)(h + o_state);
		if (hipMemcpyAsync((void*)back, d_words, 4, hipMemcpyDeviceToHost, stream) != hipSuccess ||
		    hipMemcpyAsync(h + o_totals, d + o_totals, o_words - o_totals, hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess)
			return fail();
		status = back[0];
		if (const size_t e = status_error(status))
			return e;
		for (size_t i = 0; i < n_items; ++i)
			if (h_state[i].status || h_state[i].total > cap[i]) // (the roomy streams cannot overflow)
				return STENOS_ERROR_UNDEFINED;
		// every stream lies inside its item's room, every new frame inside its buffer; then the commit's chunk table
		uint64_t* const h_cpre = (uint64_t*)(h + o_cpre);
		uint64_t chunks = 0;
		size_t i = 0;
		for (size_t f = 0; f < m; ++f) {
			const AppendBatchFrame& af = h_af[f];
			const uint64_t len0 = h_lens[2 * f], len1 = h_lens[2 * f + 1];
			h_cpre[2 * f] = chunks;
			chunks += (len0 + APPEND_COMMIT_CHUNK - 1) / APPEND_COMMIT_CHUNK;
			h_cpre[2 * f + 1] = chunks;
			chunks += (len1 + APPEND_COMMIT_CHUNK - 1) / APPEND_COMMIT_CHUNK;
			if (!af.k) {
				if (len0 || len1)
					return STENOS_ERROR_UNDEFINED;
				continue;
			}
			// (with k0 == 0 the frame's one item is its second stream)
			const size_t room0 = af.k0 ? cap[i] : 0, room1 = af.k > af.k0 ? cap[i + (af.k0 ? 1 : 0)] : 0;
			i += (af.k0 ? 1 : 0) + (af.k > af.k0 ? 1 : 0);
			if (len0 > room0 || len1 > room1 || h_totals[f] < len0 + len1 || h_totals[f] - len0 - len1 > sizes[f])
				return STENOS_ERROR_UNDEFINED;
		}
		h_cpre[M2] = chunks;
		for (size_t f = 0; f < m; ++f)
			if (h_af[f].k && h_totals[f] > capacities[f])
				return STENOS_ERROR_DST_OVERFLOW;
		if (chunks == 0)
			return STENOS_ERROR_UNDEFINED;
		if (hipMemcpyAsync(d + o_cpre, h + o_cpre, (M2 + 1) * 8, hipMemcpyHostToDevice, stream) != hipSuccess || stenos_ab_launch_commit(a, chunks, stream) != hipSuccess)
			return fail();
	}
	if (hipMemcpyAsync(ctx->sboff.p, d_new, (S_new + m) * 8, hipMemcpyDeviceToDevice, stream) != hipSuccess)
		return fail();
	if (hipStreamSynchronize(stream) != hipSuccess)
		return STENOS_ERROR_UNDEFINED;
	for (size_t f = 0; f < m; ++f)
		results[f] = (size_t)(h_af[f].k ? h_totals[f] : h_ends[f]);
	ctx->last_nsb = 0;
	ctx->last_batch = true;
	ctx->last_frames = (size_t)(S_new + m);
	return 0;
}

} // namespace stenos_host
