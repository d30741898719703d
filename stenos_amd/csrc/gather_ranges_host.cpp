// gather_ranges_host.cpp -- variable-length ranges of one frame in device memory by offsets and lengths that live on the device
// (stenos_hip_gather_ranges, gather_ranges.h).
#include "gather_ranges.h"
#include "range_host_codes.h"

namespace stenos_host {

// All of the call is enqueued on `stream` -- the header fetch, one memset (the call's words, counts, flags), the walk when no
// index is given, ranges_sums, ranges_scan, ranges_apply, ranges_count, gather_scan, ranges_fill, gather_decode, the words back
// (status, D[n]) -- so launches and host round trips grow neither with n, nor with the lengths, nor with the frame.  The host
// knows n and dst_size and sizes every table and grid by the piece bound that follows from them (gather_ranges_codec.h).  The
// tables lie in a buffer of the call's own, grtab:
//   [the PiecePlan of frame_access.h for pmax pieces][D: n + 1, where the caller gives no d_dst_offsets][pstart: n + 1][block sums:
//   8 + 4 bytes per 256 ranges]
// the plan's part zero on entry up to its o_ppre.  Pieces in superblocks that went through zstd (codes 2-5) are rebuilt here from the offsets and
// lengths, with the kernels' own measuring and cutting functions, and finished one by one (range_host_codes.h, HostCodes), which
// is slow.
size_t gather_ranges(stenos_context_s* ctx, const void* d_src, size_t T, size_t size, size_t n, const uint64_t* d_offsets, const uint64_t* d_lengths, void* d_dst,
		     size_t dst_size, uint64_t* d_dst_offsets, const uint64_t* d_index, hipStream_t stream)
{
	if (T == 0 || T > STENOS_K_LDS_MAX_T || (ctx->job_kind && ctx->job_async))
		return STENOS_ERROR_INVALID_PARAMETER;
	FrameInfo fi;
	if (const size_t e = fetch_frame_info(d_src, T, size, ~(size_t)0, stream, fi))
		return e;
	// The frame of an empty array has no superblock and so no piece, whatever dst_size is: no piece slots, no slot kernels, no
	// decode grid (only ranges of length 0 at offset 0 are valid in it; sb = 1 there is only what the measuring divides by).
	const uint64_t sb = fi.total ? fi.sb : 1;
	const uint64_t pmax = fi.total ? codec::ranges_piece_bound(n, dst_size, sb) : 0, waves = stenos_g_decode_waves(fi.nsb, pmax);
	PiecePlan plan;
	if ((fi.total && pmax == 0) || !plan.init(fi.nsb, 1, pmax) || waves > 0x7FFFFFFFull) // one thread per piece slot, one workgroup per wavefront: beyond the grid limit (parse_frame)
		return STENOS_ERROR_INVALID_PARAMETER;
	const uint64_t nblocks = stenos_gr_blocks(n);
	const size_t o_D = plan.end, o_pstart = o_D + (d_dst_offsets ? 0 : align64((n + 1) * 8)), o_bbytes = o_pstart + align64((n + 1) * 4),
		     o_bpieces = o_bbytes + align64(nblocks * 8), end = o_bpieces + align64(nblocks * 4);
	ctx->job_kind = 0;
	if (!ctx->grtab.ensure(end) || !ctx->h_grtab.ensure(64))
		return STENOS_ERROR_ALLOC;
	uint8_t* const d = ctx->grtab.as<uint8_t>();
	codec::RangesWords* const d_words = (codec::RangesWords*)d;
	uint32_t* const d_status = &d_words->status;
	auto fail = [&](size_t code = STENOS_ERROR_UNDEFINED) -> size_t {
		(void)hipStreamSynchronize(stream);
		return code;
	};
	if (hipMemsetAsync(d, 0, plan.o_ppre, stream) != hipSuccess)
		return fail();
	if (fi.nsb)
		if (const size_t e = frame_offsets(ctx, d_src, size, fi, &d_index, nullptr, d_status, stream))
			return fail(e);
	// what gather_scan and gather_decode read: the tables of the plan (one piece per "row": the slots), the frame, dst and waves
	GatherArgs a = plan.args(d, d_src, size, d_index, fi, T, 1, 0, nullptr, 1, d_status);
	a.dst = (uint8_t*)d_dst;
	a.waves = (uint32_t)waves;
	codec::RangesArgs r = codec::RangesArgs();
	r.offsets = d_offsets;
	r.lengths = d_lengths;
	r.n = n;
	r.total = fi.total;
	r.sb = sb;
	r.dst_size = dst_size;
	r.pmax = pmax;
	r.nblocks = (uint32_t)nblocks;
	r.words = d_words;
	r.D = d_dst_offsets ? d_dst_offsets : (uint64_t*)(d + o_D);
	r.pstart = (uint32_t*)(d + o_pstart);
	r.block_bytes = (uint64_t*)(d + o_bbytes);
	r.block_pieces = (uint32_t*)(d + o_bpieces);
	r.count = a.count;
	r.ppre = a.ppre;
	r.pieces = a.pieces;
	volatile codec::RangesWords* back = (volatile codec::RangesWords*)ctx->h_grtab.data(); // (page-locked)
	if (stenos_gr_launch_offsets(r, stream) != hipSuccess || stenos_gr_launch_count(r, stream) != hipSuccess || stenos_g_launch_scan(a, stream) != hipSuccess ||
	    stenos_gr_launch_fill(r, stream) != hipSuccess || stenos_g_launch_decode(a, stream) != hipSuccess ||
	    hipMemcpyAsync((void*)back, d_words, sizeof(codec::RangesWords), hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess)
		return fail();
	ctx->warm = true;
	const uint32_t status = back->status;
	const uint64_t delivered = back->total;
	if (const size_t e = status_error(status)) // (an invalid range, then the overflow, in front of any decode error)
		return e;
	if (status & DECODE_STATUS_HOST_CODES) {
		if (!zstd().ok)
			return STENOS_ERROR_ZSTD_INTERNAL;
		const size_t o_hoff = 64, o_hlen = o_hoff + align64(n * 8), o_hflags = o_hlen + align64(n * 8);
		if (!ctx->h_grtab.ensure(o_hflags + fi.nsb * 4) || !ctx->rtab.ensure(128) || !ctx->h_rtab.ensure(128))
			return STENOS_ERROR_ALLOC;
		uint8_t* const h = ctx->h_grtab.data();
		const uint64_t* const h_off = (const uint64_t*)(h + o_hoff);
		const uint64_t* const h_len = (const uint64_t*)(h + o_hlen);
		const uint32_t* const h_flags = (const uint32_t*)(h + o_hflags);
		if (hipMemcpyAsync(h + o_hoff, d_offsets, n * 8, hipMemcpyDeviceToHost, stream) != hipSuccess ||
		    hipMemcpyAsync(h + o_hlen, d_lengths, n * 8, hipMemcpyDeviceToHost, stream) != hipSuccess ||
		    hipMemcpyAsync(h + o_hflags, a.sb_flags, fi.nsb * 4, hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess)
			return fail();
		std::vector<RangeUnit> units;
		uint64_t at = 0; // D[i], formed again here
		for (uint64_t i = 0; i < n; ++i) {
			uint64_t bytes;
			uint32_t pieces;
			if (!codec::ranges_measure(fi.total, sb, h_off[i], h_len[i], &bytes, &pieces)) // (the device has let every range pass)
				return STENOS_ERROR_INVALID_PARAMETER;
			for (uint32_t j = 0; j < pieces; ++j) {
				uint64_t s;
				codec::GatherPiece p;
				codec::ranges_cut(sb, h_off[i], h_len[i], at, j, &s, &p);
				if (!h_flags[s])
					continue;
				RangeUnit u;
				u.dst = (uint8_t*)d_dst + p.dst;
				u.sb = (uint32_t)s;
				u.lo = p.lo;
				u.hi = p.hi;
				u.unused = 0;
				units.push_back(u);
			}
			at += bytes;
		}
		std::stable_sort(units.begin(), units.end(), [](const RangeUnit& x, const RangeUnit& y) { return x.sb < y.sb; });
		HostCodes hc(ctx, d_src, size, T, d_index, fi, stream);
		for (const RangeUnit& u : units)
			if (const size_t err = hc.finish(u))
				return err;
	}
	return (size_t)delivered;
}

} // namespace stenos_host
