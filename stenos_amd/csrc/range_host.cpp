// range_host.cpp -- byte ranges of one frame in device memory (stenos_hip_decompress_ranges, range.h).
#include "range_host_codes.h"

namespace stenos_host {

// Every range is cut at the superblock boundaries of the frame; a unit {superblock, lo, hi, dst} is what one wavefront of
// decode_ranges delivers.  The unit table goes up in one copy from the page-locked mirror h_rtab, in front of it the call's
// status word (zero); one word comes back.  Launches and host round trips do not grow with the number of ranges: the header
// fetch, the table, the walk when no index is given, the decode launch, the status (frame_access.h).  The table has a buffer of
// its own (rtab).
// Units in superblocks that went through zstd (codes 2-5) come back flagged and are finished here one by one, which is slow.
size_t decompress_ranges(stenos_context_s* ctx, const void* d_src, size_t T, size_t size, size_t n, const uint64_t* offsets, const uint64_t* lengths,
			 void* const* d_dsts, const uint64_t* d_index, hipStream_t stream)
{
	if (T == 0 || T > STENOS_K_LDS_MAX_T || (ctx->job_kind && ctx->job_async))
		return STENOS_ERROR_INVALID_PARAMETER;
	FrameInfo fi;
	if (const size_t e = fetch_frame_info(d_src, T, size, ~(size_t)0, stream, fi))
		return e;
	uint64_t sum = 0, nunits = 0;
	for (size_t i = 0; i < n; ++i) {
		if (offsets[i] > fi.total || lengths[i] > fi.total - offsets[i]) // (without sums: offset + length may wrap)
			return STENOS_ERROR_INVALID_PARAMETER;
		if (!lengths[i])
			continue;
		if (!d_dsts[i])
			return STENOS_ERROR_INVALID_PARAMETER;
		sum += lengths[i];
		nunits += (offsets[i] + lengths[i] - 1) / fi.sb - offsets[i] / fi.sb + 1;
		if (nunits > 0x7FFFFFFFull) // one workgroup per unit: beyond the grid limit (parse_frame)
			return STENOS_ERROR_INVALID_PARAMETER;
	}
	if (nunits == 0)
		return 0;
	ctx->job_kind = 0;
	const size_t o_units = 64, o_status = o_units + align64(nunits * sizeof(RangeUnit)), o_one = o_status + align64(nunits * 4), tab_bytes = o_one + 128;
	if (!ctx->rtab.ensure(tab_bytes) || !ctx->h_rtab.ensure(tab_bytes))
		return STENOS_ERROR_ALLOC;
	uint8_t* const h = ctx->h_rtab.data();
	uint8_t* const d = ctx->rtab.as<uint8_t>();
	memset(h, 0, o_units);
	RangeUnit* const units = (RangeUnit*)(h + o_units);
	uint64_t k = 0;
	for (size_t i = 0; i < n; ++i) {
		const uint64_t end = offsets[i] + lengths[i];
		for (uint64_t at = offsets[i]; at < end;) {
			const uint64_t s = at / fi.sb, begin = s * fi.sb;
			const uint64_t stop = end - begin < fi.sb ? end : begin + fi.sb;
			RangeUnit& u = units[k++];
			u.dst = (uint8_t*)d_dsts[i] + (at - offsets[i]);
			u.sb = (uint32_t)s;
			u.lo = (uint32_t)(at - begin);
			u.hi = (uint32_t)(stop - begin);
			u.unused = 0;
			at = stop;
		}
	}
	auto fail = [&](size_t code = STENOS_ERROR_UNDEFINED) -> size_t {
		(void)hipStreamSynchronize(stream);
		return code;
	};
	uint32_t* const d_status = (uint32_t*)d;
	if (hipMemcpyAsync(d, h, o_status, hipMemcpyHostToDevice, stream) != hipSuccess)
		return fail();
	if (const size_t e = frame_offsets(ctx, d_src, size, fi, &d_index, nullptr, d_status, stream))
		return fail(e);
	RangeArgs a = RangeArgs();
	a.frame = (const uint8_t*)d_src;
	a.size = size;
	a.sb_off = d_index;
	a.units = (const RangeUnit*)(d + o_units);
	a.unit_status = (uint32_t*)(d + o_status);
	a.status = d_status;
	a.total_bytes = fi.total;
	a.sb_bytes = (uint32_t)fi.sb;
	a.T = (uint32_t)T;
	a.nunits = (uint32_t)nunits;
	volatile uint32_t* back = &ctx->h_total->decode_status; // (page-locked)
	if (stenos_r_launch_decode(a, stream) != hipSuccess || hipMemcpyAsync((void*)back, d_status, 4, hipMemcpyDeviceToHost, stream) != hipSuccess ||
	    hipStreamSynchronize(stream) != hipSuccess)
		return fail();
	ctx->warm = true;
	const uint32_t status = *back;
	if (const size_t e = status_error(status))
		return e;
	if (status & DECODE_STATUS_HOST_CODES) {
		if (!zstd().ok)
			return STENOS_ERROR_ZSTD_INTERNAL;
		uint32_t* const h_status = (uint32_t*)(h + o_status);
		if (hipMemcpyAsync(h_status, d + o_status, nunits * 4, hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess)
			return fail();
		HostCodes hc(ctx, d_src, size, T, d_index, fi, stream, o_one);
		for (uint64_t u = 0; u < nunits; ++u)
			if (h_status[u] & DECODE_STATUS_HOST_CODES)
				if (size_t err = hc.finish(units[u]))
					return err;
	}
	return (size_t)sum;
}

} // namespace stenos_host
