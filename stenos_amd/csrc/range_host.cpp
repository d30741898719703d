// range_host.cpp -- byte ranges of one frame in device memory (stenos_hip_decompress_ranges, range.h).
#include "host.h"
#include "range.h"

namespace stenos_host {

// Every range is cut at the superblock boundaries of the frame; a unit {superblock, lo, hi, dst} is what one wavefront of
// decode_ranges delivers.  The unit table goes up in one copy from the page-locked mirror h_rtab, in front of it the call's
// status word (zero); one word comes back.  Launches and host round trips do not grow with the number of ranges: the header
// fetch, the walk when no index is given, the table, the decode launch, the status.  The table has a buffer of its own
// (rtab): an index the caller passes may be the context's own (sboff) and stays as it is.
// Units in superblocks that went through zstd (codes 2-5) come back flagged and are finished here one by one, which is slow.
namespace {

inline size_t align64(size_t v) { return (v + 63) & ~(size_t)63; }

struct HostCodes {
	stenos_context_s* ctx;
	const uint8_t* d_frame;
	size_t size, T;
	const uint64_t* d_index;
	FrameInfo fi;
	hipStream_t stream;
	uint8_t* h_tab; // mirror of rtab
	uint8_t* d_tab;
	size_t o_one;   // the words and the unit of a one-unit launch (code 5), in both
	// the superblock the buffers hold: inflated bytes at h_stage + 16 (codes 2 and 5), decoded bytes in rsb (codes 3 and 4)
	uint64_t have_sb = ~0ull;
	unsigned have_code = 0;
	size_t have_bytes = 0;

	bool copy(void* to, const void* from, size_t n, hipMemcpyKind kind) const
	{
		return hipMemcpyAsync(to, from, n, kind, stream) == hipSuccess && hipStreamSynchronize(stream) == hipSuccess;
	}
	// fetch and inflate superblock s; 0 or an error code
	size_t load(uint64_t s)
	{
		if (s == have_sb)
			return 0;
		have_sb = ~0ull;
		const size_t dsize = superblock_bytes(fi.total, fi.sb, s);
		uint64_t p = 0;
		uint8_t hd[4];
		if (!copy(&p, d_index + s, 8, hipMemcpyDeviceToHost))
			return STENOS_ERROR_UNDEFINED;
		if (p > size || size - p < 4)
			return STENOS_ERROR_SRC_OVERFLOW;
		if (!copy(hd, d_frame + p, 4, hipMemcpyDeviceToHost))
			return STENOS_ERROR_UNDEFINED;
		const unsigned code = hd[0];
		const size_t csize = (size_t)get_le(hd + 1, 3);
		if (code < 2 || code > 5 || size - p - 4 < csize)
			return STENOS_ERROR_INVALID_INPUT;
		if (!ctx->h_in.ensure(csize + 64) || !ctx->h_stage.ensure(fi.sb + 64 + 32) || !ctx->tmp1.ensure(fi.sb + 64 + 32) || !ctx->tmp2.ensure(fi.sb + 64) ||
		    !ctx->rsb.ensure(fi.sb + 64))
			return STENOS_ERROR_ALLOC;
		if (csize && !copy(ctx->h_in.data(), d_frame + p + 4, csize, hipMemcpyDeviceToHost))
			return STENOS_ERROR_UNDEFINED;
		uint8_t* const hs = ctx->h_stage.data();
		// code 5: zstd over the block stream, at most the superblock size (stenos.cpp:732)
		const size_t r = zstd().decompress(hs + 16, code == 5 ? fi.sb + 64 : dsize, ctx->h_in.data(), csize);
		if (zstd().is_error(r) || (code != 5 && code != 2 && r != dsize)) // stenos.cpp:696-698, 706-708, 718-720
			return STENOS_ERROR_INVALID_INPUT;
		if (code == 3 || code == 4) { // transposed (stenos.cpp:700-710) / transposed + byte delta (:711-725) -> rsb
			uint8_t* const t1 = ctx->tmp1.as<uint8_t>();
			uint8_t* const t2 = ctx->tmp2.as<uint8_t>();
			bool ok = hipMemcpyAsync(t1, hs + 16, dsize, hipMemcpyHostToDevice, stream) == hipSuccess;
			if (code == 4)
				ok = ok && stenos_k_launch_delta(t1, t2, dsize, true, stream) == hipSuccess;
			ok = ok && stenos_k_launch_shuffle(code == 4 ? t2 : t1, ctx->rsb.as<uint8_t>(), (uint32_t)T, dsize, true, stream) == hipSuccess;
			if (!ok || hipStreamSynchronize(stream) != hipSuccess)
				return STENOS_ERROR_UNDEFINED;
		}
		else if (code == 5) { // -> one BLOCK superblock for the block decoder (stenos.cpp:726-740), its payload 16-byte aligned
			write_superblock_header(hs + 12, 1, r);
			if (!copy(ctx->tmp1.as<uint8_t>() + 12, hs + 12, 4 + r, hipMemcpyHostToDevice))
				return STENOS_ERROR_UNDEFINED;
		}
		have_sb = s;
		have_code = code;
		have_bytes = r;
		return 0;
	}
	size_t finish(const RangeUnit& u)
	{
		if (size_t e = load(u.sb))
			return e;
		const size_t len = u.hi - u.lo;
		if (have_code == 2) { // plain zstd
			if (u.hi > have_bytes)
				return STENOS_ERROR_INVALID_INPUT;
			return copy(u.dst, ctx->h_stage.data() + 16 + u.lo, len, hipMemcpyHostToDevice) ? 0 : (size_t)STENOS_ERROR_UNDEFINED;
		}
		if (have_code != 5)
			return copy(u.dst, ctx->rsb.as<uint8_t>() + u.lo, len, hipMemcpyDeviceToDevice) ? 0 : (size_t)STENOS_ERROR_UNDEFINED;
		uint8_t* const h = h_tab + o_one;
		uint8_t* const d = d_tab + o_one;
		memset(h, 0, 128);
		*(RangeUnit*)(h + 64) = u;
		RangeArgs a = RangeArgs();
		a.frame = ctx->tmp1.as<uint8_t>();
		a.size = 16 + have_bytes;
		a.sb_off = nullptr;
		a.direct_off = 12;
		a.units = (const RangeUnit*)(d + 64);
		a.unit_status = (uint32_t*)(d + 8);
		a.status = (uint32_t*)d;
		a.total_bytes = fi.total;
		a.sb_bytes = (uint32_t)fi.sb;
		a.T = (uint32_t)T;
		a.nunits = 1;
		volatile uint32_t* back = &ctx->h_total->decode_status;
		if (hipMemcpyAsync(d, h, 128, hipMemcpyHostToDevice, stream) != hipSuccess || stenos_r_launch_decode(a, stream) != hipSuccess ||
		    !copy((void*)back, d, 4, hipMemcpyDeviceToHost))
			return STENOS_ERROR_UNDEFINED;
		return *back ? (size_t)STENOS_ERROR_INVALID_INPUT : 0;
	}
};

} // namespace

size_t decompress_ranges(stenos_context_s* ctx, const void* d_src, size_t T, size_t size, size_t n, const uint64_t* offsets, const uint64_t* lengths,
			 void* const* d_dsts, const uint64_t* d_index, hipStream_t stream)
{
	if (T == 0 || T > STENOS_K_LDS_MAX_T || (ctx->job_kind && ctx->job_async))
		return STENOS_ERROR_INVALID_PARAMETER;
	uint8_t head[12] = { 0 };
	const size_t have = size < 12 ? size : 12;
	if (have && (hipMemcpyAsync(head, d_src, have, hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess))
		return STENOS_ERROR_UNDEFINED;
	FrameInfo fi;
	const size_t e = parse_frame(head, have, T, ~(size_t)0, fi);
	if (is_err(e))
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
	auto fail = [&]() -> size_t {
		(void)hipStreamSynchronize(stream);
		return STENOS_ERROR_UNDEFINED;
	};
	uint32_t* const d_status = (uint32_t*)d;
	if (hipMemcpyAsync(d, h, o_status, hipMemcpyHostToDevice, stream) != hipSuccess)
		return fail();
	if (!d_index) { // the chain is walked first, into the context's index
		if (!ctx->sboff.ensure((fi.nsb + 2) * 8) || !ctx->walk.ensure(stenos_k_walk_scratch_bytes()))
			return (void)hipStreamSynchronize(stream), STENOS_ERROR_ALLOC;
		d_index = ctx->sboff.as<uint64_t>();
		if (stenos_k_launch_walk((const uint8_t*)d_src, size, fi.header, fi.nsb, (uint32_t)fi.sb, ctx->sboff.as<uint64_t>(), d_status,
					 ctx->test_serial_walk ? nullptr : ctx->walk.p, stream) != hipSuccess)
			return fail();
	}
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
	if (status & DECODE_STATUS_TRUNCATED)
		return STENOS_ERROR_SRC_OVERFLOW;
	if (status & DECODE_STATUS_INVALID)
		return STENOS_ERROR_INVALID_INPUT;
	if (status & DECODE_STATUS_HOST_CODES) {
		if (!zstd().ok)
			return STENOS_ERROR_ZSTD_INTERNAL;
		uint32_t* const h_status = (uint32_t*)(h + o_status);
		if (hipMemcpyAsync(h_status, d + o_status, nunits * 4, hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess)
			return fail();
		HostCodes hc;
		hc.ctx = ctx;
		hc.d_frame = (const uint8_t*)d_src;
		hc.size = size;
		hc.T = T;
		hc.d_index = d_index;
		hc.fi = fi;
		hc.stream = stream;
		hc.h_tab = h;
		hc.d_tab = d;
		hc.o_one = o_one;
		for (uint64_t u = 0; u < nunits; ++u)
			if (h_status[u] & DECODE_STATUS_HOST_CODES)
				if (size_t err = hc.finish(units[u]))
					return err;
	}
	return (size_t)sum;
}

} // namespace stenos_host
