// strategy_host.cpp -- levels >= 2 and bytesoftype 1: the host side strategy layer around the GPU passes (the estimator
// itself is strategy.cpp).
#include "host.h"

namespace stenos_host {

// zstd_from_reduced_level (zstd_wrapper.h:49-56)
static int zstd_level_of(int clevel)
{
	if (clevel < 1)
		return 1;
	if (clevel < 9)
		return clevel * 2 - 1;
	return zstd().max_level();
}

// Levels >= 2 and bytesoftype 1: the strategy layer of compress_generic_superblock (stenos.cpp:451-604, 617-678).
// The GPU encodes every superblock with the block codec (capacity = the superblock's own size, as the reference's
// scratch buffer), shuffles the input and prepares the plane middles for the LZ4-dry estimates; the host runs
// the estimator and zstd (third-party entropy coder) and assembles the frame in `h_dst` with the reference's
// serial capacity semantics.  h_src / d_src: host and device copies of the input.
// d_dst (device destinations): the frame is uploaded batch by batch while the next batch is in zstd; h_dst is the staging.
size_t compress_strategy(stenos_context_s* ctx, const uint8_t* h_src, const uint8_t* d_src, size_t T, size_t bytes, uint8_t* h_dst, size_t dst_size,
			 int level, const FramePlan& f, hipStream_t stream, uint8_t* d_dst)
{
	if (!zstd().ok)
		return STENOS_ERROR_ZSTD_INTERNAL;
	if (dst_size < f.header)
		return STENOS_ERROR_DST_OVERFLOW;
	write_frame_header(h_dst, f.shift, bytes, f.sb);
	const uint64_t nblocks = f.nfull + (f.tail ? 1 : 0);
	const uint32_t stride = stenos_k_slot_stride((uint32_t)T);
	const size_t tmp_cap = bytes + 4 * (size_t)f.nsb + 64;
	if (!ensure_workspace(ctx, nblocks, f.nsb, 1) || !ctx->qprod.ensure((f.nsb + 1) * 4) || !ctx->slots.ensure((nblocks + 1) * (size_t)stride) ||
	    !ctx->tmp1.ensure(tmp_cap))
		return STENOS_ERROR_ALLOC;
	DeviceWords* w = ctx->words();
	codec::FrameJob j;
	if (!frame_job(ctx, f, T, bytes, 0, 0, 0, j))
		return STENOS_ERROR_ALLOC;
	j.src = d_src;
	j.dst = ctx->tmp1.as<uint8_t>();
	j.dst_size = ~(uint64_t)0 >> 1;
	j.shift_byte = 0xFFFFFFFFu;
	j.fixed_capacity = 1;
	j.qprod = ctx->qprod.as<uint32_t>();
	uint64_t* d_carry = &w->scan_carry;
	// The block codec's verdict per superblock first (sizes only: nothing is packed or moved yet) ...
	if (stenos_k_launch_init((uint8_t*)w, 0, nullptr, 0, nullptr, 0, stream) != hipSuccess || stenos_k_launch_encode(j, 0, nblocks, stream) != hipSuccess || stenos_k_launch_plan(j, 0, f.nsb, stream) != hipSuccess)
		return STENOS_ERROR_UNDEFINED;
	std::vector<uint8_t> code(f.nsb);
	std::vector<uint32_t> csize(f.nsb), qprod(f.nsb);
	std::vector<uint64_t> sboff(f.nsb + 1);
	if (hipMemcpyAsync(code.data(), j.sb_code, f.nsb, hipMemcpyDeviceToHost, stream) != hipSuccess ||
	    hipMemcpyAsync(csize.data(), j.sb_csize, f.nsb * 4, hipMemcpyDeviceToHost, stream) != hipSuccess ||
	    hipMemcpyAsync(qprod.data(), j.qprod, f.nsb * 4, hipMemcpyDeviceToHost, stream) != hipSuccess)
		return STENOS_ERROR_UNDEFINED;
	PhaseTrace trace(ctx->stage_ms);
	// ... and, for an input that lives on the device (h_src == NULL), the part of it the estimator looks at: the first
	// 1/16 of every superblock (stenos.cpp:497-499), one strided copy into a host image of the input.  The rest of a
	// superblock is fetched only if it ends up going through zstd as it is (or as a copy).
	const bool lazy_src = h_src == nullptr;
	if (lazy_src) {
		if (!ctx->h_in.ensure(bytes + 64))
			return STENOS_ERROR_ALLOC;
		uint8_t* img = ctx->h_in.data();
		const uint64_t whole = bytes / f.sb;
		if (whole && f.sb / 16 &&
		    hipMemcpy2DAsync(img, f.sb, d_src, f.sb, f.sb / 16, (size_t)whole, hipMemcpyDeviceToHost, stream) != hipSuccess)
			return STENOS_ERROR_UNDEFINED;
		if (bytes > whole * f.sb && hipMemcpyAsync(img + whole * f.sb, d_src + whole * f.sb, bytes - whole * f.sb, hipMemcpyDeviceToHost, stream) != hipSuccess)
			return STENOS_ERROR_UNDEFINED; // (the last, partial superblock: all of it)
		h_src = img;
	}
	if (hipStreamSynchronize(stream) != hipSuccess)
		return STENOS_ERROR_UNDEFINED;
	trace.mark("verdicts and samples to host", STAGE_GPU_PASS);
	HostBuf& blocks = ctx->h_blocks;
	// transposed views for the estimator and the transposed zstd strategies (levels > 2 only, stenos.cpp:515-537)
	const bool transposed = T > 1 && level > 2;
	HostBuf &shuf = ctx->h_shuf, &mid0 = ctx->h_mid0, &mid1 = ctx->h_mid1;
	if (transposed) {
		if (!ctx->shuf.ensure(bytes + 64) || !ctx->mid0.ensure(bytes + 64) || !ctx->mid1.ensure(bytes + 64))
			return STENOS_ERROR_ALLOC;
		if (stenos_k_launch_shuffle_superblocks(d_src, ctx->shuf.as<uint8_t>(), (uint32_t)T, f.sb, bytes, stream) != hipSuccess ||
		    stenos_k_launch_delta_middles(ctx->shuf.as<uint8_t>(), ctx->mid0.as<uint8_t>(), (uint32_t)T, f.sb, bytes, (uint32_t)level, false, stream) != hipSuccess ||
		    stenos_k_launch_delta_middles(ctx->shuf.as<uint8_t>(), ctx->mid1.as<uint8_t>(), (uint32_t)T, f.sb, bytes, (uint32_t)level, true, stream) != hipSuccess)
			return STENOS_ERROR_UNDEFINED;
		if (!shuf.ensure(bytes + 64) || !mid0.ensure(bytes + 64) || !mid1.ensure(bytes + 64))
			return STENOS_ERROR_ALLOC;
		if (hipMemcpy(shuf.data(), ctx->shuf.p, bytes, hipMemcpyDeviceToHost) != hipSuccess ||
		    hipMemcpy(mid0.data(), ctx->mid0.p, bytes, hipMemcpyDeviceToHost) != hipSuccess ||
		    hipMemcpy(mid1.data(), ctx->mid1.p, bytes, hipMemcpyDeviceToHost) != hipSuccess)
			return STENOS_ERROR_UNDEFINED;
		trace.mark("transposed views to host", STAGE_GPU_PASS);
	}

	int zstd_level = level; // stenos.cpp:441-460
	if (T > 1) {
		zstd_level = level - 1;
		if (zstd_level >= 4)
			++zstd_level;
	}
	const int zl = zstd_level_of(zstd_level);
	const size_t bs = 256 * T;
	// What a superblock becomes is decided first (it does not depend on the room left in the destination):
	//   0 = tiny input, plain zstd level 1 (stenos.cpp:435-437)      1 = block codec + zstd (code 5, or 1)
	//   2/3/4 = zstd over the raw / transposed / transposed+delta bytes (stenos.cpp:548-558)
	auto decide = [&](uint64_t s) -> int {
		const uint8_t* src = h_src + s * f.sb;
		const size_t sbytes = superblock_bytes(bytes, f.sb, s);
		if (sbytes < 128)
			return 0;
		double lz_ratio = 1.1, lz_tr = 0, lz_trd = 0;
		if (sbytes >= bs)
			lz_ratio = (double)(sbytes / 16) / (double)strategy::lz4_dry_size(src, sbytes / 16, 10 - level);
		if (T > 1) {
			if (transposed && sbytes >= bs) {
				const size_t step = strategy::middle_step(T, sbytes, level);
				lz_tr = strategy::transposed_ratio(mid0.data() + s * f.sb, T, step, level);
				if (lz_tr > lz_ratio)
					lz_ratio = lz_tr;
				lz_trd = strategy::transposed_ratio(mid1.data() + s * f.sb, T, step, level) * 1.1;
				if (lz_trd > lz_ratio)
					lz_ratio = lz_trd;
				const double factor = 1. + level / 12.;
				lz_tr *= factor;
				lz_trd *= factor;
				lz_ratio *= factor;
			}
		}
		else
			lz_ratio *= 1. + level / 12.;
		// block codec result of the GPU; the reference gives up when, after 1/16 of the input, the running
		// ratio is below the estimate (block_compress.h:1266-1274)
		bool ok = code[s] == 1;
		if (ok && qprod[s]) {
			size_t bq = (sbytes / 16 + bs - 1) / bs;
			bq = bq == 0 ? 0 : bq - 1;
			const double ratio = (double)((bq + 1) * bs) / (double)qprod[s];
			if (ratio < lz_ratio)
				ok = false;
		}
		if (ok)
			return 1;
		int c = 2; // stenos.cpp:548-558
		if (lz_ratio > 1.40) {
			if (lz_ratio == lz_tr)
				c = 3;
			else if (lz_ratio == lz_trd)
				c = 4;
		}
		return c;
	};

	// One superblock -> [code][csize:3][payload] at `out` with `room` bytes of capacity (what the reference
	// hands to its strategies, stenos.cpp:895).  `delta_src`: the GPU's byte delta of the transposed
	// superblock for choice 4.  Returns the bytes written or an error code.
	auto emit = [&](uint64_t s, int choice, const uint8_t* delta_src, uint8_t* out, size_t room) -> size_t {
		const uint8_t* src = h_src + s * f.sb;
		const size_t sbytes = superblock_bytes(bytes, f.sb, s);
		if (choice == 0) { // (the capacity zstd sees is the room itself, as in the reference's serial loop)
			uint32_t tiny_size = 0;
			const uint32_t tiny_code = tiny_superblock(src, sbytes, room - 4, out + 4, room - 4, &tiny_size);
			if (!tiny_code)
				return (size_t)STENOS_ERROR_DST_OVERFLOW;
			write_superblock_header(out, tiny_code, tiny_size);
			return (size_t)tiny_size + 4;
		}
		size_t r;
		if (choice == 1) {
			const uint8_t* payload = blocks.data() + sboff[s] + 4;
			const size_t cblock = csize[s];
			r = zstd().compress(out + 4, room - 4, payload, cblock, zl); // stenos.cpp:583
			if (zstd().is_error(r) || r > cblock) {                     // NO_ZSTD (:585-596)
				if (room < 4 + cblock)
					return (size_t)STENOS_ERROR_DST_OVERFLOW;
				write_superblock_header(out, 1, cblock);
				memcpy(out + 4, payload, cblock);
				return cblock + 4;
			}
			write_superblock_header(out, 5, r);
			return r + 4;
		}
		const uint8_t* zsrc = choice == 3 ? shuf.data() + s * f.sb : choice == 4 ? delta_src : src;
		r = zstd().compress(out + 4, room - 4, zsrc, sbytes, zl);
		if (zstd().is_error(r) || r > sbytes)
			return room < sbytes + 4 ? (size_t)STENOS_ERROR_DST_OVERFLOW : copy_superblock(out, src, sbytes);
		write_superblock_header(out, (uint32_t)choice, r);
		return r + 4;
	};

	// What every superblock becomes, then only the block streams that are kept are packed and brought to the host: the
	// reference abandons the block codec for a superblock after 1/16 of it when the ratio target fails
	// (block_compress.h:1266-1274) -- here the verdict comes from the sizes, and an abandoned superblock costs neither a
	// pack nor a transfer.
	std::vector<int> all_choice(f.nsb);
	parallel_for(f.nsb, [&](uint64_t s) { all_choice[s] = decide(s); });
	trace.mark("estimates", STAGE_ESTIMATES);
	{
		std::vector<uint8_t> keep(f.nsb);
		uint64_t dropped = 0;
		for (uint64_t s = 0; s < f.nsb; ++s) {
			keep[s] = all_choice[s] == 1;
			dropped += code[s] == 1 && !keep[s];
		}
		if (dropped) {
			if (!ctx->tmp2.ensure(f.nsb + 64) || hipMemcpyAsync(ctx->tmp2.p, keep.data(), f.nsb, hipMemcpyHostToDevice, stream) != hipSuccess ||
			    stenos_k_launch_keep_superblocks(ctx->tmp2.as<uint8_t>(), j.sb_code, j.sb_csize, f.nsb, stream) != hipSuccess)
				return STENOS_ERROR_UNDEFINED;
		}
		if (stenos_k_launch_scan(j, 0, f.nsb, d_carry, stream) != hipSuccess || stenos_k_launch_pack(j, 0, f.nsb, stream) != hipSuccess ||
		    hipMemcpyAsync(sboff.data(), j.sb_off, (f.nsb + 1) * 8, hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess)
			return STENOS_ERROR_UNDEFINED;
		const size_t blocks_size = (size_t)sboff[f.nsb];
		if (!blocks.ensure(blocks_size + 64))
			return STENOS_ERROR_ALLOC;
		trace.mark("pack", STAGE_GPU_PASS);
	}
	// The block streams come to the host batch by batch on a stream of their own, in the order the batches are compressed:
	// the transfer of batch k + 1 runs while batch k is in zstd (the link moves 50 GB/s, sixteen cores' zstd a quarter of
	// that), and so does the upload of the finished part of the frame when the destination is device memory.
	const size_t ample = (4 + f.sb + f.sb / 128 + 1024 + 15) & ~(size_t)15; // (a multiple of 16: the gather kernel reads the slots with aligned 16-byte loads)
	uint64_t batch = ((size_t)256 << 20) / f.sb;
	batch = batch < 64 ? 64 : batch > 1024 ? 1024 : batch;
	const uint64_t nbatch = (f.nsb + batch - 1) / batch;
	if (!ctx->ensure_stream(&ctx->copy_stream) || (d_dst && !ctx->ensure_stream(&ctx->upload_stream)))
		return STENOS_ERROR_ALLOC;
	hipStream_t copy = ctx->copy_stream;                          // device -> host: block streams, in batch order
	hipStream_t up = d_dst ? ctx->upload_stream : ctx->copy_stream; // host -> device: the frame (not queued behind the downloads)
	struct Drain { // (whatever way this function is left, no transfer of this call is still in flight)
		hipStream_t a, b;
		~Drain()
		{
			(void)hipStreamSynchronize(a);
			(void)hipStreamSynchronize(b);
		}
	} drain = { copy, up };
	if (!ctx->ensure_events(ctx->batch_ev, nbatch))
		return STENOS_ERROR_ALLOC;
	{
		if (lazy_src) { // raw bytes of the superblocks that go through zstd as they are (runs of neighbours in one copy), first
			uint8_t* img = ctx->h_in.data();
			for (uint64_t s = 0; s < f.nsb;) {
				if (all_choice[s] == 1) {
					++s;
					continue;
				}
				uint64_t e = s;
				while (e < f.nsb && all_choice[e] != 1)
					++e;
				const size_t b0 = (size_t)(s * f.sb), b1 = (size_t)(e * f.sb < bytes ? e * f.sb : bytes);
				if (hipMemcpyAsync(img + b0, d_src + b0, b1 - b0, hipMemcpyDeviceToHost, copy) != hipSuccess)
					return STENOS_ERROR_UNDEFINED;
				s = e;
			}
		}
		for (uint64_t b = 0; b < nbatch; ++b) {
			const uint64_t s0 = b * batch, s1 = s0 + batch < f.nsb ? s0 + batch : f.nsb;
			const size_t lo = (size_t)sboff[s0], hi = (size_t)sboff[s1];
			if ((hi > lo && hipMemcpyAsync(blocks.data() + lo, j.dst + lo, hi - lo, hipMemcpyDeviceToHost, copy) != hipSuccess) ||
			    hipEventRecord(ctx->batch_ev[b], copy) != hipSuccess)
				return STENOS_ERROR_UNDEFINED;
		}
	}
	// zstd's result depends on the capacity only below ZSTD_compressBound of its input, so the superblocks of a
	// batch are compressed in parallel into roomy scratch buffers and then laid out in order; a superblock that
	// meets less room than that in the caller's buffer (the end of a tight buffer) is redone with the exact
	// capacity, as the reference's serial loop would have seen it.
	// Device destinations: the batch's slots go to the device as they are (one transfer, beside the next batch's zstd) and a
	// kernel puts every superblock at its place in the frame: the host's threads do not touch the bytes again.  Two sets of
	// slots, so that a batch can be compressed while the one before it is on its way.
	std::vector<int> choice;
	const size_t set_slots = (size_t)(batch < f.nsb ? batch : f.nsb) * ample;
	const int nsets = d_dst ? 2 : 1;
	if (!ctx->h_stage.ensure((size_t)nsets * set_slots)) // (kept by the context: a fresh 100 MB allocation per call costs more than the zstd calls)
		return STENOS_ERROR_ALLOC;
	const size_t tab_bytes = ((size_t)batch * 16 + 63) & ~(size_t)63; // per set: offsets, sizes (uint64 each)
	if (d_dst && (!ctx->dslots.ensure(2 * set_slots + 64) || !ctx->dtab.ensure(2 * tab_bytes + 64) || !ctx->h_tab.ensure(2 * tab_bytes + 64)))
		return STENOS_ERROR_ALLOC;
	if (d_dst && !ctx->ensure_events(ctx->set_ev, 2))
		return STENOS_ERROR_ALLOC;
	bool set_busy[2] = { false, false };
	struct { uint8_t* p; uint8_t* get() const { return p; } } scratch = { ctx->h_stage.data() };
	std::vector<size_t> sizes;
	std::vector<uint64_t> dslot; // position of a choice-4 superblock in the batch's delta buffer
	std::vector<size_t> offsets;
	std::vector<uint8_t> deltas;
	size_t off = f.header;
	auto upload = [&](size_t lo, size_t hi) -> bool { // frame bytes [lo, hi) that the host laid out in h_dst
		return !d_dst || hi <= lo || hipMemcpyAsync(d_dst + lo, h_dst + lo, hi - lo, hipMemcpyHostToDevice, up) == hipSuccess;
	};
	uint64_t nb = 0;
	for (uint64_t s0 = 0; s0 < f.nsb; s0 += batch, ++nb) {
		const uint64_t cnt = (s0 + batch < f.nsb ? s0 + batch : f.nsb) - s0;
		choice.assign(all_choice.begin() + (ptrdiff_t)s0, all_choice.begin() + (ptrdiff_t)(s0 + cnt));
		const int set = d_dst ? (int)(nb & 1) : 0;
		scratch.p = ctx->h_stage.data() + (size_t)set * set_slots;
		if (set_busy[set]) { // the slots of this set are still on their way to the device (two batches ago)
			if (hipEventSynchronize(ctx->set_ev[(size_t)set]) != hipSuccess)
				return STENOS_ERROR_UNDEFINED;
			set_busy[set] = false;
			trace.mark("slots to device", STAGE_UPLOAD);
		}
		if (hipEventSynchronize(ctx->batch_ev[s0 / batch]) != hipSuccess) // the batch's block streams (and the raw superblocks) are on the host
			return STENOS_ERROR_UNDEFINED;
		trace.mark("block streams to host", STAGE_BLOCKS_TO_HOST);
#ifdef STENOS_HOST_TRACE
		{
			unsigned h[5] = { 0, 0, 0, 0, 0 };
			for (uint64_t k = 0; k < cnt; ++k)
				++h[choice[k]];
			fprintf(stderr, "[stenos]   superblocks %llu: tiny %u, block codec %u, zstd %u, transposed %u, transposed+delta %u\n", (unsigned long long)cnt, h[0], h[1],
				h[2], h[3], h[4]);
		}
#endif
		// byte delta of the whole transposed superblock on the GPU for the choice-4 ones (stenos.cpp:646)
		dslot.assign(cnt, 0);
		uint64_t nd = 0;
		for (uint64_t k = 0; k < cnt; ++k)
			if (choice[k] == 4)
				dslot[k] = nd++;
		if (nd) {
			if (!ctx->tmp2.ensure(nd * f.sb + 64))
				return STENOS_ERROR_ALLOC;
			deltas.resize(nd * f.sb);
			for (uint64_t k = 0; k < cnt; ++k)
				if (choice[k] == 4) {
					const uint64_t s = s0 + k;
					const size_t sbytes = superblock_bytes(bytes, f.sb, s);
					if (stenos_k_launch_delta(ctx->shuf.as<uint8_t>() + s * f.sb, ctx->tmp2.as<uint8_t>() + dslot[k] * f.sb, sbytes, false, stream) !=
					    hipSuccess)
						return STENOS_ERROR_UNDEFINED;
				}
			if (hipMemcpyAsync(deltas.data(), ctx->tmp2.p, nd * f.sb, hipMemcpyDeviceToHost, stream) != hipSuccess ||
			    hipStreamSynchronize(stream) != hipSuccess)
				return STENOS_ERROR_UNDEFINED;
		}
		sizes.assign(cnt, 0);
		parallel_for(cnt, [&](uint64_t k) {
			sizes[k] = emit(s0 + k, choice[k], deltas.data() + dslot[k] * f.sb, scratch.get() + k * ample, ample);
		});
		trace.mark("zstd", STAGE_ZSTD);
		// Layout in order.  When even the last superblock of the batch finds ample room (the usual case), the
		// offsets are a plain prefix sum and the copies run on the worker threads.
		{
			size_t end = off;
			bool plain = true;
			offsets.resize(cnt);
			for (uint64_t k = 0; k < cnt && plain; ++k) {
				offsets[k] = end;
				plain = !is_err(sizes[k]) && dst_size >= end + ample;
				end += plain ? sizes[k] : 0;
			}
			if (plain && d_dst) { // laid out on the device
				uint64_t* tab = (uint64_t*)(ctx->h_tab.data() + (size_t)set * tab_bytes);
				for (uint64_t k = 0; k < cnt; ++k) {
					tab[k] = offsets[k];
					tab[batch + k] = sizes[k];
				}
				uint8_t* d_slots = ctx->dslots.as<uint8_t>() + (size_t)set * set_slots;
				uint64_t* d_tab = (uint64_t*)(ctx->dtab.as<uint8_t>() + (size_t)set * tab_bytes);
				if (hipMemcpyAsync(d_slots, scratch.get(), (size_t)cnt * ample, hipMemcpyHostToDevice, up) != hipSuccess ||
				    hipMemcpyAsync(d_tab, tab, (size_t)batch * 16, hipMemcpyHostToDevice, up) != hipSuccess ||
				    stenos_k_launch_gather_pieces(d_slots, ample, d_tab, d_tab + batch, (uint32_t)cnt, d_dst, up) != hipSuccess ||
				    hipEventRecord(ctx->set_ev[(size_t)set], up) != hipSuccess)
					return STENOS_ERROR_UNDEFINED;
				set_busy[set] = true;
				off = end;
				trace.mark("layout", STAGE_LAYOUT);
				continue;
			}
			if (plain) {
				parallel_for(cnt, [&](uint64_t k) { memcpy(h_dst + offsets[k], scratch.get() + k * ample, sizes[k]); });
				off = end;
				trace.mark("layout", STAGE_LAYOUT);
				continue;
			}
		}
		const size_t batch_begin = off;
		for (uint64_t k = 0; k < cnt; ++k) {
			if (dst_size < off + 4) // stenos.cpp:427-429
				return STENOS_ERROR_DST_OVERFLOW;
			const size_t room = dst_size - off;
			size_t r = sizes[k];
			if (room >= ample) {
				if (!is_err(r))
					memcpy(h_dst + off, scratch.get() + k * ample, r);
			}
			else
				r = emit(s0 + k, choice[k], deltas.data() + dslot[k] * f.sb, h_dst + off, room);
			if (is_err(r))
				return r;
			off += r;
		}
		trace.mark("layout", STAGE_LAYOUT);
		if (!upload(batch_begin, off)) // (a batch the host laid out itself: the end of a tight destination)
			return STENOS_ERROR_UNDEFINED;
	}
	if (d_dst) { // the frame header last; then everything has to be there
		if (!upload(0, f.header) || hipStreamSynchronize(up) != hipSuccess)
			return STENOS_ERROR_UNDEFINED;
		trace.mark("upload", STAGE_UPLOAD);
	}
	return off;
}

} // namespace stenos_host
