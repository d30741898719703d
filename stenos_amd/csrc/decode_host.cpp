// decode_host.cpp -- decoding on device memory: frame header checks, the decode launch, the host finish of zstd-coded
// superblocks, the index of a frame.
#include "frame_access.h"

namespace stenos_host {

// frame header checks of stenos_decompress_generic (stenos.cpp:1066-1116); returns 0 or an error code
size_t parse_frame(const uint8_t* h, size_t have, size_t T, size_t dst_size, FrameInfo& fi)
{
	if (T == 0 || T >= STENOS_MAX_BYTESOFTYPE)
		return STENOS_ERROR_INVALID_BYTESOFTYPE;
	if (have < 8)
		return STENOS_ERROR_SRC_OVERFLOW;
	const unsigned shift = h[0];
	if (shift > 4 && shift != 255)
		return STENOS_ERROR_INVALID_INPUT;
	fi.total = get_le(h + 1, 7);
	if (fi.total > dst_size)
		return STENOS_ERROR_DST_OVERFLOW;
	fi.header = 8;
	if (fi.total == 0)
		return 0;
	if (shift == 255) {
		if (have < 12)
			return STENOS_ERROR_SRC_OVERFLOW;
		fi.sb = (size_t)get_le(h + 8, 4);
		fi.header = 12;
		// what the compressor can have written (prepare(): a whole number of blocks' worth, below STENOS_MAX_BLOCK_BYTES);
		// the reference trusts the field (stenos.cpp:1098-1103) and would divide by zero or size buffers from garbage
		if (fi.sb < T * 256 || fi.sb >= STENOS_MAX_BLOCK_BYTES)
			return STENOS_ERROR_INVALID_INPUT;
	}
	else
		fi.sb = base_superblock(T * 256) << shift;
	// Unlike the reference (stenos.cpp:1115-1116, 1131) the last superblock of a frame whose size is an
	// exact multiple of the superblock size is decoded with its full size instead of 0 bytes.
	fi.nsb = fi.total / fi.sb + (fi.total % fi.sb ? 1 : 0);
	if (fi.nsb > 0x7FFFFFFFull) // one workgroup per superblock: beyond the grid limit (256 TiB of int32)
		return STENOS_ERROR_INVALID_PARAMETER;
	return 0;
}

// The arguments of a decode launch over nsb superblocks (the scratch of the wide kernels included); false: no memory for it
bool decode_args(stenos_context_s* ctx, const void* frame, size_t size, const uint64_t* sb_off, void* dst, uint64_t total, uint64_t nsb, size_t sb, size_t T,
		 uint32_t* status, DecodeArgs& a)
{
	a = DecodeArgs();
	a.frame = (const uint8_t*)frame;
	a.size = size;
	a.sb_off = sb_off;
	a.dst = (uint8_t*)dst;
	a.total_bytes = total;
	a.nsb = nsb;
	a.sb_bytes = (uint32_t)sb;
	a.T = (uint32_t)T;
	a.status = status;
	return wide_scratch(ctx, T, nsb, &a.wide_scratch, &a.wide_scratch_bytes);
}

// Finish the superblocks whose payload went through zstd (codes 2-5, decompress_generic_superblock,
// stenos.cpp:694-740): zstd itself runs on the host (third-party entropy coder, dlopen'ed), the byte kernels and
// the block decoder that follow it run on the device.  h_index: nsb + 1 header offsets on the host; h_frame: host
// copy of the frame or NULL (then the headers and payloads are fetched from the device).
size_t finish_host_codes(stenos_context_s* ctx, const uint8_t* d_frame, const uint8_t* h_frame, size_t size, size_t T, const uint64_t* h_index,
			 const FrameInfo& fi, uint8_t* d_dst, hipStream_t stream)
{
	PhaseTrace trace(ctx->stage_ms);
	// A frame that lives on the device comes to the host in pieces, on a stream of its own: the threads inflate the
	// superblocks of the first pieces while the rest is still on the link (the frame of 8 GiB of bytes at level 3 is 4 GB:
	// 80 ms of link time, as much as half the inflation).
	constexpr size_t PIECE = (size_t)64 << 20;
	const size_t pieces = h_frame ? 0 : (size + PIECE - 1) / PIECE;
	size_t pieces_here = 0;
	if (!h_frame) {
		HostBuf& frame_copy = ctx->h_in;
		if (!frame_copy.ensure(size + 64))
			return STENOS_ERROR_ALLOC;
		if (!ctx->ensure_stream(&ctx->copy_stream) || !ctx->ensure_events(ctx->set_ev, pieces))
			return STENOS_ERROR_ALLOC;
		h_frame = frame_copy.data();
	}
	// (the caller's stream has been waited for: the frame is complete on the device.  Only a few pieces are queued ahead of
	// the one being read: the copies of the inflated batches to the device wait behind whatever the other direction has queued)
	constexpr size_t AHEAD = 4;
	size_t pieces_queued = 0;
	auto queue_pieces = [&](size_t upto) -> bool {
		for (; pieces_queued < pieces && pieces_queued < upto; ++pieces_queued) {
			const size_t at = pieces_queued * PIECE, n = size - at < PIECE ? size - at : PIECE;
			if (hipMemcpyAsync(ctx->h_in.data() + at, d_frame + at, n, hipMemcpyDeviceToHost, ctx->copy_stream) != hipSuccess ||
			    hipEventRecord(ctx->set_ev[pieces_queued], ctx->copy_stream) != hipSuccess)
				return false;
		}
		return true;
	};
	auto frame_here = [&](size_t upto) -> bool { // the first `upto` bytes of the frame are on the host
		while (pieces_here < pieces && pieces_here * PIECE < upto) {
			if (!queue_pieces(pieces_here + 1 + AHEAD) || hipEventSynchronize(ctx->set_ev[pieces_here]) != hipSuccess)
				return false;
			++pieces_here;
		}
		return true;
	};
	struct Item {
		uint64_t s;
		uint32_t code;
		size_t csize, dsize, r;
	};
	std::vector<Item> items;
	uint64_t next_sb = 0;
	// the next (up to) `want` superblocks that went through zstd, in frame order; 0 or an error code
	auto collect = [&](size_t want) -> size_t {
		items.clear();
		for (; next_sb < fi.nsb && items.size() < want; ++next_sb) {
			const uint64_t s = next_sb;
			if (h_index[s] + 4 > size)
				return STENOS_ERROR_SRC_OVERFLOW;
			if (!frame_here(h_index[s] + 4))
				return STENOS_ERROR_UNDEFINED;
			const uint8_t* hd = h_frame + h_index[s];
			const unsigned code = hd[0];
			if (code == 1 || code == 6)
				continue;
			if (code < 2 || code > 5)
				return STENOS_ERROR_INVALID_INPUT;
			const size_t csize = (size_t)get_le(hd + 1, 3);
			const size_t dsize = superblock_bytes(fi.total, fi.sb, s);
			if (h_index[s] + 4 + csize > size)
				return STENOS_ERROR_INVALID_INPUT;
			if (!frame_here(h_index[s] + 4 + csize))
				return STENOS_ERROR_UNDEFINED;
			items.push_back({ s, code, csize, dsize, 0 });
		}
		return 0;
	};
	auto drain_frame = [&]() {
		if (pieces)
			(void)hipStreamSynchronize(ctx->copy_stream);
	};
	if (!zstd().ok) {
		// (only an error if a superblock needs it)
		size_t e = collect(1);
		drain_frame();
		return e ? e : items.empty() ? 0 : (size_t)STENOS_ERROR_ZSTD_INTERNAL;
	}

	// The superblocks are inflated by the worker threads into one staging buffer per batch (slot k: 12 spare bytes,
	// a [1][size:3] header for code 5, the bytes at +16), moved to the device in one copy and finished there.  Four sets of
	// buffers, each with a stream of its own: a batch is a few hundred superblocks, one wave each in the block decoder, which
	// is far from filling the device -- what a batch costs there is latency, and the batches of different sets overlap (the
	// copy of one beside the kernels of two others) while the threads inflate the next.
	constexpr int NSETS = 4;
	const size_t slot = (((size_t)fi.sb + 64 + 15) & ~(size_t)15) + 16;
	uint64_t batch = ((size_t)128 << 20) / slot;
	batch = batch < 64 ? 64 : batch > 1024 ? 1024 : batch;
	if (batch > fi.nsb)
		batch = fi.nsb;
	const size_t set_bytes = (batch * slot + 63) & ~(size_t)63, set_ids = (batch * 4 + 63) & ~(size_t)63, set_idx = (batch * 8 + 63) & ~(size_t)63;
	if (!ctx->tmp1.ensure(NSETS * set_bytes + 64) || !ctx->tmp2.ensure(NSETS * set_bytes + 64) || !ctx->bsize.ensure(NSETS * set_ids + 64) ||
	    !ctx->binfo.ensure(NSETS * set_idx + 64) || !ctx->misc.ensure(4096))
		return drain_frame(), STENOS_ERROR_ALLOC;
	HostBuf& stage = ctx->h_stage;
	// (behind the sets of slots: the superblock numbers and slot offsets of each batch, page-locked like the slots)
	const size_t tab_off = NSETS * set_bytes + 64;
	if (!stage.ensure(tab_off + NSETS * (set_ids + set_idx) + 64))
		return drain_frame(), STENOS_ERROR_ALLOC;
	if (!ctx->ensure_events(ctx->batch_ev, NSETS + 1))
		return drain_frame(), STENOS_ERROR_ALLOC;
	// (bytesoftype above 64 decodes through one scratch area, wide_scratch(): its batches stay in line on the caller's stream)
	const bool one_stream = T > STENOS_K_LDS_MAX_T;
	while (!one_stream && ctx->set_streams.size() < NSETS) {
		hipStream_t st = nullptr;
		if (!ctx->ensure_stream(&st))
			return drain_frame(), STENOS_ERROR_ALLOC;
		ctx->set_streams.push_back(st);
	}
	auto sync_all = [&]() {
		drain_frame();
		(void)hipStreamSynchronize(stream);
		for (hipStream_t st : ctx->set_streams)
			(void)hipStreamSynchronize(st);
	};
	// what the caller's stream has queued (the block-coded superblocks of this frame, whatever wrote the frame) comes first
	if (!one_stream) {
		hipEvent_t start = ctx->batch_ev[NSETS];
		if (hipEventRecord(start, stream) != hipSuccess)
			return drain_frame(), STENOS_ERROR_UNDEFINED;
		for (hipStream_t st : ctx->set_streams)
			if (hipStreamWaitEvent(st, start, 0) != hipSuccess)
				return drain_frame(), STENOS_ERROR_UNDEFINED;
	}
	std::vector<uint32_t> ids[NSETS];
	std::vector<uint64_t> idx[NSETS];
	volatile uint32_t* h_status = ctx->h_total->set_status; // (page-locked: the device writes it)
	bool pending[NSETS];
	for (int set = 0; set < NSETS; ++set) {
		h_status[set] = 0;
		pending[set] = false;
	}
	auto settle = [&](int set) -> size_t { // the batch that used this set of buffers is through
		if (!pending[set])
			return 0;
		pending[set] = false;
		if (hipEventSynchronize(ctx->batch_ev[(size_t)set]) != hipSuccess)
			return STENOS_ERROR_UNDEFINED;
		return h_status[set] ? (size_t)STENOS_ERROR_INVALID_INPUT : 0;
	};
	for (size_t nbatch = 0;; ++nbatch) {
		if (size_t e = collect((size_t)batch)) {
			sync_all();
			return e;
		}
		if (items.empty())
			break;
		constexpr size_t i0 = 0;
		const int set = (int)(nbatch % NSETS);
		hipStream_t const qs = one_stream ? stream : ctx->set_streams[(size_t)set];
		const size_t cnt = items.size();
		if (size_t e = settle(set)) {
			sync_all();
			return e;
		}
		trace.mark("device finish", STAGE_DEVICE_FINISH);
		uint8_t* const hs = stage.data() + (size_t)set * set_bytes;
		uint8_t* const t1 = ctx->tmp1.as<uint8_t>() + (size_t)set * set_bytes;
		uint8_t* const t2 = ctx->tmp2.as<uint8_t>() + (size_t)set * set_bytes;
		uint32_t* const d_ids = (uint32_t*)(ctx->bsize.as<uint8_t>() + (size_t)set * set_ids);
		uint64_t* const d_idx = (uint64_t*)(ctx->binfo.as<uint8_t>() + (size_t)set * set_idx);
		uint32_t* const d_status = &ctx->words()->set_status[set];
		parallel_for(cnt, [&](uint64_t k) {
			Item& it = items[i0 + k];
			// code 5: zstd over the block stream, at most the superblock size (stenos.cpp:732)
			const size_t cap = it.code == 5 ? (size_t)fi.sb + 64 : it.dsize;
			it.r = zstd().decompress(hs + k * slot + 16, cap, h_frame + h_index[it.s] + 4, it.csize);
		});
		trace.mark("zstd inflate", STAGE_INFLATE);
		ids[set].clear();
		idx[set].clear();
		for (size_t k = 0; k < cnt; ++k) {
			const Item& it = items[i0 + k];
			if (zstd().is_error(it.r) || (it.code != 5 && it.code != 2 && it.r != it.dsize)) { // stenos.cpp:696-698, 706-708, 718-720
				sync_all();
				return STENOS_ERROR_INVALID_INPUT;
			}
			if (it.code == 5) { // -> one BLOCK superblock for the block decoder (stenos.cpp:726-740)
				write_superblock_header(hs + k * slot + 12, 1, it.r);
				ids[set].push_back((uint32_t)it.s);
				idx[set].push_back(k * slot + 12);
			}
		}
		// Only the part of the slots that is in use goes up: an inflated block stream is about half its 256 KiB slot, and the
		// link is what the device's side of a batch waits for.  One strided copy (rows of the widest item, a slot apart).
		size_t width = 0;
		for (size_t k = 0; k < cnt; ++k) {
			const Item& it = items[i0 + k];
			const size_t w = 16 + (it.code == 5 ? it.r : it.dsize);
			width = w > width ? w : width;
		}
		width = (width + 63) & ~(size_t)63;
		width = width > slot ? slot : width;
		bool ok = hipMemcpy2DAsync(t1, slot, hs, slot, width, cnt, hipMemcpyHostToDevice, qs) == hipSuccess;
		for (size_t k = 0; k < cnt && ok; ++k) {
			const Item& it = items[i0 + k];
			uint8_t* out = d_dst + it.s * (uint64_t)fi.sb;
			const uint8_t* in = t1 + k * slot + 16;
			hipError_t e = hipSuccess;
			if (it.code == 2) // plain zstd
				e = hipMemcpyAsync(out, in, it.dsize, hipMemcpyDeviceToDevice, qs);
			else if (it.code == 3) // zstd on the transposed superblock (stenos.cpp:700-710)
				e = stenos_k_launch_shuffle(in, out, (uint32_t)T, it.dsize, true, qs);
			else if (it.code == 4) { // transposed + byte delta (stenos.cpp:711-725)
				e = stenos_k_launch_delta(in, t2 + k * slot, it.dsize, true, qs);
				if (e == hipSuccess)
					e = stenos_k_launch_shuffle(t2 + k * slot, out, (uint32_t)T, it.dsize, true, qs);
			}
			ok = e == hipSuccess;
		}
		if (ok && !ids[set].empty()) {
			// (the two small tables come from the page-locked buffer: a copy from pageable memory is staged by the runtime and
			// waits for the stream, which would keep the host from inflating the next batch meanwhile)
			uint8_t* h_ids = stage.data() + tab_off + (size_t)set * (set_ids + set_idx);
			uint8_t* h_idx = h_ids + set_ids;
			memcpy(h_ids, ids[set].data(), ids[set].size() * 4);
			memcpy(h_idx, idx[set].data(), idx[set].size() * 8);
			ok = hipMemcpyAsync(d_ids, h_ids, ids[set].size() * 4, hipMemcpyHostToDevice, qs) == hipSuccess &&
			     hipMemcpyAsync(d_idx, h_idx, idx[set].size() * 8, hipMemcpyHostToDevice, qs) == hipSuccess &&
			     hipMemsetAsync(d_status, 0, 4, qs) == hipSuccess;
			DecodeArgs a;
			ok = ok && decode_args(ctx, t1, cnt * slot, d_idx, d_dst, fi.total, ids[set].size(), fi.sb, T, d_status, a);
			a.sb_ids = d_ids;
			ok = ok && stenos_k_launch_decode(a, qs) == hipSuccess && hipMemcpyAsync((void*)(h_status + set), d_status, 4, hipMemcpyDeviceToHost, qs) == hipSuccess;
		}
		ok = ok && hipEventRecord(ctx->batch_ev[(size_t)set], qs) == hipSuccess;
		if (!ok) {
			sync_all();
			return STENOS_ERROR_UNDEFINED;
		}
		pending[set] = true;
	}
	drain_frame();
	for (int set = 0; set < NSETS; ++set)
		if (size_t e = settle(set)) {
			sync_all();
			return e;
		}
	trace.mark("device finish", STAGE_DEVICE_FINISH);
	return 0;
}

size_t decompress_device(stenos_context_s* ctx, const void* d_src, size_t T, size_t size, void* d_dst, size_t dst_size, const uint64_t* d_index,
			 const uint64_t* h_index, const uint8_t* h_frame, hipStream_t stream, bool wait)
{
	if (!ctx->device_ready())
		return STENOS_ERROR_INVALID_INSTRUCTION_SET;
	FrameInfo fi;
	size_t e = fetch_frame_info(d_src, T, size, dst_size, stream, fi);
	if (is_err(e))
		return e;
	ctx->job_kind = 0;
	if (fi.total == 0)
		return 0;
	if (!ctx->misc.ensure(4096))
		return STENOS_ERROR_ALLOC;
	uint32_t* d_status = &ctx->words()->decode_status;
	if (hipMemsetAsync(d_status, 0, 4, stream) != hipSuccess)
		return STENOS_ERROR_UNDEFINED;
	if ((e = frame_offsets(ctx, d_src, size, fi, &d_index, nullptr, d_status, stream)))
		return e;
	DecodeArgs a;
	if (!decode_args(ctx, d_src, size, d_index, d_dst, fi.total, fi.nsb, fi.sb, T, d_status, a))
		return STENOS_ERROR_ALLOC;
	ctx->mark(2, stream);
	if (stenos_k_launch_decode(a, stream) != hipSuccess)
		return STENOS_ERROR_UNDEFINED;
	ctx->mark(3, stream);
	if (hipMemcpyAsync(&ctx->h_total->decode_status, d_status, 4, hipMemcpyDeviceToHost, stream) != hipSuccess)
		return STENOS_ERROR_UNDEFINED;
	ctx->set_job(2, stream, !wait, (size_t)fi.total);
	if (!wait)
		return 0;
	size_t r = finish_job(ctx);
	if (!is_err(r) && ctx->job_host_codes) { // zstd-based superblocks present
		std::vector<uint64_t> idx;
		if (!h_index) {
			idx.resize(fi.nsb + 1);
			if (hipMemcpy(idx.data(), d_index, (fi.nsb + 1) * 8, hipMemcpyDeviceToHost) != hipSuccess)
				return STENOS_ERROR_UNDEFINED;
			h_index = idx.data();
		}
		e = finish_host_codes(ctx, (const uint8_t*)d_src, h_frame, size, T, h_index, fi, (uint8_t*)d_dst, stream);
		return is_err(e) ? e : (size_t)fi.total;
	}
	return r;
}

const uint64_t* frame_index(stenos_context_s* ctx, const void* d_src, size_t bytesoftype, size_t bytes, size_t* nsb, hipStream_t stream)
{
	if (nsb)
		*nsb = 0;
	if (!ctx || !d_src || !ctx->device_ready())
		return nullptr;
	FrameInfo fi;
	if (fetch_frame_info(d_src, bytesoftype, bytes, ~(size_t)0, stream, fi) || fi.total == 0 || !ctx->misc.ensure(4096))
		return nullptr;
	uint32_t* d_status = &ctx->words()->decode_status;
	uint32_t status = 0;
	const uint64_t* index = nullptr;
	if (hipMemsetAsync(d_status, 0, 4, stream) != hipSuccess || frame_offsets(ctx, d_src, bytes, fi, &index, nullptr, d_status, stream) ||
	    hipMemcpyAsync(&status, d_status, 4, hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess || status)
		return nullptr; // a header or payload runs past the end of the frame
	if (nsb)
		*nsb = (size_t)fi.nsb;
	return index;
}

} // namespace stenos_host
