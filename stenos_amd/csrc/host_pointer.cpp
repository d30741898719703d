// host_pointer.cpp -- the host-pointer ABI on top of the device calls: staging, chunked overlap, page-locked aliasing,
// several devices, time-limited compression.
#include <atomic>
#include <condition_variable>
#include <mutex>
#include <new>
#include <thread>

#include "host.h"

namespace stenos_host {
namespace {

// ---- host-pointer calls on large inputs -------------------------------------------------------------
// The link is full duplex and the codec is ~30x faster than it, so the call is cut into chunks of whole superblocks:
// a helper thread uploads chunk k+1 on its own stream while the calling thread codes chunk k and downloads the
// result.  A chunk is a frame of its own on the device (superblocks are independent units, stenos.cpp:893-904), the
// caller's frame is the concatenation of the chunks' superblock streams behind one header.
constexpr size_t kHostChunkBytes = 32u << 20; // ~0.6 ms of link time, ~0.25 ms of fixed cost of a device call
constexpr size_t kHostChunkedFrom = 3 * kHostChunkBytes;

class Uploader {
	std::thread th;
	std::mutex m;
	std::condition_variable cv;
	size_t ready = 0;
	bool failed = false;
	std::atomic<bool> cancel{ false };

public:
	bool start(size_t chunks, std::function<bool(size_t)> upload) // false: no thread to be had (the caller takes the single pass)
	{
		int device = 0;
		(void)hipGetDevice(&device);
		try {
			th = std::thread([this, chunks, upload, device] {
			bool ok = hipSetDevice(device) == hipSuccess;
			for (size_t k = 0; k < chunks; ++k) {
				ok = ok && !cancel.load() && upload(k);
				std::lock_guard<std::mutex> l(m);
				failed = !ok;
				ready = ok ? k + 1 : chunks; // nobody waits for ever
				cv.notify_all();
				if (!ok)
					break;
			}
			});
		}
		catch (...) {
			return false;
		}
		return true;
	}
	bool wait_for(size_t k)
	{
		std::unique_lock<std::mutex> l(m);
		cv.wait(l, [&] { return ready > k; });
		return !failed;
	}
	~Uploader()
	{
		cancel = true;
		if (th.joinable())
			th.join();
	}
};

inline bool chunk_streams(stenos_context_s* ctx)
{
	return ctx->ensure_stream(&ctx->up_stream) && ctx->ensure_stream(&ctx->main_stream);
}

// *no_thread: the helper thread could not be started and nothing has been done (the caller takes the single pass)
size_t compress_chunked(stenos_context_s* ctx, const uint8_t* src, size_t T, size_t bytes, uint8_t* out, size_t dst_size, const FramePlan& f, bool* no_thread)
{
	*no_thread = false;
	const size_t chunk = kHostChunkBytes / f.sb * f.sb;
	const size_t chunks = (bytes + chunk - 1) / chunk;
	const size_t worst = f.header + (chunk / f.sb) * 4 + chunk; // a chunk stored as copies
	if (!chunk_streams(ctx) || !ctx->in.ensure(bytes + 64) || !ctx->out.ensure((dst_size < worst ? dst_size : worst) + 64))
		return STENOS_ERROR_ALLOC;
	uint8_t* d_in = ctx->in.as<uint8_t>();
	hipStream_t up_stream = ctx->up_stream, stream = ctx->main_stream;
	Uploader up;
	if (!up.start(chunks, [=](size_t k) {
		    const size_t begin = k * chunk, n = bytes - begin < chunk ? bytes - begin : chunk;
		    return hipMemcpyAsync(d_in + begin, src + begin, n, hipMemcpyHostToDevice, up_stream) == hipSuccess && hipStreamSynchronize(up_stream) == hipSuccess;
	    })) {
		*no_thread = true;
		return STENOS_ERROR_ALLOC;
	}
	write_frame_header(out, f.shift, bytes, f.sb);
	size_t off = f.header;
	for (size_t k = 0; k < chunks; ++k) {
		if (!up.wait_for(k))
			return STENOS_ERROR_UNDEFINED;
		const size_t begin = k * chunk, n = bytes - begin < chunk ? bytes - begin : chunk;
		// the chunk's frame sees the capacity the caller's buffer has left, so every superblock meets the room it would
		// meet in a single pass (stenos.cpp:893-904)
		const size_t room = dst_size - off + f.header;
		const size_t r = compress_device(ctx, d_in + begin, T, n, ctx->out.p, room, stream, true);
		if (is_err(r))
			return r;
		if (hipMemcpyAsync(out + off, ctx->out.as<uint8_t>() + f.header, r - f.header, hipMemcpyDeviceToHost, stream) != hipSuccess ||
		    hipStreamSynchronize(stream) != hipSuccess)
			return STENOS_ERROR_UNDEFINED;
		off += r - f.header;
	}
	return off;
}

// h_index: offsets of the superblock headers in the frame and its end (walked by the caller); only codes 1 and 6 inside.
// Superblocks [sA, sB) of the frame -> their bytes of `out`.
size_t decompress_chunked(stenos_context_s* ctx, const uint8_t* in, size_t T, const FrameInfo& fi, const std::vector<uint64_t>& h_index, uint8_t* out, uint64_t sA,
			  uint64_t sB, bool* no_thread = nullptr)
{
	if (no_thread)
		*no_thread = false;
	const uint64_t per = kHostChunkBytes / fi.sb ? kHostChunkBytes / fi.sb : 1; // superblocks per chunk
	const uint64_t count = sB - sA;
	const size_t chunks = (size_t)((count + per - 1) / per);
	const size_t size = (size_t)(h_index[sB] - h_index[sA]);
	const uint64_t oA = sA * fi.sb, oB = sB * fi.sb < fi.total ? sB * fi.sb : fi.total;
	const size_t H = fi.header; // 8, or 12 with a custom superblock size (repeated in every chunk's header)
	// chunk k on the device: [frame header of its own][its superblocks], 16 bytes further than in the frame per chunk
	// before it so that the headers do not overlap the neighbours; its index in sboff at entry (s0 - sA) + k
	ctx->last_frames = 0; // (the index workspace takes the chunks' offsets)
	if (!chunk_streams(ctx) || !ctx->in.ensure(size + 16 * (chunks + 1) + H + 64) || !ctx->out.ensure((size_t)(oB - oA) + 64) || !ctx->sboff.ensure((count + chunks + 2) * 8))
		return STENOS_ERROR_ALLOC;
	std::vector<uint64_t> rel(count + chunks);
	std::vector<uint8_t> hdr(12 * chunks);
	for (size_t k = 0; k < chunks; ++k) {
		const uint64_t s0 = sA + k * per, s1 = s0 + per < sB ? s0 + per : sB;
		for (uint64_t s = s0; s <= s1; ++s)
			rel[s - sA + k] = h_index[s] - h_index[s0] + H;
		const uint64_t o0 = s0 * fi.sb, o1 = s1 * fi.sb < fi.total ? s1 * fi.sb : fi.total;
		write_frame_header(&hdr[12 * k], in[0], o1 - o0, fi.sb);
	}
	uint8_t* d_in = ctx->in.as<uint8_t>();
	uint64_t* d_rel = ctx->sboff.as<uint64_t>();
	hipStream_t up_stream = ctx->up_stream, stream = ctx->main_stream;
	const uint64_t* idx = h_index.data();
	const uint64_t* relp = rel.data();
	const uint8_t* hdrp = hdr.data();
	auto chunk_frame = [=](size_t k) { return d_in + (idx[sA + k * per] - idx[sA]) + 16 * (k + 1); };
	Uploader up;
	if (!up.start(chunks, [=](size_t k) {
		    const uint64_t s0 = sA + k * per, s1 = s0 + per < sB ? s0 + per : sB;
		    uint8_t* d = chunk_frame(k);
		    return hipMemcpyAsync(d, hdrp + 12 * k, H, hipMemcpyHostToDevice, up_stream) == hipSuccess &&
			   hipMemcpyAsync(d + H, in + idx[s0], idx[s1] - idx[s0], hipMemcpyHostToDevice, up_stream) == hipSuccess &&
			   hipMemcpyAsync(d_rel + (s0 - sA) + k, relp + (s0 - sA) + k, (s1 - s0 + 1) * 8, hipMemcpyHostToDevice, up_stream) == hipSuccess &&
			   hipStreamSynchronize(up_stream) == hipSuccess;
	    })) {
		if (no_thread)
			*no_thread = true;
		return STENOS_ERROR_ALLOC;
	}
	for (size_t k = 0; k < chunks; ++k) {
		if (!up.wait_for(k))
			return STENOS_ERROR_UNDEFINED;
		const uint64_t s0 = sA + k * per, s1 = s0 + per < sB ? s0 + per : sB;
		const uint64_t o0 = s0 * fi.sb, o1 = s1 * fi.sb < fi.total ? s1 * fi.sb : fi.total;
		uint8_t* d_out = ctx->out.as<uint8_t>() + (o0 - oA);
		const size_t r = decompress_device(ctx, chunk_frame(k), T, (size_t)(H + h_index[s1] - h_index[s0]), d_out, (size_t)(o1 - o0), d_rel + (s0 - sA) + k, nullptr, nullptr,
						   stream, true);
		if (is_err(r))
			return r;
		if (r != o1 - o0 || ctx->job_host_codes)
			return STENOS_ERROR_INVALID_INPUT;
		if (hipMemcpyAsync(out + o0, d_out, (size_t)(o1 - o0), hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess)
			return STENOS_ERROR_UNDEFINED;
	}
	return (size_t)(oB - oA);
}

// ---- host-pointer calls on page-locked memory ---------------------------------------------------------
// Memory the caller has page-locked (hipHostMalloc, hipHostRegister, a pinned tensor) is visible to the device: the
// kernels then read the input and write the frame THROUGH the link, both directions at once, with no staging copy on
// either side -- the call is bound by the larger of the two transfers instead of their sum.  Returns the device alias of
// [p, p + n) or NULL (pageable memory, or a range that leaves its registration).
void* device_alias(const void* p, size_t n)
{
	hipPointerAttribute_t a;
	if (!p || hipPointerGetAttributes(&a, p) != hipSuccess) {
		(void)hipGetLastError(); // (pageable memory is "invalid value" to the runtime)
		return nullptr;
	}
	if (a.type != hipMemoryTypeHost || !a.devicePointer)
		return nullptr;
	void* base = nullptr;
	size_t size = 0;
	if (hipMemGetAddressRange((hipDeviceptr_t*)&base, &size, (hipDeviceptr_t)a.devicePointer) != hipSuccess) {
		(void)hipGetLastError();
		return nullptr;
	}
	const uintptr_t lo = (uintptr_t)a.devicePointer, end = (uintptr_t)base + size;
	return lo >= (uintptr_t)base && lo + n <= end ? a.devicePointer : nullptr;
}

// ---- host-pointer calls on several devices ------------------------------------------------------------
// The reference's dispatcher hands superblocks to the threads of stenos_set_threads (stenos.cpp:909-1010, 1151-1202).
// Here a host-pointer call is bound by the PCIe link of the device, not by the codec, so what pays is more DEVICES --
// more links -- per call.  That is opt-in (stenos_hip_set_devices, or STENOS_HIP_DEVICES >= 2 in the environment): the
// devices of a process are not the caller's to take just because it asked for CPU threads.  With it, a call uses
// min(threads, devices) of them: superblocks are independent in both directions, every device takes a
// contiguous range of them through a child context driven by a host thread of its own, and nothing is exchanged between
// devices (no collective: the caller's buffers are the meeting point).
//   compress:   every device uploads and encodes its range (a frame of its own, roomy destination); the sizes meet on
//               the host, a prefix sum gives every range its place and each device downloads straight to it.  Only
//               superblocks whose encoding cannot depend on the room that is left (safe_superblocks) are shared out; the
//               last one or two of a frame -- or all of them under a tight dst_size -- follow on the calling thread's
//               device with the exact room, as in the single-device path.
//   decompress: the host walks the superblock headers anyway; every device gets a range of them and writes its bytes.
// stenos_hip_test_lanes (tests on a one-GPU box) lets the lanes share the current device and makes one of them fail.
constexpr size_t kLanesFrom = (size_t)64 << 20; // below, one link moves the data before a second thread is up

// devices visible to the process (asked once: the answer does not change while the process lives)
int visible_devices()
{
	static const int n = [] {
		int k = 0;
		return hipGetDeviceCount(&k) == hipSuccess && k > 0 ? k : 1;
	}();
	return n;
}
// How many devices a host-pointer call of `bytes` may spread over.  Opt-in: stenos_hip_set_devices(ctx, n >= 2), or the
// environment variable STENOS_HIP_DEVICES >= 2 (read once) for callers that cannot be changed; without either a call stays
// on the calling thread's device whatever stenos_set_threads() says (the reference's CPU-thread knob, stenos.h:140).
int lane_count(stenos_context_s* ctx, size_t bytes)
{
	if (ctx->threads <= 1 || bytes < kLanesFrom)
		return 1;
	static const int env = [] {
		const char* e = getenv("STENOS_HIP_DEVICES");
		return e ? atoi(e) : 0;
	}();
	int n = ctx->hip_devices > 0 ? ctx->hip_devices : env;
	if (n < 2)
		return 1;
	if (!ctx->test_lanes_share_device && n > visible_devices())
		n = visible_devices();
	return n < ctx->threads ? n : ctx->threads;
}
// lane 0 is the context itself (the calling thread's device); lane i > 0 a child on device (current + i) % count
stenos_context_s* lane_context(stenos_context_s* ctx, int i, int* device)
{
	int cur = 0;
	(void)hipGetDevice(&cur);
	*device = ctx->test_lanes_share_device ? cur : (cur + i) % visible_devices();
	if (i == 0)
		return ctx;
	if ((int)ctx->lanes.size() < i)
		ctx->lanes.resize((size_t)i, nullptr);
	stenos_context_s*& l = ctx->lanes[(size_t)i - 1];
	if (!l) {
		void* m = malloc(sizeof(stenos_context_s));
		if (!m)
			return nullptr;
		l = new (m) stenos_context_s();
	}
	l->level = ctx->level;
	l->threads = 1;
	l->max_nanoseconds = 0;
	l->custom_shift = ctx->custom_shift;
	return l;
}
// Runs fn(i) for every lane on a thread of its own (lane 0 on the calling thread) with the lane's device current.
// result[i] must hold an error code on entry: a lane whose thread cannot be started, whose device cannot be made current
// or that is made to fail by the test hook leaves it there, so a lane that never ran is an error, not a result of 0.
bool run_lanes(stenos_context_s* ctx, int n, const std::vector<int>& device, const std::function<void(int)>& fn)
{
	std::vector<std::thread> th;
	bool ok = true;
	const int fail = ctx->test_fail_lane;
	for (int i = 1; i < n; ++i) {
		try {
			th.emplace_back([&, i] {
				if (i != fail && hipSetDevice(device[(size_t)i]) == hipSuccess)
					fn(i);
			});
		}
		catch (...) {
			ok = false;
			break;
		}
	}
	if (ok && fail != 0)
		fn(0);
	for (std::thread& t : th)
		t.join();
	return ok;
}

size_t compress_lanes(stenos_context_s* ctx, const uint8_t* src, size_t T, size_t bytes, uint8_t* out, size_t dst_size, const FramePlan& f, int n)
{
	// superblocks that are coded the same whatever room is left, all of them full: these are shared out
	uint64_t safe = codec::safe_superblocks(dst_size, f.header, f.bps, (uint32_t)T, f.sb, f.nsb);
	const uint64_t whole = f.nfull / f.bps;
	safe = safe < whole ? safe : whole;
	if (safe < (uint64_t)(2 * n))
		return STENOS_ERROR_INVALID_PARAMETER; // (not an error: the caller takes the single-device path)
	std::vector<stenos_context_s*> lane((size_t)n);
	std::vector<int> device((size_t)n);
	for (int i = 0; i < n; ++i)
		if (!(lane[(size_t)i] = lane_context(ctx, i, &device[(size_t)i])))
			return STENOS_ERROR_ALLOC;
	std::vector<size_t> got((size_t)n, (size_t)STENOS_ERROR_UNDEFINED); // (a lane that never runs is an error)
	auto range = [&](int i, uint64_t* a, uint64_t* b) {
		*a = safe * (uint64_t)i / (uint64_t)n;
		*b = safe * (uint64_t)(i + 1) / (uint64_t)n;
	};
	// upload + encode
	if (!run_lanes(ctx, n, device, [&](int i) {
		    stenos_context_s* c = lane[(size_t)i];
		    uint64_t a, b;
		    range(i, &a, &b);
		    const size_t nb = (size_t)(b - a) * f.sb, worst = f.header + (size_t)(b - a) * 4 + nb + 4096;
		    if (!c->device_ready() || !chunk_streams(c) || !c->in.ensure(nb + 64) || !c->out.ensure(worst + 64)) {
			    got[(size_t)i] = STENOS_ERROR_ALLOC;
			    return;
		    }
		    if (hipMemcpyAsync(c->in.p, src + a * f.sb, nb, hipMemcpyHostToDevice, c->main_stream) != hipSuccess) {
			    got[(size_t)i] = STENOS_ERROR_UNDEFINED;
			    return;
		    }
		    got[(size_t)i] = compress_device(c, c->in.p, T, nb, c->out.p, worst, c->main_stream, true);
	    }))
		return STENOS_ERROR_ALLOC;
	std::vector<size_t> off((size_t)n + 1);
	off[0] = f.header;
	for (int i = 0; i < n; ++i) {
		if (is_err(got[(size_t)i]))
			return got[(size_t)i];
		if (got[(size_t)i] < f.header)
			return STENOS_ERROR_UNDEFINED;
		off[(size_t)i + 1] = off[(size_t)i] + got[(size_t)i] - f.header;
	}
	if (off[(size_t)n] > dst_size)
		return STENOS_ERROR_DST_OVERFLOW; // (cannot happen for safe superblocks; never write past the buffer)
	// download, every range to its place
	std::vector<int> bad((size_t)n, 1); // (cleared by the lane once its bytes are in place)
	if (!run_lanes(ctx, n, device, [&](int i) {
		    stenos_context_s* c = lane[(size_t)i];
		    if (hipMemcpyAsync(out + off[(size_t)i], c->out.as<uint8_t>() + f.header, got[(size_t)i] - f.header, hipMemcpyDeviceToHost, c->main_stream) == hipSuccess &&
			hipStreamSynchronize(c->main_stream) == hipSuccess)
			    bad[(size_t)i] = 0;
	    }))
		return STENOS_ERROR_ALLOC;
	for (int b : bad)
		if (b)
			return STENOS_ERROR_UNDEFINED;
	write_frame_header(out, f.shift, bytes, f.sb);
	size_t end = off[(size_t)n];
	if (safe < f.nsb) { // the superblocks that look at the room: one more frame, with exactly the room the caller's buffer has left
		const size_t begin = (size_t)safe * f.sb, rest = bytes - begin;
		const size_t room = dst_size - end + f.header, worst = f.header + (size_t)(f.nsb - safe) * 4 + rest;
		if (!ctx->in.ensure(rest + 64) || !ctx->out.ensure((room < worst ? room : worst) + 64))
			return STENOS_ERROR_ALLOC;
		if (hipMemcpy(ctx->in.p, src + begin, rest, hipMemcpyHostToDevice) != hipSuccess)
			return STENOS_ERROR_UNDEFINED;
		const size_t r = compress_device(ctx, ctx->in.p, T, rest, ctx->out.p, room, nullptr, true);
		if (is_err(r))
			return r;
		if (hipMemcpy(out + end, ctx->out.as<uint8_t>() + f.header, r - f.header, hipMemcpyDeviceToHost) != hipSuccess)
			return STENOS_ERROR_UNDEFINED;
		end += r - f.header;
	}
	return end;
}

size_t decompress_lanes(stenos_context_s* ctx, const uint8_t* in, size_t T, const FrameInfo& fi, const std::vector<uint64_t>& h_index, uint8_t* out, int n)
{
	std::vector<stenos_context_s*> lane((size_t)n);
	std::vector<int> device((size_t)n);
	for (int i = 0; i < n; ++i)
		if (!(lane[(size_t)i] = lane_context(ctx, i, &device[(size_t)i])))
			return STENOS_ERROR_ALLOC;
	std::vector<size_t> got((size_t)n, (size_t)STENOS_ERROR_UNDEFINED); // (a lane that never runs is an error)
	if (!run_lanes(ctx, n, device, [&](int i) {
		    const uint64_t a = fi.nsb * (uint64_t)i / (uint64_t)n, b = fi.nsb * (uint64_t)(i + 1) / (uint64_t)n;
		    stenos_context_s* c = lane[(size_t)i];
		    got[(size_t)i] = !c->device_ready() ? (size_t)STENOS_ERROR_INVALID_INSTRUCTION_SET : (a < b ? decompress_chunked(c, in, T, fi, h_index, out, a, b) : 0);
	    }))
		return STENOS_ERROR_ALLOC;
	for (size_t r : got)
		if (is_err(r))
			return r;
	return (size_t)fi.total;
}

// Time-limited compression (stenos_set_max_nanoseconds).  The reference keeps adjusting its level to the time that is left:
// per block inside the block codec, down to blocks stored as they are (block_compress.h:1024-1075, 1158-1176), per
// superblock for the zstd stages (zstd_wrapper.h:118-174, stenos.cpp:471-490), on superblocks sized after the thread
// count (stenos.cpp:126-149), and finishes with plain copies when nothing else fits.  Its output depends on the clock and
// is not reproducible.  Here the unit of adjustment is a slice of whole superblocks (default size, frame byte 0): before
// each slice the host clock and the rates measured so far decide whether the slice goes through zstd on top of the block
// codec (level 2, when the context's level allows it), through the block codec (level 1) or is stored as copies; a slice
// is only compressed when copying everything behind it would still fit the time that is left.  Every frame decodes with
// the ordinary decoder.
size_t compress_timed(stenos_context* ctx, const uint8_t* src, size_t T, size_t bytes, uint8_t* out, size_t dst_size)
{
	using clock = std::chrono::steady_clock;
	const auto start = clock::now();
	const double budget = (double)ctx->max_nanoseconds * 1e-9;
	if (T == 0 || T >= STENOS_MAX_BYTESOFTYPE)
		return STENOS_ERROR_INVALID_BYTESOFTYPE;
	const size_t sb = base_superblock(T * 256);
	if (dst_size < 8)
		return STENOS_ERROR_DST_OVERFLOW;
	write_frame_header(out, 0, bytes, 0);
	// slices of 1/16 of the input, between 4 and 64 MiB: enough of them to adjust, each large enough for the device
	size_t slice = bytes / 16;
	slice = slice < ((size_t)4 << 20) ? ((size_t)4 << 20) : (slice > ((size_t)64 << 20) ? ((size_t)64 << 20) : slice);
	slice = (slice + sb - 1) / sb * sb;
	const int top = ctx->level > 2 ? 2 : ctx->level; // levels above 2 change the superblock size of a frame: not inside one frame
	double rate[3] = { 6e9, 12e9, 1e9 }; // bytes per second of a slice stored as copies / at level 1 / at level 2: first guesses, then measured
	const int saved_level = ctx->level;
	const uint64_t saved_ns = ctx->max_nanoseconds;
	const size_t saved_shift = ctx->custom_shift; // (the reference's time-limited frames choose their superblock size themselves, too)
	size_t off = 8, pos = 0, result = 0;
	while (pos < bytes) {
		const size_t n = bytes - pos < slice ? bytes - pos : slice;
		const double left = budget - std::chrono::duration<double>(clock::now() - start).count();
		const double rest = (double)(bytes - pos - n) / rate[0]; // what copying everything behind this slice takes
		// the first device call of a context also pays for the runtime's start, the code object and the buffers: a tight
		// budget on a cold context is better spent copying
		const double cold = ctx->warm ? 0.0 : 0.25;
		int level = 0;
		if (top >= 1 && left > 0 && (double)n / rate[1] + rest + cold <= left)
			level = 1;
		if (level == 1 && top >= 2 && zstd().ok && (double)n / rate[2] + rest <= left * 0.5)
			level = 2;
		const auto t0 = clock::now();
		size_t r;
		if (level == 0) {
			const size_t nsb = n / sb + (n % sb ? 1 : 0);
			if (dst_size - off < n + 4 * nsb) {
				result = STENOS_ERROR_DST_OVERFLOW;
				break;
			}
			for (size_t s = 0; s < nsb; ++s) // compress_memcpy (stenos.cpp:363-374)
				off += copy_superblock(out + off, src + pos + s * sb, superblock_bytes(n, sb, s));
			r = 0;
		}
		else {
			// the slice as a frame of its own, written so that its 8-byte header falls on the 8 bytes in front of `off`
			uint8_t keep[8];
			memcpy(keep, out + off - 8, 8);
			ctx->level = level;
			ctx->max_nanoseconds = 0;
			ctx->custom_shift = STENOS_NO_BLOCK_SHIFT;
			r = compress_host(ctx, src + pos, T, n, out + off - 8, dst_size - off + 8);
			ctx->level = saved_level;
			ctx->max_nanoseconds = saved_ns;
			ctx->custom_shift = saved_shift;
			memcpy(out + off - 8, keep, 8);
			if (is_err(r)) {
				result = r;
				break;
			}
			off += r - 8;
		}
		const double took = std::chrono::duration<double>(clock::now() - t0).count();
		if (took > 0)
			rate[level] = 0.5 * rate[level] + 0.5 * (double)n / took;
		pos += n;
	}
	return is_err(result) ? result : off;
}

// "Stage the input up, run the device call, bring the result down."  a_src / a_dst: the device alias of the caller's
// page-locked memory on that side (no staging there), or NULL.
size_t compress_staged(stenos_context_s* ctx, const void* src, size_t T, size_t bytes, void* dst, size_t dst_size, const FramePlan& f, void* a_src, void* a_dst)
{
	// the largest frame there can be: every superblock stored as a copy.  (stenos_bound() assumes superblocks of the
	// default size; with stenos_set_block_size() there can be many more headers.)  Nothing is written past dst_size.
	const size_t worst = f.header + f.nsb * 4 + bytes;
	if ((!a_src && !ctx->in.ensure(bytes + 64)) || (!a_dst && !ctx->out.ensure((dst_size < worst ? dst_size : worst) + 64)))
		return STENOS_ERROR_ALLOC;
	if (!a_src && hipMemcpy(ctx->in.p, src, bytes, hipMemcpyHostToDevice) != hipSuccess)
		return STENOS_ERROR_UNDEFINED;
	if (needs_strategy(T, ctx->level)) // (never aliased) the host assembles the frame in the caller's buffer
		return compress_strategy(ctx, (const uint8_t*)src, ctx->in.as<uint8_t>(), T, bytes, (uint8_t*)dst, dst_size, ctx->level, f, nullptr);
	// the caller's dst_size is the logical capacity (a frame that does not fit is reported, nothing is written past it)
	const size_t r = compress_device(ctx, a_src ? a_src : ctx->in.p, T, bytes, a_dst ? a_dst : ctx->out.p, dst_size, nullptr, true);
	if (is_err(r))
		return r;
	if (!a_dst && hipMemcpy(dst, ctx->out.p, r, hipMemcpyDeviceToHost) != hipSuccess)
		return STENOS_ERROR_UNDEFINED;
	return r;
}
size_t decompress_staged(stenos_context_s* ctx, const void* src, size_t T, size_t size, void* dst, const FrameInfo& fi, const std::vector<uint64_t>& index, void* a_src,
			 void* a_dst)
{
	const size_t total = (size_t)fi.total;
	ctx->last_frames = 0; // (the index workspace takes this frame's offsets)
	if ((!a_src && !ctx->in.ensure(size + 64)) || (!a_dst && !ctx->out.ensure(total + 64)) || !ctx->sboff.ensure((fi.nsb + 2) * 8))
		return STENOS_ERROR_ALLOC;
	if ((!a_src && hipMemcpy(ctx->in.p, src, size, hipMemcpyHostToDevice) != hipSuccess) ||
	    hipMemcpy(ctx->sboff.p, index.data(), (fi.nsb + 1) * 8, hipMemcpyHostToDevice) != hipSuccess)
		return STENOS_ERROR_UNDEFINED;
	const size_t r = decompress_device(ctx, a_src ? a_src : ctx->in.p, T, size, a_dst ? a_dst : ctx->out.p, total, ctx->sboff.as<uint64_t>(), index.data(),
					   (const uint8_t*)src, nullptr, true);
	if (is_err(r))
		return r;
	if (!a_dst && hipMemcpy(dst, ctx->out.p, total, hipMemcpyDeviceToHost) != hipSuccess)
		return STENOS_ERROR_UNDEFINED;
	return total;
}

} // namespace

size_t compress_host(stenos_context_s* ctx, const void* src, size_t bytesoftype, size_t bytes, void* dst, size_t dst_size)
{
	FramePlan f;
	size_t e = plan_frame(ctx, bytesoftype, bytes, ctx->level, f);
	if (is_err(e))
		return e;
	if (ctx->max_nanoseconds && bytes && ctx->level)
		return compress_timed(ctx, (const uint8_t*)src, bytesoftype, bytes, (uint8_t*)dst, dst_size);
	e = check_supported(ctx, bytesoftype, ctx->level);
	if (is_err(e))
		return e;
	if (dst_size < f.header)
		return STENOS_ERROR_DST_OVERFLOW;
	uint8_t* out = (uint8_t*)dst;
	if (bytes == 0 || ctx->level == 0) {
		// header only, or plain copies (stenos.cpp:431-433, 363-374): no codec involved, done in place
		const size_t need = f.header + f.nsb * 4 + bytes;
		if (dst_size < need)
			return STENOS_ERROR_DST_OVERFLOW;
		size_t off = write_frame_header(out, f.shift, bytes, f.sb);
		for (uint64_t s = 0; s < f.nsb; ++s)
			off += copy_superblock(out + off, (const uint8_t*)src + s * f.sb, superblock_bytes(bytes, f.sb, s));
		return off;
	}
	if (!ctx->device_ready())
		return STENOS_ERROR_INVALID_INSTRUCTION_SET;
	if (!needs_strategy(bytesoftype, ctx->level)) {
		const int lanes = lane_count(ctx, bytes);
		ctx->last_devices = 1;
		if (lanes > 1) {
			const size_t r = compress_lanes(ctx, (const uint8_t*)src, bytesoftype, bytes, out, dst_size, f, lanes);
			if (r != STENOS_ERROR_INVALID_PARAMETER) { // (that one: too few shareable superblocks, e.g. a tight dst_size)
				ctx->last_devices = lanes;
				return r;
			}
		}
		// page-locked caller memory: no staging on that side (both sides: no copy at all)
		void* a_src = device_alias(src, bytes);
		void* a_dst = device_alias(dst, dst_size);
		// (one side only and a large call: the chunked path below overlaps its upload, coding and download, which a single
		// pass with a blocking copy on the other side would not)
		if ((a_src && a_dst) || ((a_src || a_dst) && bytes < kHostChunkedFrom))
			return compress_staged(ctx, src, bytesoftype, bytes, dst, dst_size, f, a_src, a_dst);
		if (bytes >= kHostChunkedFrom) {
			bool no_thread = false;
			const size_t r = compress_chunked(ctx, (const uint8_t*)src, bytesoftype, bytes, out, dst_size, f, &no_thread);
			if (!no_thread)
				return r;
		}
	}
	return compress_staged(ctx, src, bytesoftype, bytes, dst, dst_size, f, nullptr, nullptr);
}

size_t decompress_host(stenos_context_s* ctx, const void* src, size_t bytesoftype, size_t size, void* dst, size_t dst_size)
{
	const uint8_t* in = (const uint8_t*)src;
	FrameInfo fi;
	size_t e = parse_frame(in, size, bytesoftype, dst_size, fi);
	if (is_err(e))
		return e;
	if (fi.total == 0)
		return 0;
	// walk the superblock chain on the host (stenos.cpp:1124-1143): cheap here, serial on a GPU
	std::vector<uint64_t> index(fi.nsb + 1);
	uint64_t p = fi.header;
	bool gpu_codes = false, host_codes = false;
	for (uint64_t s = 0; s < fi.nsb; ++s) {
		if (p + 4 > size)
			return STENOS_ERROR_SRC_OVERFLOW;
		index[s] = p;
		const unsigned code = in[p];
		const size_t csize = (size_t)get_le(in + p + 1, 3);
		if (p + 4 + csize > size)
			return STENOS_ERROR_INVALID_INPUT;
		if (code == 1)
			gpu_codes = true;
		else if (code >= 2 && code <= 5)
			host_codes = true;
		else if (code != 6)
			return STENOS_ERROR_INVALID_INPUT;
		p += 4 + csize;
	}
	index[fi.nsb] = p;
	uint8_t* out = (uint8_t*)dst;
	bool device_codes = gpu_codes;
	for (uint64_t s = 0; s < fi.nsb && !device_codes; ++s)
		device_codes = in[index[s]] >= 3 && in[index[s]] <= 5;
	if (!device_codes) { // copies and zstd-only superblocks: nothing for the GPU to do
		std::atomic<size_t> err(0);
		parallel_for(fi.nsb, [&](uint64_t s) {
			const uint64_t begin = s * (uint64_t)fi.sb;
			const size_t dsize = superblock_bytes(fi.total, fi.sb, s);
			const unsigned code = in[index[s]];
			const size_t csize = (size_t)get_le(in + index[s] + 1, 3);
			if (code == 6) {
				if (csize != dsize)
					err = STENOS_ERROR_INVALID_INPUT;
				else
					memcpy(out + begin, in + index[s] + 4, csize);
			}
			else if (code == 2) {
				if (!zstd().ok)
					err = STENOS_ERROR_ZSTD_INTERNAL;
				else if (zstd().is_error(zstd().decompress(out + begin, dsize, in + index[s] + 4, csize)))
					err = STENOS_ERROR_INVALID_INPUT;
			}
			else
				err = STENOS_ERROR_INVALID_INPUT;
		});
		if (err)
			return err;
		return (size_t)fi.total;
	}
	if (!ctx->device_ready())
		return STENOS_ERROR_INVALID_INSTRUCTION_SET;
	if (!host_codes) {
		const int lanes = lane_count(ctx, (size_t)fi.total);
		ctx->last_devices = 1;
		if (lanes > 1 && fi.nsb >= (uint64_t)(2 * lanes)) {
			ctx->last_devices = lanes;
			return decompress_lanes(ctx, in, bytesoftype, fi, index, out, lanes);
		}
		void* a_src = device_alias(src, size);
		void* a_dst = device_alias(dst, (size_t)fi.total);
		if ((a_src && a_dst) || ((a_src || a_dst) && fi.total < kHostChunkedFrom)) // (one side only and large: the chunked path overlaps)
			return decompress_staged(ctx, src, bytesoftype, size, dst, fi, index, a_src, a_dst);
		if (fi.total >= kHostChunkedFrom) {
			bool no_thread = false;
			const size_t r = decompress_chunked(ctx, in, bytesoftype, fi, index, out, 0, fi.nsb, &no_thread);
			if (!no_thread)
				return r;
		}
	}
	return decompress_staged(ctx, src, bytesoftype, size, dst, fi, index, nullptr, nullptr);
}

} // namespace stenos_host
