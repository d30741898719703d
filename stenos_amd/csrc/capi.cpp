// capi.cpp -- host side of libstenos.so: the frozen Stenos C ABI (include/stenos.h) and the
// device-pointer entry points (include/stenos_hip.h) on top of the gfx950 kernels of kernels.hip.
//
// What this file restates from the reference (stenos/internal/stenos.cpp): context and setters
// (:81-286), frame header and superblock sizing (:115-185, 862-874), the superblock strategy slice for
// levels 0/1 (:403-450, 606-615, 658-678), decode framing (:1052-1208), stenos_get_info (:1019-1050),
// the private single-superblock API (:768-842) and the timer wrappers (:1232-1257).  The per-chunk
// thread dispatcher (:909-1010, tiny_pool.h) is replaced by the GPU grid: `threads` is accepted and ignored.
//
// There is no CPU codec here.  If no HIP device is usable every codec call returns
// STENOS_ERROR_INVALID_INSTRUCTION_SET (the reference's code for "required instruction set missing").
#include <time.h>

#include <new>

#include "host.h"

using namespace stenos_host;

// =====================================================================================================
// exported C ABI
// =====================================================================================================
extern "C" {

stenos_context* stenos_make_context(void)
{
	void* m = malloc(sizeof(stenos_context_s));
	return m ? new (m) stenos_context_s() : nullptr;
}
void stenos_destroy_context(stenos_context* ctx)
{
	if (ctx) {
		ctx->~stenos_context_s();
		free(ctx);
	}
}
void stenos_reset_context(stenos_context* ctx) // stenos.cpp:245-252 (the custom block size is kept, as there)
{
	if (ctx) {
		ctx->level = 1;
		ctx->threads = 1;
		ctx->max_nanoseconds = 0;
	}
}
size_t stenos_set_level(stenos_context* ctx, int level)
{
	ctx->level = level > 9 ? 9 : (level < 0 ? 0 : level);
	return 0;
}
size_t stenos_set_threads(stenos_context* ctx, int threads)
{
	ctx->threads = threads < 1 ? 1 : threads;
	return 0;
}
size_t stenos_set_max_nanoseconds(stenos_context* ctx, uint64_t nanoseconds)
{
	ctx->max_nanoseconds = nanoseconds;
	return 0;
}
size_t stenos_set_block_size(stenos_context* ctx, size_t blocksize_shift)
{
	if (blocksize_shift >= 16 && blocksize_shift != STENOS_NO_BLOCK_SHIFT)
		return STENOS_ERROR_INVALID_PARAMETER;
	ctx->custom_shift = blocksize_shift;
	return 0;
}
size_t stenos_memory_footprint(stenos_context* ctx)
{
	// host bytes of the context; device buffers are reported by stenos_hip_workspace_bytes()
	(void)ctx;
	return sizeof(stenos_context_s);
}
int stenos_has_error(size_t r) { return r >= STENOS_LAST_ERROR_CODE; }
size_t stenos_bound(size_t bytes) { return stenos::compress_bound(bytes); }


size_t stenos_compress_generic(stenos_context* ctx, const void* src, size_t bytesoftype, size_t bytes, void* dst, size_t dst_size)
{
	return compress_host(ctx, src, bytesoftype, bytes, dst, dst_size);
}
size_t stenos_decompress_generic(stenos_context* ctx, const void* src, size_t bytesoftype, size_t size, void* dst, size_t dst_size)
{
	return decompress_host(ctx, src, bytesoftype, size, dst, dst_size);
}

// The reference builds a temporary context per call (stenos.cpp:1210-1226).  Here a context owns device buffers of about
// twice the input, so the one-shot calls of a thread share one context that lives as long as the thread: its buffers
// are kept between calls (and freed by the thread's exit).
static stenos_context_s& one_shot_context()
{
	static thread_local stenos_context_s ctx;
	ctx.threads = 1; // every parameter as a fresh context has it (the level is set by the caller)
	ctx.max_nanoseconds = 0;
	ctx.custom_shift = STENOS_NO_BLOCK_SHIFT;
	return ctx;
}
size_t stenos_compress(const void* src, size_t bytesoftype, size_t bytes, void* dst, size_t dst_size, int level)
{
	stenos_context_s& ctx = one_shot_context();
	ctx.level = level > 9 ? 9 : (level < 0 ? 0 : level);
	return stenos_compress_generic(&ctx, src, bytesoftype, bytes, dst, dst_size);
}
size_t stenos_decompress(const void* src, size_t bytesoftype, size_t bytes, void* dst, size_t dst_size)
{
	return stenos_decompress_generic(&one_shot_context(), src, bytesoftype, bytes, dst, dst_size);
}

size_t stenos_get_info(const void* src, size_t bytesoftype, size_t bytes, stenos_info* info) // stenos.cpp:1019-1050
{
	const uint8_t* in = (const uint8_t*)src;
	if (bytes < 8)
		return STENOS_ERROR_SRC_OVERFLOW;
	const unsigned shift = in[0];
	if (shift > 4 && shift != 255)
		return STENOS_ERROR_INVALID_INPUT;
	info->decompressed_size = (size_t)get_le(in + 1, 7);
	if (shift == 255) {
		if (bytes < 12)
			return STENOS_ERROR_SRC_OVERFLOW;
		info->superblock_size = (size_t)get_le(in + 8, 4);
		return 12;
	}
	info->superblock_size = base_superblock(bytesoftype * 256) << shift;
	return 8;
}

// ---- timer (stenos.cpp:1232-1257, timer.hpp:104-133) ----
struct stenos_timer_s {
	struct timespec t0;
};
stenos_timer* stenos_make_timer(void)
{
	stenos_timer* t = (stenos_timer*)malloc(sizeof(stenos_timer));
	if (t)
		clock_gettime(CLOCK_MONOTONIC, &t->t0);
	return t;
}
void stenos_destroy_timer(stenos_timer* timer) { free(timer); }
void stenos_tick(stenos_timer* timer) { clock_gettime(CLOCK_MONOTONIC, &timer->t0); }
uint64_t stenos_tock(stenos_timer* timer)
{
	struct timespec t1;
	clock_gettime(CLOCK_MONOTONIC, &t1);
	return (uint64_t)(t1.tv_sec - timer->t0.tv_sec) * 1000000000ull + (uint64_t)t1.tv_nsec - (uint64_t)timer->t0.tv_nsec;
}

// ---- private single-superblock API used by stenos::cvector (stenos.cpp:768-842) ----
size_t stenos_private_compress_block(stenos_context* ctx, const void* src, size_t bytesoftype, size_t super_block_size, size_t bytes, void* dst,
				     size_t dst_size)
{
	if (dst_size < 4) // stenos.cpp:427-429
		return STENOS_ERROR_DST_OVERFLOW;
	if (bytesoftype == 0 || bytesoftype >= STENOS_MAX_BYTESOFTYPE)
		return STENOS_ERROR_INVALID_BYTESOFTYPE;
	if (bytes == 0 || ctx->level == 0) // MEMCPY (stenos.cpp:431-433)
		return dst_size < bytes + 4 ? (size_t)STENOS_ERROR_DST_OVERFLOW : copy_superblock((uint8_t*)dst, src, bytes);
	size_t e = check_supported(ctx, bytesoftype, ctx->level);
	if (is_err(e))
		return e;
	if (!ctx->device_ready())
		return STENOS_ERROR_INVALID_INSTRUCTION_SET;
	if (bytes > super_block_size || super_block_size >= STENOS_MAX_BLOCK_BYTES)
		return STENOS_ERROR_INVALID_PARAMETER;
	FramePlan f;
	f.sb = super_block_size;
	f.nsb = 1;
	f.nfull = bytes / (bytesoftype * 256);
	f.tail = (uint32_t)(bytes % (bytesoftype * 256));
	f.bps = (uint32_t)(super_block_size / (bytesoftype * 256));
	if (f.bps == 0)
		return STENOS_ERROR_INVALID_PARAMETER;
	if (!ctx->in.ensure(bytes + 64) || !ctx->out.ensure(bytes + 64))
		return STENOS_ERROR_ALLOC;
	if (hipMemcpy(ctx->in.p, src, bytes, hipMemcpyHostToDevice) != hipSuccess)
		return STENOS_ERROR_UNDEFINED;
	if (needs_strategy(bytesoftype, ctx->level)) {
		// levels >= 2 and bytesoftype 1 (stenos::cvector<char>, cvector at higher levels): the strategy layer on this one
		// superblock, as a frame of one superblock whose 8-byte header is dropped; the superblock sees the caller's capacity
		f.header = 8;
		f.shift = 0;
		HostBuf& tmp = ctx->h_out;
		if (!tmp.ensure(dst_size + 8 + 64))
			return STENOS_ERROR_ALLOC;
		const size_t r = compress_strategy(ctx, (const uint8_t*)src, ctx->in.as<uint8_t>(), bytesoftype, bytes, tmp.data(), dst_size + 8, ctx->level, f, nullptr);
		if (is_err(r))
			return r;
		memcpy(dst, tmp.data() + 8, r - 8);
		return r - 8;
	}
	e = enqueue_compress(ctx, ctx->in.as<uint8_t>(), bytesoftype, bytes, ctx->out.as<uint8_t>(), dst_size, ctx->level, f, false, nullptr);
	if (is_err(e))
		return e;
	ctx->set_job(1, nullptr, false, dst_size);
	size_t r = finish_job(ctx);
	if (is_err(r))
		return r;
	if (r > dst_size)
		return STENOS_ERROR_DST_OVERFLOW;
	if (hipMemcpy(dst, ctx->out.p, r, hipMemcpyDeviceToHost) != hipSuccess)
		return STENOS_ERROR_UNDEFINED;
	return r;
}

size_t stenos_private_decompress_block(stenos_context* ctx, const void* src, size_t bytesoftype, size_t super_block_size, size_t bytes, void* dst,
				       size_t dst_size)
{
	const uint8_t* in = (const uint8_t*)src;
	if (bytes < 4) // stenos.cpp:792-793
		return STENOS_ERROR_SRC_OVERFLOW;
	if (bytesoftype == 0 || bytesoftype >= STENOS_MAX_BYTESOFTYPE)
		return STENOS_ERROR_INVALID_BYTESOFTYPE;
	const unsigned code = in[0];
	const size_t csize = (size_t)get_le(in + 1, 3);
	if (4 + csize > bytes)
		return STENOS_ERROR_INVALID_INPUT;
	if (code == 6) {
		if (csize != dst_size)
			return STENOS_ERROR_INVALID_INPUT;
		memcpy(dst, in + 4, csize);
		return dst_size;
	}
	if (code == 2) {
		if (!zstd().ok)
			return STENOS_ERROR_ZSTD_INTERNAL;
		size_t r = zstd().decompress(dst, dst_size, in + 4, csize);
		return zstd().is_error(r) ? STENOS_ERROR_INVALID_INPUT : dst_size;
	}
	if (code >= 3 && code <= 5) {
		// transposed / transposed + delta / block codec output, each under zstd (decompress_generic_superblock, stenos.cpp:700-740):
		// the same machinery as for frames, given this superblock as a frame of one superblock of a custom size
		if (dst_size == 0 || dst_size > super_block_size || super_block_size < bytesoftype * 256 || super_block_size >= STENOS_MAX_BLOCK_BYTES)
			return STENOS_ERROR_INVALID_INPUT;
		std::vector<uint8_t> frame(12 + 4 + csize);
		write_frame_header(frame.data(), 255, dst_size, super_block_size);
		memcpy(frame.data() + 12, in, 4 + csize);
		return stenos_decompress_generic(ctx, frame.data(), bytesoftype, frame.size(), dst, dst_size);
	}
	if (code != 1)
		return STENOS_ERROR_INVALID_INPUT;
	if (dst_size == 0)
		return 0;
	if (!ctx->device_ready())
		return STENOS_ERROR_INVALID_INSTRUCTION_SET;
	ctx->last_frames = 0; // (the index workspace takes this superblock's offsets)
	if (!ctx->in.ensure(4 + csize + 64) || !ctx->out.ensure(dst_size + 64) || !ctx->sboff.ensure(32) || !ctx->misc.ensure(4096))
		return STENOS_ERROR_ALLOC;
	const uint64_t index[2] = { 0, 4 + csize };
	if (hipMemcpy(ctx->in.p, src, 4 + csize, hipMemcpyHostToDevice) != hipSuccess ||
	    hipMemcpy(ctx->sboff.p, index, sizeof(index), hipMemcpyHostToDevice) != hipSuccess)
		return STENOS_ERROR_UNDEFINED;
	uint32_t* d_status = &ctx->words()->decode_status;
	if (hipMemsetAsync(d_status, 0, 4, nullptr) != hipSuccess)
		return STENOS_ERROR_UNDEFINED;
	DecodeArgs a;
	if (!decode_args(ctx, ctx->in.p, 4 + csize, ctx->sboff.as<uint64_t>(), ctx->out.p, dst_size, 1, dst_size, bytesoftype, d_status, a))
		return STENOS_ERROR_ALLOC;
	if (stenos_k_launch_decode(a, nullptr) != hipSuccess)
		return STENOS_ERROR_UNDEFINED;
	uint32_t status = 0;
	if (hipMemcpy(&status, d_status, 4, hipMemcpyDeviceToHost) != hipSuccess)
		return STENOS_ERROR_UNDEFINED;
	if (status)
		return STENOS_ERROR_INVALID_INPUT;
	if (hipMemcpy(dst, ctx->out.p, dst_size, hipMemcpyDeviceToHost) != hipSuccess)
		return STENOS_ERROR_UNDEFINED;
	return dst_size;
}

size_t stenos_private_block_size(const void* src, size_t src_size)
{
	if (src_size < 4)
		return STENOS_ERROR_SRC_OVERFLOW;
	return (size_t)get_le((const uint8_t*)src + 1, 3) + 4;
}
size_t stenos_private_block_csize(const void* src)
{
	if (!src)
		return 0;
	return (size_t)get_le((const uint8_t*)src + 1, 3) + 4;
}
size_t stenos_private_create_compression_header(size_t decompressed_size, size_t super_block_size, void* dst, size_t dst_size)
{
	if (dst_size < 12)
		return STENOS_ERROR_DST_OVERFLOW;
	return write_frame_header((uint8_t*)dst, 255, decompressed_size, super_block_size);
}

// =====================================================================================================
// device-pointer entry points (include/stenos_hip.h)
// =====================================================================================================

int stenos_hip_last_devices(stenos_context* ctx) { return ctx ? ctx->last_devices : 0; }
void stenos_hip_set_devices(stenos_context* ctx, int devices)
{
	if (ctx)
		ctx->hip_devices = devices > 0 ? devices : 0;
}
int stenos_hip_stage_ms(stenos_context* ctx, double* out, int n, int reset)
{
	if (!ctx)
		return 0;
	const int k = n < (int)STAGE_COUNT ? n : (int)STAGE_COUNT;
	for (int i = 0; i < k && out; ++i)
		out[i] = ctx->stage_ms[i];
	if (reset)
		for (double& v : ctx->stage_ms)
			v = 0;
	return (int)STAGE_COUNT;
}
int stenos_hip_fused_fallbacks(stenos_context* ctx) { return ctx ? ctx->fused_fallbacks : 0; }
#ifdef STENOS_TEST_HOOKS // (the test suite's own build only: tests/hooks/Makefile)
int stenos_hip_test_walk(stenos_context* ctx, int serial)
{
	if (!ctx)
		return -1;
	int fell_back = -1; // the flag word the last parallel walk left in its scratch (walk_kernels.hip): 1 = the serial walk ran after all
	uint32_t flags = 0;
	if (!ctx->test_serial_walk && ctx->walk.p && ctx->device_ready() && hipDeviceSynchronize() == hipSuccess &&
	    hipMemcpy(&flags, ctx->walk.p, 4, hipMemcpyDeviceToHost) == hipSuccess)
		fell_back = flags != 0;
	ctx->test_serial_walk = serial != 0;
	return fell_back;
}
void stenos_hip_test_lanes(stenos_context* ctx, int share_current_device, int fail_lane)
{
	if (!ctx)
		return;
	ctx->test_lanes_share_device = share_current_device != 0;
	ctx->test_fail_lane = fail_lane;
}
void stenos_hip_test_fused_timeouts(stenos_context* ctx, int n)
{
	if (ctx && n > 0)
		ctx->inject_chain_timeout = n;
	if (ctx && n < 0 && n >= -3) // (the choice of fused kernel rides on this switch: the set of test switches is fixed, tests/test_abi_cpu.py)
		ctx->test_fused_variant = -n - 1;
}
#endif
int stenos_hip_device_count(void)
{
	int n = 0;
	return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

size_t stenos_hip_workspace_bytes(size_t bytesoftype, size_t bytes)
{
	if (bytesoftype == 0 || bytesoftype > kMaxT)
		return 0;
	const size_t bs = bytesoftype * 256;
	const size_t sb = base_superblock(bs);
	const size_t nblocks = bytes / bs + 2;
	const size_t nsb = bytes / sb + 2;
	const uint32_t T = (uint32_t)bytesoftype;
	// the arena: staging buffers of the fused encoder (two per resident workgroup, whatever the input size) plus the slots of
	// the last superblocks or, where that kernel does not apply, one padded slot per block; then 12 bytes of tables per block
	// and 37 per superblock (default superblock size).  (A destination below stenos_bound() sends every block through slots.)
	const size_t arena = stenos_k_fused_supported(T) ? fused_stage_bytes_any(T, (uint32_t)(sb / bs), nsb) + 2 * (sb / bs + 1) * stenos_k_slot_stride(T)
							 : nblocks * (size_t)stenos_k_slot_stride(T);
	const size_t wide = (size_t)wide_scratch_bytes(T, nblocks); // bytesoftype above 64: the scratch of kernels_wide.hip
	return arena + wide + nblocks * 16 + nsb * 37 + 4096;
}

size_t stenos_hip_compress(stenos_context* ctx, const void* d_src, size_t bytesoftype, size_t bytes, void* d_dst, size_t dst_size, void* stream)
{
	return compress_device(ctx, d_src, bytesoftype, bytes, d_dst, dst_size, (hipStream_t)stream, true);
}
size_t stenos_hip_compress_async(stenos_context* ctx, const void* d_src, size_t bytesoftype, size_t bytes, void* d_dst, size_t dst_size, void* stream)
{
	return compress_device(ctx, d_src, bytesoftype, bytes, d_dst, dst_size, (hipStream_t)stream, false);
}

size_t stenos_hip_finish(stenos_context* ctx)
{
	size_t r = finish_job(ctx);
	// frames with zstd-based superblocks need the synchronous call, which finishes them on the host
	return (!is_err(r) && ctx->job_host_codes) ? STENOS_ERROR_ZSTD_INTERNAL : r;
}

static size_t byte_kernel(hipError_t e) { return e == hipSuccess ? 0 : STENOS_ERROR_UNDEFINED; }
size_t stenos_hip_shuffle(const void* d_src, size_t bytesoftype, size_t bytes, void* d_dst, void* stream)
{
	if (bytesoftype == 0 || bytesoftype >= STENOS_MAX_BYTESOFTYPE)
		return STENOS_ERROR_INVALID_BYTESOFTYPE;
	return byte_kernel(stenos_k_launch_shuffle((const uint8_t*)d_src, (uint8_t*)d_dst, (uint32_t)bytesoftype, bytes, false, (hipStream_t)stream));
}
size_t stenos_hip_unshuffle(const void* d_src, size_t bytesoftype, size_t bytes, void* d_dst, void* stream)
{
	if (bytesoftype == 0 || bytesoftype >= STENOS_MAX_BYTESOFTYPE)
		return STENOS_ERROR_INVALID_BYTESOFTYPE;
	return byte_kernel(stenos_k_launch_shuffle((const uint8_t*)d_src, (uint8_t*)d_dst, (uint32_t)bytesoftype, bytes, true, (hipStream_t)stream));
}
size_t stenos_hip_delta(const void* d_src, void* d_dst, size_t bytes, void* stream)
{
	return byte_kernel(stenos_k_launch_delta((const uint8_t*)d_src, (uint8_t*)d_dst, bytes, false, (hipStream_t)stream));
}
size_t stenos_hip_delta_inv(const void* d_src, void* d_dst, size_t bytes, void* stream)
{
	return byte_kernel(stenos_k_launch_delta((const uint8_t*)d_src, (uint8_t*)d_dst, bytes, true, (hipStream_t)stream));
}

void stenos_hip_set_profiling(stenos_context* ctx, int enabled) { ctx->profiling = enabled != 0; }
double stenos_hip_kernel_ms(stenos_context* ctx, int which)
{
	if (which < 0 || which > 1 || !ctx->ev_valid[which])
		return -1.0;
	float ms = 0.f;
	if (hipEventSynchronize(ctx->ev[2 * which + 1]) != hipSuccess || hipEventElapsedTime(&ms, ctx->ev[2 * which], ctx->ev[2 * which + 1]) != hipSuccess)
		return -1.0;
	return (double)ms;
}

const uint64_t* stenos_hip_last_index(stenos_context* ctx, size_t* nsb)
{
	if (nsb)
		*nsb = ctx->last_batch ? 0 : ctx->last_nsb;
	return ctx->last_batch ? nullptr : ctx->sboff.as<uint64_t>();
}

const uint64_t* stenos_hip_frame_index(stenos_context* ctx, const void* d_src, size_t bytesoftype, size_t bytes, size_t* nsb, void* stream)
{
	return frame_index(ctx, d_src, bytesoftype, bytes, nsb, (hipStream_t)stream);
}

size_t stenos_hip_compress_batch(stenos_context* ctx, size_t n, size_t bytesoftype, const void* const* d_srcs, const size_t* bytes, void* const* d_dsts,
				 const size_t* dst_sizes, size_t* results, void* stream)
{
	if (n == 0)
		return 0;
	if (!ctx || !d_srcs || !bytes || !d_dsts || !dst_sizes || !results)
		return STENOS_ERROR_INVALID_PARAMETER;
	if (!ctx->device_ready())
		return STENOS_ERROR_INVALID_INSTRUCTION_SET;
	return compress_batch(ctx, n, bytesoftype, d_srcs, bytes, d_dsts, dst_sizes, results, (hipStream_t)stream);
}
size_t stenos_hip_decompress_batch(stenos_context* ctx, size_t n, size_t bytesoftype, const void* const* d_srcs, const size_t* src_sizes, void* const* d_dsts,
				   const size_t* dst_sizes, size_t* results, void* stream)
{
	if (n == 0)
		return 0;
	if (!ctx || !d_srcs || !src_sizes || !d_dsts || !dst_sizes || !results)
		return STENOS_ERROR_INVALID_PARAMETER;
	if (!ctx->device_ready())
		return STENOS_ERROR_INVALID_INSTRUCTION_SET;
	return decompress_batch(ctx, n, bytesoftype, d_srcs, src_sizes, d_dsts, dst_sizes, results, (hipStream_t)stream);
}
size_t stenos_hip_decompress_ranges(stenos_context* ctx, const void* d_src, size_t bytesoftype, size_t bytes, size_t n, const uint64_t* offsets,
				    const uint64_t* lengths, void* const* d_dsts, const uint64_t* d_index, void* stream)
{
	if (n == 0)
		return 0;
	if (!ctx || !d_src || !offsets || !lengths || !d_dsts)
		return STENOS_ERROR_INVALID_PARAMETER;
	if (!ctx->device_ready())
		return STENOS_ERROR_INVALID_INSTRUCTION_SET;
	return decompress_ranges(ctx, d_src, bytesoftype, bytes, n, offsets, lengths, d_dsts, d_index, (hipStream_t)stream);
}
size_t stenos_hip_gather_rows(stenos_context* ctx, const void* d_src, size_t bytesoftype, size_t bytes, size_t row_bytes, size_t n, const uint64_t* d_rows,
			      void* d_dst, size_t dst_stride, const uint64_t* d_index, void* stream)
{
	if (n == 0)
		return 0;
	if (!ctx || !d_src || !d_rows || !d_dst)
		return STENOS_ERROR_INVALID_PARAMETER;
	// what needs no device to be refused: the shape of the call (n * row_bytes and the end of the last slot must be representable)
	if (row_bytes == 0 || dst_stride < row_bytes || bytesoftype == 0 || bytesoftype > STENOS_K_LDS_MAX_T || n > ~(size_t)0 / row_bytes ||
	    n - 1 > (~(size_t)0 - row_bytes) / dst_stride)
		return STENOS_ERROR_INVALID_PARAMETER;
	if (!ctx->device_ready())
		return STENOS_ERROR_INVALID_INSTRUCTION_SET;
	return gather_rows(ctx, d_src, bytesoftype, bytes, row_bytes, n, d_rows, d_dst, dst_stride, d_index, (hipStream_t)stream);
}
size_t stenos_hip_gather_ranges(stenos_context* ctx, const void* d_src, size_t bytesoftype, size_t bytes, size_t n, const uint64_t* d_offsets, const uint64_t* d_lengths,
				void* d_dst, size_t dst_size, uint64_t* d_dst_offsets, const uint64_t* d_index, void* stream)
{
	if (n == 0)
		return 0;
	if (!ctx || !d_src || !d_offsets || !d_lengths || (!d_dst && dst_size))
		return STENOS_ERROR_INVALID_PARAMETER;
	// what needs no device to be refused: the bytesoftype, and so many ranges that two pieces each pass 2^31 - 1
	if (bytesoftype == 0 || bytesoftype > STENOS_K_LDS_MAX_T || n > 0x7FFFFFFFull / 2)
		return STENOS_ERROR_INVALID_PARAMETER;
	if (!ctx->device_ready())
		return STENOS_ERROR_INVALID_INSTRUCTION_SET;
	return gather_ranges(ctx, d_src, bytesoftype, bytes, n, d_offsets, d_lengths, d_dst, dst_size, d_dst_offsets, d_index, (hipStream_t)stream);
}
size_t stenos_hip_gather_rows_batch(stenos_context* ctx, size_t m, size_t bytesoftype, const void* const* d_frames, const size_t* sizes, size_t row_bytes, size_t n,
				    const uint64_t* d_frame_ids, const uint64_t* d_rows, void* d_dst, size_t dst_stride, const uint64_t* d_index, void* stream)
{
	if (n == 0)
		return 0;
	if (!ctx || !d_frames || !sizes || !d_frame_ids || !d_rows || !d_dst)
		return STENOS_ERROR_INVALID_PARAMETER;
	// what needs no device to be refused: no frame, more frames than one thread each, the shape of the call (stenos_hip_gather_rows)
	if (m == 0 || m > 0x7FFFFFFFull || row_bytes == 0 || dst_stride < row_bytes || bytesoftype == 0 || bytesoftype > STENOS_K_LDS_MAX_T || n > ~(size_t)0 / row_bytes ||
	    n - 1 > (~(size_t)0 - row_bytes) / dst_stride)
		return STENOS_ERROR_INVALID_PARAMETER;
	if (!ctx->device_ready())
		return STENOS_ERROR_INVALID_INSTRUCTION_SET;
	return gather_rows_batch(ctx, m, bytesoftype, d_frames, sizes, row_bytes, n, d_frame_ids, d_rows, d_dst, dst_stride, d_index, (hipStream_t)stream);
}
const uint64_t* stenos_hip_frames_index(stenos_context* ctx, size_t m, size_t bytesoftype, const void* const* d_frames, const size_t* sizes, size_t* entries, void* stream)
{
	return frames_index(ctx, m, bytesoftype, d_frames, sizes, entries, (hipStream_t)stream);
}
size_t stenos_hip_update_rows(stenos_context* ctx, const void* d_frame, size_t bytesoftype, size_t bytes, size_t row_bytes, size_t n, const uint64_t* d_rows,
			      const void* d_src, size_t src_stride, void* d_out, size_t out_size, const uint64_t* d_index, void* stream)
{
	if (!ctx || !d_frame || !d_out || (n && (!d_rows || !d_src)))
		return STENOS_ERROR_INVALID_PARAMETER;
	// what needs no device to be refused: the shape of the call, and what the context could not compress the touched superblocks with
	if (row_bytes == 0 || src_stride < row_bytes || bytesoftype == 0 || bytesoftype > STENOS_K_LDS_MAX_T ||
	    (n && (n > ~(size_t)0 / row_bytes || n - 1 > (~(size_t)0 - row_bytes) / src_stride)) || needs_strategy(bytesoftype, ctx->level) || ctx->max_nanoseconds)
		return STENOS_ERROR_INVALID_PARAMETER;
	if (!ctx->device_ready())
		return STENOS_ERROR_INVALID_INSTRUCTION_SET;
	return update_rows(ctx, d_frame, bytesoftype, bytes, row_bytes, n, d_rows, d_src, src_stride, d_out, out_size, d_index, (hipStream_t)stream);
}
size_t stenos_hip_update_rows_batch(stenos_context* ctx, size_t m, size_t bytesoftype, const void* const* d_frames, const size_t* sizes, size_t row_bytes, size_t n,
				    const uint64_t* d_frame_ids, const uint64_t* d_rows, const void* d_src, size_t src_stride, void* const* d_outs, const size_t* out_sizes,
				    size_t* results, const uint64_t* d_index, void* stream)
{
	if (!ctx || !d_frames || !sizes || !d_outs || !out_sizes || !results || (n && (!d_frame_ids || !d_rows || !d_src)))
		return STENOS_ERROR_INVALID_PARAMETER;
	// what needs no device to be refused: no frame, more frames than one thread each, the shape of the call and what the context
	// could not compress the touched superblocks with (stenos_hip_update_rows), a NULL among the frames or the outputs
	if (m == 0 || m > 0x7FFFFFFFull || row_bytes == 0 || src_stride < row_bytes || bytesoftype == 0 || bytesoftype > STENOS_K_LDS_MAX_T ||
	    (n && (n > ~(size_t)0 / row_bytes || n - 1 > (~(size_t)0 - row_bytes) / src_stride)) || needs_strategy(bytesoftype, ctx->level) || ctx->max_nanoseconds)
		return STENOS_ERROR_INVALID_PARAMETER;
	for (size_t f = 0; f < m; ++f)
		if (!d_frames[f] || !d_outs[f])
			return STENOS_ERROR_INVALID_PARAMETER;
	if (!ctx->device_ready())
		return STENOS_ERROR_INVALID_INSTRUCTION_SET;
	return update_rows_batch(ctx, m, bytesoftype, d_frames, sizes, row_bytes, n, d_frame_ids, d_rows, d_src, src_stride, d_outs, out_sizes, results, d_index,
				 (hipStream_t)stream);
}
size_t stenos_hip_append(stenos_context* ctx, void* d_frame, size_t bytesoftype, size_t bytes, size_t capacity, const void* d_src, size_t src_bytes,
			 const uint64_t* d_index, void* stream)
{
	if (!ctx || !d_frame || (src_bytes && !d_src))
		return STENOS_ERROR_INVALID_PARAMETER;
	// what needs no device to be refused: the buffer's shape, a size the header cannot hold, and what the context could not
	// compress the new superblocks with
	if (capacity < bytes || bytesoftype == 0 || bytesoftype > STENOS_K_LDS_MAX_T || (uint64_t)src_bytes >> 56 || needs_strategy(bytesoftype, ctx->level) ||
	    ctx->level < 0 || ctx->max_nanoseconds)
		return STENOS_ERROR_INVALID_PARAMETER;
	if (!ctx->device_ready())
		return STENOS_ERROR_INVALID_INSTRUCTION_SET;
	return append(ctx, d_frame, bytesoftype, bytes, capacity, d_src, src_bytes, d_index, (hipStream_t)stream);
}
size_t stenos_hip_append_batch(stenos_context* ctx, size_t m, size_t bytesoftype, void* const* d_frames, const size_t* sizes, const size_t* capacities,
			       const void* const* d_srcs, const size_t* src_sizes, size_t* results, const uint64_t* d_index, void* stream)
{
	if (!ctx)
		return STENOS_ERROR_INVALID_PARAMETER;
	ctx->last_frames = 0; // (a call that fails leaves no many-frame index)
	if (!d_frames || !sizes || !capacities || !d_srcs || !src_sizes || !results)
		return STENOS_ERROR_INVALID_PARAMETER;
	// what needs no device to be refused: no frame, more frames than one thread each, what stenos_hip_append refuses of every frame
	// (the buffer's shape, a size the header cannot hold, a NULL), and what the context could not compress the new superblocks with
	if (m == 0 || m > 0x7FFFFFFFull || bytesoftype == 0 || bytesoftype > STENOS_K_LDS_MAX_T || needs_strategy(bytesoftype, ctx->level) || ctx->level < 0 ||
	    ctx->max_nanoseconds)
		return STENOS_ERROR_INVALID_PARAMETER;
	for (size_t f = 0; f < m; ++f)
		if (!d_frames[f] || capacities[f] < sizes[f] || (uint64_t)src_sizes[f] >> 56 || (src_sizes[f] && !d_srcs[f]))
			return STENOS_ERROR_INVALID_PARAMETER;
	if (append_batch_overlap(m, d_frames, capacities, d_srcs, src_sizes))
		return STENOS_ERROR_INVALID_PARAMETER;
	if (!ctx->device_ready())
		return STENOS_ERROR_INVALID_INSTRUCTION_SET;
	return append_batch(ctx, m, bytesoftype, d_frames, sizes, capacities, d_srcs, src_sizes, results, d_index, (hipStream_t)stream);
}
const uint64_t* stenos_hip_last_frames_index(stenos_context* ctx, size_t* entries)
{
	const size_t have = ctx && ctx->last_batch ? ctx->last_frames : 0;
	if (entries)
		*entries = have;
	return have ? ctx->sboff.as<uint64_t>() : nullptr;
}
size_t stenos_hip_batch_workspace_bytes(size_t bytesoftype, size_t n, const size_t* bytes)
{
	if (bytesoftype == 0 || bytesoftype > STENOS_K_LDS_MAX_T || (n && !bytes))
		return 0;
	// one padded slot and 16 bytes of tables per block, 21 bytes of tables per superblock, the item tables (compress_batch)
	const size_t bs = bytesoftype * 256, sb = base_superblock(bs), stride = stenos_k_slot_stride((uint32_t)bytesoftype);
	size_t blocks = 0, sbs = 0;
	for (size_t i = 0; i < n; ++i) {
		blocks += bytes[i] / bs + (bytes[i] % bs ? 1 : 0);
		sbs += bytes[i] / sb + (bytes[i] % sb ? 1 : 0);
	}
	return blocks * (stride + 16) + sbs * 21 + n * (sizeof(codec::FrameJob) + 8 * 3 + sizeof(BatchItemState) + sizeof(BatchTinyIn) + sizeof(BatchTinyOut) + 4) + 4096;
}

size_t stenos_hip_decompress(stenos_context* ctx, const void* d_src, size_t bytesoftype, size_t bytes, void* d_dst, size_t dst_size,
			     const uint64_t* d_index, void* stream)
{
	return decompress_device(ctx, d_src, bytesoftype, bytes, d_dst, dst_size, d_index, nullptr, nullptr, (hipStream_t)stream, true);
}
size_t stenos_hip_decompress_async(stenos_context* ctx, const void* d_src, size_t bytesoftype, size_t bytes, void* d_dst, size_t dst_size,
				   const uint64_t* d_index, void* stream)
{
	return decompress_device(ctx, d_src, bytesoftype, bytes, d_dst, dst_size, d_index, nullptr, nullptr, (hipStream_t)stream, false);
}

} // extern "C"
