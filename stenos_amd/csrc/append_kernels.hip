// append_kernels.hip -- gfx950 kernels behind stenos_hip_append (append.h):
//   append_plan         the index entries the call uses, the code byte of the partial last superblock, p for the host
//   append_decode       one wavefront: the partial last superblock, whole -> the stitch buffer
//   append_commit_plan  one thread per new superblock: the new index entries, the streams' bytes and the new total
//   append_commit       the encoded streams to their place behind p, the size field of the header: the only writes to the frame
// What a thread or a wavefront of each does is in append_codec.h (the host emulation runs the same text).
// Compiled with the decoder's options (csrc/Makefile, decode_kernels.hip): append_decode has no divergent branch.
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "append.h"
#include "decode_body.h"
#include "append_codec.h"

using namespace codec;
using namespace wv;

static_assert(UPDATE_ST_TRUNCATED == DECODE_STATUS_TRUNCATED && UPDATE_ST_INVALID == DECODE_STATUS_INVALID && UPDATE_ST_HOST_CODES == DECODE_STATUS_HOST_CODES,
	      "update_codec.h");

namespace {

extern __shared__ __attribute__((aligned(16))) uint8_t g_lds[];

__global__ __launch_bounds__(64) void append_plan(AppendArgs a)
{
	if (threadIdx.x == 0)
		append_plan_thread(a);
}

// Waves per SIMD, as decode_superblocks (decode_kernels.hip).
#ifndef STENOS_DECODE_OCCUPANCY_T8
#define STENOS_DECODE_OCCUPANCY_T8 8
#endif
constexpr uint32_t append_decode_occupancy(uint32_t TT) { return TT == 8 ? STENOS_DECODE_OCCUPANCY_T8 : 8; }

// Superblock `keep` of the old frame, whole, to raw: the one copy of the header checks and the code 1 / 6 dispatch that
// decode_frames_batch uses (decode_body.h), given a destination base that puts the superblock at raw.  A zstd-based code only
// sets DECODE_STATUS_HOST_CODES again: append_plan has flagged it for the host.
template <uint32_t TT>
__global__ __launch_bounds__(64, append_decode_occupancy(TT)) void append_decode(AppendArgs a, uint8_t* raw, uint64_t total, uint32_t sb, uint32_t T)
{
	DecodeArgs d = DecodeArgs();
	d.frame = a.frame;
	d.size = a.size;
	d.sb_off = a.idx;
	d.dst = (uint8_t*)((uintptr_t)raw - (uint64_t)a.keep * sb); // (+ keep * sb: raw)
	d.total_bytes = total;
	d.nsb = (uint64_t)a.keep + 1;
	d.sb_bytes = sb;
	d.T = T;
	d.status = a.words + APPEND_W_STATUS;
	decode_superblock_entry<TT>(g_lds, d, a.keep);
}

__global__ __launch_bounds__(APPEND_PLAN_THREADS) void append_commit_plan(AppendArgs a)
{
	const uint64_t j = (uint64_t)blockIdx.x * APPEND_PLAN_THREADS + threadIdx.x;
	const uint32_t st = j < a.k ? append_commit_plan_thread(a, (uint32_t)j) : 0u;
	if (st)
		atomicOr(a.words + APPEND_W_STATUS, st);
}

__global__ __launch_bounds__(64 * APPEND_COMMIT_WAVES) void append_commit(AppendArgs a)
{
	const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
	append_commit_wave(a, (uint64_t)blockIdx.x * APPEND_COMMIT_WAVES + w);
}

} // namespace

hipError_t stenos_a_launch_plan(const AppendArgs& a, hipStream_t stream)
{
	hipLaunchKernelGGL(append_plan, dim3(1), dim3(64), 0, stream, a);
	return hipGetLastError();
}

hipError_t stenos_a_launch_decode(const AppendArgs& a, uint8_t* raw, uint64_t total, uint32_t sb, uint32_t T, hipStream_t stream)
{
	if (a.r == 0)
		return hipSuccess;
	if (T == 0 || T > STENOS_K_LDS_MAX_T)
		return hipErrorInvalidValue;
	return stenos_k_decode_variant(T, [&](auto tt) { return stenos_k_launch_decoder(append_decode<decltype(tt)::value>, 1u, T, stream, a, raw, total, sb, T); });
}

hipError_t stenos_a_launch_commit_plan(const AppendArgs& a, hipStream_t stream)
{
	if (a.k == 0)
		return hipErrorInvalidValue;
	hipLaunchKernelGGL(append_commit_plan, dim3((a.k + APPEND_PLAN_THREADS - 1) / APPEND_PLAN_THREADS), dim3(APPEND_PLAN_THREADS), 0, stream, a);
	return hipGetLastError();
}

hipError_t stenos_a_launch_commit(const AppendArgs& a, uint64_t len0, uint64_t len1, hipStream_t stream)
{
	const uint64_t chunk = APPEND_COMMIT_CHUNK, waves = (len0 + chunk - 1) / chunk + (len1 + chunk - 1) / chunk; // (append_commit_chunks)
	const uint64_t groups = (waves + APPEND_COMMIT_WAVES - 1) / APPEND_COMMIT_WAVES;
	if (groups == 0 || groups > 0x7FFFFFFFull)
		return hipErrorInvalidValue;
	hipLaunchKernelGGL(append_commit, dim3((uint32_t)groups), dim3(64 * APPEND_COMMIT_WAVES), 0, stream, a);
	return hipGetLastError();
}
