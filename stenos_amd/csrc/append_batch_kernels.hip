// append_batch_kernels.hip -- gfx950 kernels behind stenos_hip_append_batch (append_batch.h):
//   append_batch_plan         one thread per frame: the index entries the frame uses, the code byte of its partial last
//                             superblock, p_f; flags of zstd-based codes and the ends of untouched chains for the host
//   append_batch_decode       one wavefront per frame with a partial last superblock: that superblock, whole -> its stitch slot
//   append_batch_stitch       the head of every B_f behind the decoded bytes
//   append_batch_commit_plan  one thread per new superblock of all frames: the new index entries, per frame the streams' bytes
//                             and the new total
//   append_batch_index        one thread per old index entry that moves to the new layout
//   append_batch_commit       the encoded streams to their places, the size fields: the only writes to the frames
// What a thread or a wavefront of each does is in append_batch_codec.h (the host emulation, tests/emul_append_batch, runs the
// same text).  Compiled with the decoder's options (csrc/Makefile, decode_kernels.hip): append_batch_decode has no divergent branch.
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "batch.h"
#include "append_batch.h"
#include "decode_body.h"
#include "append_batch_codec.h"

using namespace codec;
using namespace wv;

static_assert(UPDATE_ST_TRUNCATED == DECODE_STATUS_TRUNCATED && UPDATE_ST_INVALID == DECODE_STATUS_INVALID && UPDATE_ST_HOST_CODES == DECODE_STATUS_HOST_CODES,
	      "update_codec.h");

namespace {

extern __shared__ __attribute__((aligned(16))) uint8_t g_lds[];

__global__ __launch_bounds__(APPEND_PLAN_THREADS) void append_batch_plan(AppendBatchArgs a)
{
	const uint64_t f = (uint64_t)blockIdx.x * APPEND_PLAN_THREADS + threadIdx.x;
	const uint32_t st = f < a.m ? append_batch_plan_thread(a, (uint32_t)f) : 0u;
	if (st)
		atomicOr(a.words + APPEND_W_STATUS, st);
}

// The frame's entry comes out of memory, and a pointer loaded as a plain one is a flat pointer: what is loaded through it may be
// private to a lane, so the compiler would take everything read from the frame for divergent (update_batch_kernels.hip,
// GlobalUpdateFrame).  The table is read as what it is: AppendBatchFrame with pointers into global memory.
#define GLOBAL __attribute__((address_space(1)))
struct GlobalAppendFrame {
	const GLOBAL uint8_t* frame;
	uint64_t size;
	const GLOBAL uint8_t* src;
	uint64_t total, new_bytes, first, first_new, stitch, enc_base0, enc_base1, enc_first;
	uint32_t keep, r, k, k0, header, n0, start, unused;
};
static_assert(sizeof(GlobalAppendFrame) == sizeof(AppendBatchFrame) && offsetof(GlobalAppendFrame, stitch) == offsetof(AppendBatchFrame, stitch) &&
		      offsetof(GlobalAppendFrame, keep) == offsetof(AppendBatchFrame, keep),
	      "");
#undef GLOBAL

// Waves per SIMD, as append_decode (append_kernels.hip).
#ifndef STENOS_DECODE_OCCUPANCY_T8
#define STENOS_DECODE_OCCUPANCY_T8 8
#endif
constexpr uint32_t append_batch_decode_occupancy(uint32_t TT) { return TT == 8 ? STENOS_DECODE_OCCUPANCY_T8 : 8; }

// Superblock keep_f of frame f = dec[blockIdx.x], whole, to the frame's stitch slot: append_decode's step (append_kernels.hip) on
// the frame's own pointer, size and entries of the old index.  A zstd-based code only sets DECODE_STATUS_HOST_CODES again:
// append_batch_plan has flagged the frame for the host.
template <uint32_t TT>
__global__ __launch_bounds__(64, append_batch_decode_occupancy(TT)) void append_batch_decode(AppendBatchArgs a)
{
	const uint32_t f = a.dec[blockIdx.x];
	const GlobalAppendFrame& fr = ((const GlobalAppendFrame*)a.frames)[f];
	DecodeArgs d = DecodeArgs();
	d.frame = (const uint8_t*)fr.frame;
	d.size = fr.size;
	d.sb_off = a.idx + fr.first + f;
	d.dst = (uint8_t*)((uintptr_t)a.raw + fr.stitch - (uint64_t)fr.keep * a.sb); // (+ keep * sb: the slot)
	d.total_bytes = fr.total;
	d.nsb = (uint64_t)fr.keep + 1;
	d.sb_bytes = a.sb;
	d.T = a.T;
	d.status = a.words + APPEND_W_STATUS;
	decode_superblock_entry<TT>(g_lds, d, fr.keep);
}

__global__ __launch_bounds__(64 * APPEND_COMMIT_WAVES) void append_batch_stitch(AppendBatchArgs a)
{
	const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
	append_batch_stitch_wave(a, (uint64_t)blockIdx.x * APPEND_COMMIT_WAVES + w);
}

__global__ __launch_bounds__(APPEND_PLAN_THREADS) void append_batch_commit_plan(AppendBatchArgs a)
{
	const uint32_t st = append_batch_commit_plan_thread(a, (uint64_t)blockIdx.x * APPEND_PLAN_THREADS + threadIdx.x);
	if (st)
		atomicOr(a.words + APPEND_W_STATUS, st);
}

__global__ __launch_bounds__(APPEND_PLAN_THREADS) void append_batch_index(AppendBatchArgs a)
{
	append_batch_index_thread(a, (uint64_t)blockIdx.x * APPEND_PLAN_THREADS + threadIdx.x);
}

__global__ __launch_bounds__(64 * APPEND_COMMIT_WAVES) void append_batch_commit(AppendBatchArgs a)
{
	const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
	append_batch_commit_wave(a, (uint64_t)blockIdx.x * APPEND_COMMIT_WAVES + w);
}

// workgroups of `per` units each for n units; 0: more than a grid holds
uint32_t groups_of(uint64_t n, uint32_t per)
{
	const uint64_t g = (n + per - 1) / per;
	return g > 0x7FFFFFFFull ? 0u : (uint32_t)g;
}

} // namespace

hipError_t stenos_ab_launch_plan(const AppendBatchArgs& a, hipStream_t stream)
{
	const uint32_t groups = groups_of(a.m, APPEND_PLAN_THREADS);
	if (!groups)
		return hipErrorInvalidValue;
	hipLaunchKernelGGL(append_batch_plan, dim3(groups), dim3(APPEND_PLAN_THREADS), 0, stream, a);
	return hipGetLastError();
}

hipError_t stenos_ab_launch_decode(const AppendBatchArgs& a, hipStream_t stream)
{
	if (a.ndec == 0)
		return hipSuccess;
	if (a.T == 0 || a.T > STENOS_K_LDS_MAX_T || a.ndec > 0x7FFFFFFFu)
		return hipErrorInvalidValue;
	return stenos_k_decode_variant(a.T, [&](auto tt) { return stenos_k_launch_decoder(append_batch_decode<decltype(tt)::value>, a.ndec, a.T, stream, a); });
}

hipError_t stenos_ab_launch_stitch(const AppendBatchArgs& a, uint64_t chunks, hipStream_t stream)
{
	if (chunks == 0)
		return hipSuccess;
	const uint32_t groups = groups_of(chunks, APPEND_COMMIT_WAVES);
	if (!groups)
		return hipErrorInvalidValue;
	hipLaunchKernelGGL(append_batch_stitch, dim3(groups), dim3(64 * APPEND_COMMIT_WAVES), 0, stream, a);
	return hipGetLastError();
}

hipError_t stenos_ab_launch_commit_plan(const AppendBatchArgs& a, uint64_t K, hipStream_t stream)
{
	const uint32_t groups = groups_of(K, APPEND_PLAN_THREADS);
	if (!groups)
		return hipErrorInvalidValue;
	hipLaunchKernelGGL(append_batch_commit_plan, dim3(groups), dim3(APPEND_PLAN_THREADS), 0, stream, a);
	return hipGetLastError();
}

hipError_t stenos_ab_launch_index(const AppendBatchArgs& a, uint64_t moved, hipStream_t stream)
{
	if (moved == 0)
		return hipSuccess;
	const uint32_t groups = groups_of(moved, APPEND_PLAN_THREADS);
	if (!groups)
		return hipErrorInvalidValue;
	hipLaunchKernelGGL(append_batch_index, dim3(groups), dim3(APPEND_PLAN_THREADS), 0, stream, a);
	return hipGetLastError();
}

hipError_t stenos_ab_launch_commit(const AppendBatchArgs& a, uint64_t chunks, hipStream_t stream)
{
	const uint32_t groups = groups_of(chunks, APPEND_COMMIT_WAVES);
	if (!groups)
		return hipErrorInvalidValue;
	hipLaunchKernelGGL(append_batch_commit, dim3(groups), dim3(64 * APPEND_COMMIT_WAVES), 0, stream, a);
	return hipGetLastError();
}
