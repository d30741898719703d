// update_kernels.hip -- gfx950 kernels behind stenos_hip_update_rows (update.h):
//   update_plan         the compact list of the superblocks that hold pieces, k for the host
//   update_decode       one wavefront per touched superblock: the whole superblock -> its slot of the raw scratch buffer
//   update_apply        the pieces' source bytes -> the slots
//   update_splice_plan  the index and the size of the new frame
//   update_splice       one workgroup per superblock copies it to its place in the new frame
// What a thread or a wavefront of each does is in update_codec.h (the host emulation runs the same text).
// Compiled with the decoder's options (csrc/Makefile, decode_kernels.hip): update_decode has no divergent branch.
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "update.h"
#include "decode_body.h"
#include "update_codec.h"

using namespace codec;
using namespace wv;

static_assert(UPDATE_ST_TRUNCATED == DECODE_STATUS_TRUNCATED && UPDATE_ST_INVALID == DECODE_STATUS_INVALID && UPDATE_ST_HOST_CODES == DECODE_STATUS_HOST_CODES,
	      "update_codec.h");

namespace {

extern __shared__ __attribute__((aligned(16))) uint8_t g_lds[];

constexpr uint32_t PLAN_THREADS = UPDATE_PLAN_THREADS;

// inclusive sums of v over the workgroup's threads, in sh
template <class V>
__device__ __forceinline__ void scan_workgroup(V* sh, uint32_t k, V v)
{
	sh[k] = v;
	__syncthreads();
	for (uint32_t d = 1; d < PLAN_THREADS; d <<= 1) {
		const V t = k >= d ? sh[k - d] : (V)0;
		__syncthreads();
		sh[k] += t;
		__syncthreads();
	}
}

__global__ __launch_bounds__(PLAN_THREADS) void update_plan(UpdateArgs a)
{
	__shared__ uint32_t sh[PLAN_THREADS];
	const uint32_t k = threadIdx.x;
	uint32_t begin, end;
	update_run_of_thread(a.nsb, k, &begin, &end);
	const uint32_t t = update_plan_count(a, begin, end);
	scan_workgroup(sh, k, t);
	uint32_t last = 0;
	const uint32_t st = update_plan_write(a, begin, end, sh[k] - t, &last);
	if (st)
		atomicOr(a.words + UPDATE_W_STATUS, st);
	if (t)
		atomicMax(a.words + UPDATE_W_LAST, last);
	if (k == PLAN_THREADS - 1)
		a.words[UPDATE_W_K] = sh[k];
}

// Waves per SIMD, as decode_superblocks (decode_kernels.hip).
#ifndef STENOS_DECODE_OCCUPANCY_T8
#define STENOS_DECODE_OCCUPANCY_T8 8
#endif
constexpr uint32_t update_decode_occupancy(uint32_t TT) { return TT == 8 ? STENOS_DECODE_OCCUPANCY_T8 : 8; }

// The superblock in place blockIdx.x of the compact list, whole, into its slot: the one copy of the header checks and the code
// 1 / 6 dispatch that decode_frames_batch uses (decode_body.h), given a destination base that puts superblock s at the slot.
// A zstd-based code only sets DECODE_STATUS_HOST_CODES again: update_plan has flagged it for the host.
template <uint32_t TT>
__global__ __launch_bounds__(64, update_decode_occupancy(TT)) void update_decode(UpdateArgs a)
{
	const uint32_t c = blockIdx.x;
	const uint32_t s = a.touched[c];
	DecodeArgs d = DecodeArgs();
	d.frame = a.frame;
	d.size = a.size;
	d.sb_off = a.idx;
	d.dst = (uint8_t*)((uintptr_t)a.raw + (uint64_t)c * a.sb - (uint64_t)s * a.sb); // (+ s * sb: the slot)
	d.total_bytes = a.total;
	d.nsb = a.nsb;
	d.sb_bytes = a.sb;
	d.T = a.T;
	d.status = a.words + UPDATE_W_STATUS;
	decode_superblock_entry<TT>(g_lds, d, s);
}

__global__ __launch_bounds__(64) void update_apply(UpdateArgs a) { update_apply_wave(a, blockIdx.x, blockIdx.y); }

__global__ __launch_bounds__(PLAN_THREADS) void update_splice_plan(UpdateArgs a)
{
	__shared__ uint64_t sh[PLAN_THREADS];
	const uint32_t k = threadIdx.x;
	uint32_t begin, end, st = 0;
	update_run_of_thread(a.nsb, k, &begin, &end);
	const uint64_t sum = update_splice_sum(a, begin, end, &st);
	scan_workgroup(sh, k, sum);
	if (st)
		atomicOr(a.words + UPDATE_W_STATUS, st);
	update_splice_write(a, begin, end, a.header + sh[k] - sum);
	if (k == PLAN_THREADS - 1) {
		const uint64_t total = a.header + sh[k];
		a.new_idx[a.nsb] = total;
		a.words[UPDATE_W_TOTAL] = (uint32_t)total;
		a.words[UPDATE_W_TOTAL + 1] = (uint32_t)(total >> 32);
	}
}

__global__ __launch_bounds__(64 * UPDATE_SPLICE_WAVES) void update_splice(UpdateArgs a)
{
	update_splice_wave(a, blockIdx.x, (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)));
}

} // namespace

hipError_t stenos_u_launch_plan(const UpdateArgs& a, hipStream_t stream)
{
	hipLaunchKernelGGL(update_plan, dim3(1), dim3(PLAN_THREADS), 0, stream, a);
	return hipGetLastError();
}

hipError_t stenos_u_launch_decode(const UpdateArgs& a, hipStream_t stream)
{
	if (a.k == 0)
		return hipSuccess;
	if (a.T == 0 || a.T > STENOS_K_LDS_MAX_T)
		return hipErrorInvalidValue;
	return stenos_k_decode_variant(a.T, [&](auto tt) { return stenos_k_launch_decoder(update_decode<decltype(tt)::value>, a.k, a.T, stream, a); });
}

hipError_t stenos_u_launch_apply(const UpdateArgs& a, hipStream_t stream)
{
	if (a.k == 0)
		return hipSuccess;
	hipLaunchKernelGGL(update_apply, dim3(a.k, UPDATE_APPLY_WAVES), dim3(64), 0, stream, a);
	return hipGetLastError();
}

hipError_t stenos_u_launch_splice_plan(const UpdateArgs& a, hipStream_t stream)
{
	hipLaunchKernelGGL(update_splice_plan, dim3(1), dim3(PLAN_THREADS), 0, stream, a);
	return hipGetLastError();
}

hipError_t stenos_u_launch_splice(const UpdateArgs& a, hipStream_t stream)
{
	hipLaunchKernelGGL(update_splice, dim3(a.nsb ? a.nsb : 1u), dim3(64 * UPDATE_SPLICE_WAVES), 0, stream, a);
	return hipGetLastError();
}
