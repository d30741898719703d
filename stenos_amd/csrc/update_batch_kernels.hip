// update_batch_kernels.hip -- gfx950 kernels behind stenos_hip_update_rows_batch (update_batch.h):
//   update_batch_plan         the compact list of the superblocks of all frames that hold pieces; K and (k_f, last_f) for the host
//   update_batch_decode       one wavefront per touched superblock: the whole superblock -> its slot of the raw scratch buffer
//   update_batch_apply        the pieces' source bytes -> the slots
//   update_batch_splice_plan  the indices and the sizes of the new frames
//   update_batch_splice       one workgroup per superblock of all frames copies it to its place in its new frame
// What a thread or a wavefront of each does is in update_codec.h (the host emulation, tests/emul_update_batch, runs the same text).
// Compiled with the decoder's options (csrc/Makefile, decode_kernels.hip): update_batch_decode has no divergent branch.
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "batch.h"
#include "update_batch.h"
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

__global__ __launch_bounds__(PLAN_THREADS) void update_batch_plan(UpdateBatchArgs a)
{
	__shared__ uint32_t sh[PLAN_THREADS];
	const uint32_t k = threadIdx.x;
	uint32_t begin, end;
	update_run_of_thread(a.S, k, &begin, &end);
	const uint32_t t = update_plan_count(a, begin, end);
	scan_workgroup(sh, k, t);
	const uint32_t st = update_batch_plan_write(a, begin, end, sh[k] - t);
	if (st)
		atomicOr(a.words + UPDATE_W_STATUS, st);
	if (k == PLAN_THREADS - 1)
		a.words[UPDATE_W_K] = sh[k];
}

// The frame's entry comes out of memory, and a pointer loaded as a plain one is a flat pointer: what is loaded through it may be
// private to a lane, so the compiler would take everything read from the frame for divergent (batch_decode_kernels.hip,
// GlobalDecodeArgs; gather_batch_kernels.hip).  The table is read as what it is: GatherFrame with a pointer into global memory.
#define GLOBAL __attribute__((address_space(1)))
struct GlobalUpdateFrame {
	const GLOBAL uint8_t* frame;
	uint64_t size, total, valid_rows, sb, first;
	uint32_t nsb, pieces;
};
static_assert(sizeof(GlobalUpdateFrame) == sizeof(GatherFrame) && offsetof(GlobalUpdateFrame, nsb) == offsetof(GatherFrame, nsb), "");
#undef GLOBAL

// The superblock in place blockIdx.x of the compact list, whole, into its slot: update_decode's step (update_kernels.hip), on
// the frame the superblock's number in the batch lies in.  The search is wave-uniform.  A zstd-based code only sets
// DECODE_STATUS_HOST_CODES again: update_batch_plan has flagged it for the host.
template <uint32_t TT>
__global__ __launch_bounds__(64, 8) void update_batch_decode(UpdateBatchArgs a)
{
	const uint32_t c = blockIdx.x;
	const uint32_t g = a.touched[c];
	const uint32_t f = stenos_b_find_item(a.first, a.m, g);
	const GlobalUpdateFrame& fr = ((const GlobalUpdateFrame*)a.frames)[f];
	const uint64_t s = g - fr.first;
	DecodeArgs d = DecodeArgs();
	d.frame = (const uint8_t*)fr.frame;
	d.size = fr.size;
	d.sb_off = a.idx + fr.first + f;
	d.dst = (uint8_t*)((uintptr_t)a.raw + (uint64_t)c * a.sb - s * a.sb); // (+ s * sb: the slot)
	d.total_bytes = fr.total;
	d.nsb = fr.nsb;
	d.sb_bytes = a.sb;
	d.T = a.T;
	d.status = a.words + UPDATE_W_STATUS;
	decode_superblock_entry<TT>(g_lds, d, (uint32_t)s);
}

__global__ __launch_bounds__(64) void update_batch_apply(UpdateBatchArgs a) { update_batch_apply_wave(a, blockIdx.x, blockIdx.y); }

__global__ __launch_bounds__(PLAN_THREADS) void update_batch_splice_plan(UpdateBatchArgs a)
{
	__shared__ uint64_t sh[PLAN_THREADS];
	const uint32_t k = threadIdx.x;
	uint32_t begin, end, st = 0;
	update_run_of_thread(a.S, k, &begin, &end);
	const uint64_t sum = update_batch_splice_sum(a, begin, end, &st);
	scan_workgroup(sh, k, sum);
	if (st)
		atomicOr(a.words + UPDATE_W_STATUS, st);
	update_batch_splice_write(a, begin, end, sh[k] - sum);
	if (k == PLAN_THREADS - 1)
		a.gpre[a.S] = sh[k];
	__syncthreads(); // (gpre is whole, and the workgroup sees it)
	update_batch_splice_index(a, begin, end);
	for (uint32_t f = k; f < a.m; f += PLAN_THREADS)
		update_batch_splice_total(a, f);
}

__global__ __launch_bounds__(64 * UPDATE_SPLICE_WAVES) void update_batch_splice(UpdateBatchArgs a)
{
	update_batch_splice_wave(a, blockIdx.x, (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)));
}

} // namespace

hipError_t stenos_ub_launch_plan(const UpdateBatchArgs& a, hipStream_t stream)
{
	hipLaunchKernelGGL(update_batch_plan, dim3(1), dim3(PLAN_THREADS), 0, stream, a);
	return hipGetLastError();
}

hipError_t stenos_ub_launch_decode(const UpdateBatchArgs& a, hipStream_t stream)
{
	if (a.K == 0)
		return hipSuccess;
	if (a.T == 0 || a.T > STENOS_K_LDS_MAX_T)
		return hipErrorInvalidValue;
	return stenos_k_decode_variant(a.T, [&](auto tt) { return stenos_k_launch_decoder(update_batch_decode<decltype(tt)::value>, a.K, a.T, stream, a); });
}

hipError_t stenos_ub_launch_apply(const UpdateBatchArgs& a, hipStream_t stream)
{
	if (a.K == 0)
		return hipSuccess;
	hipLaunchKernelGGL(update_batch_apply, dim3(a.K, UPDATE_APPLY_WAVES), dim3(64), 0, stream, a);
	return hipGetLastError();
}

hipError_t stenos_ub_launch_splice_plan(const UpdateBatchArgs& a, hipStream_t stream)
{
	hipLaunchKernelGGL(update_batch_splice_plan, dim3(1), dim3(PLAN_THREADS), 0, stream, a);
	return hipGetLastError();
}

hipError_t stenos_ub_launch_splice(const UpdateBatchArgs& a, hipStream_t stream)
{
	hipLaunchKernelGGL(update_batch_splice, dim3(a.S + a.m), dim3(64 * UPDATE_SPLICE_WAVES), 0, stream, a);
	return hipGetLastError();
}
