// gather_ranges_kernels.hip -- gfx950 kernels behind stenos_hip_gather_ranges (gather_ranges.h): the cutting stage for ranges
// whose piece count differs from range to range.  Every rule is in gather_ranges_codec.h; in here are the kernels, which give
// the block steps their threads and their barrier, and the launchers.  The decoding is gather_kernels.hip's, unchanged.
// Compiled with the decoder's options (csrc/Makefile), as gather_kernels.hip.
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "gather_ranges.h"

using namespace codec;

namespace {

constexpr uint32_t SCAN_THREADS = 1024;

static_assert(RANGES_ST_BAD_RANGE == DECODE_STATUS_BAD_ROW && RANGES_ST_DST_OVERFLOW == DECODE_STATUS_DST_OVERFLOW, "");
static_assert(sizeof(RangesWords) == 16 && sizeof(GatherPiece) == 16, "");

// a step of a block: every thread runs it, then all of them meet
struct BlockEach {
	template <class F>
	__device__ __forceinline__ void operator()(F f) const
	{
		f(threadIdx.x);
		__syncthreads();
	}
};

__global__ __launch_bounds__(STENOS_GR_BLOCK) void ranges_sums(RangesArgs a)
{
	__shared__ RangesTile<STENOS_GR_BLOCK> t;
	BlockEach each;
	ranges_block_sums<STENOS_GR_BLOCK>(a, blockIdx.x, t, each);
}

__global__ __launch_bounds__(SCAN_THREADS) void ranges_scan(RangesArgs a)
{
	__shared__ RangesTile<SCAN_THREADS> t;
	BlockEach each;
	ranges_scan_sums<SCAN_THREADS>(a, t, each);
}

__global__ __launch_bounds__(STENOS_GR_BLOCK) void ranges_apply(RangesArgs a)
{
	__shared__ RangesTile<STENOS_GR_BLOCK> t;
	BlockEach each;
	ranges_block_apply<STENOS_GR_BLOCK>(a, blockIdx.x, t, each);
}

__global__ __launch_bounds__(STENOS_GR_BLOCK) void ranges_count(RangesArgs a)
{
	const uint64_t t = (uint64_t)blockIdx.x * STENOS_GR_BLOCK + threadIdx.x;
	if (t < a.pmax)
		ranges_count_slot(a, t);
}

__global__ __launch_bounds__(STENOS_GR_BLOCK) void ranges_fill(RangesArgs a)
{
	const uint64_t t = (uint64_t)blockIdx.x * STENOS_GR_BLOCK + threadIdx.x;
	if (t < a.pmax)
		ranges_fill_slot(a, t);
}

} // namespace

static uint32_t slot_grid(const RangesArgs& a) { return (uint32_t)((a.pmax + STENOS_GR_BLOCK - 1) / STENOS_GR_BLOCK); }

hipError_t stenos_gr_launch_offsets(const RangesArgs& a, hipStream_t stream)
{
	if (a.n == 0 || a.nblocks != stenos_gr_blocks(a.n))
		return hipErrorInvalidValue;
	hipLaunchKernelGGL(ranges_sums, dim3(a.nblocks), dim3(STENOS_GR_BLOCK), 0, stream, a);
	hipLaunchKernelGGL(ranges_scan, dim3(1), dim3(SCAN_THREADS), 0, stream, a);
	hipLaunchKernelGGL(ranges_apply, dim3(a.nblocks), dim3(STENOS_GR_BLOCK), 0, stream, a);
	return hipGetLastError();
}
hipError_t stenos_gr_launch_count(const RangesArgs& a, hipStream_t stream)
{
	if (a.pmax == 0) // (the frame of an empty array: no slot)
		return hipSuccess;
	hipLaunchKernelGGL(ranges_count, dim3(slot_grid(a)), dim3(STENOS_GR_BLOCK), 0, stream, a);
	return hipGetLastError();
}
hipError_t stenos_gr_launch_fill(const RangesArgs& a, hipStream_t stream)
{
	if (a.pmax == 0) // (the frame of an empty array: no slot)
		return hipSuccess;
	hipLaunchKernelGGL(ranges_fill, dim3(slot_grid(a)), dim3(STENOS_GR_BLOCK), 0, stream, a);
	return hipGetLastError();
}
