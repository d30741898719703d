// batch_decode_kernels.hip -- gfx950 kernels that decode many independent frames in one pass (batch.h):
//   frame_heads_batch    the first min(12, size) bytes of every frame, for the host's header checks
//   walk_frames_batch    one lane per item: the serial walk of its superblock chain (walk_superblocks, walk_kernels.hip); items
//                        with many superblocks take the parallel walk instead, one launch each (capi.cpp)
//   decode_frames_batch  one wavefront per superblock of all items (decode_body.h)
// Compiled with the decoder's options (csrc/Makefile, decode_kernels.hip): decode_frames_batch has no divergent branch.
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "batch.h"
#include "decode_body.h"

using namespace codec;
using namespace wv;

namespace {

extern __shared__ __attribute__((aligned(16))) uint8_t g_lds[];

constexpr uint32_t DECODE_BATCH_OCCUPANCY = 8; // waves per SIMD, as decode_superblocks (decode_kernels.hip)

__global__ __launch_bounds__(256) void frame_heads_batch(const uint8_t* const* __restrict__ frames, const uint64_t* __restrict__ sizes, uint32_t n, uint8_t* __restrict__ heads)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n)
		return;
	const uint64_t have = sizes[i] < 12 ? sizes[i] : 12;
	for (uint32_t k = 0; k < have; ++k)
		heads[12ull * i + k] = frames[i][k];
}

// off[s] = byte offset of superblock s's header, as walk_superblocks finds them
__global__ __launch_bounds__(64) void walk_frames_batch(const DecodeArgs* __restrict__ args, const uint64_t* __restrict__ first, const uint8_t* __restrict__ walk, uint32_t n)
{
	const uint32_t i = blockIdx.x * 64 + threadIdx.x;
	if (i >= n || !walk[i])
		return;
	const DecodeArgs& a = args[i];
	uint64_t* off = (uint64_t*)a.sb_off;
	uint64_t p = first[i];
	for (uint64_t s = 0; s < a.nsb; ++s) {
		if (p + 4 > a.size) { // stenos.cpp:1126-1127
			atomicOr(a.status, DECODE_STATUS_TRUNCATED);
			for (; s <= a.nsb; ++s)
				off[s] = a.size;
			return;
		}
		off[s] = p;
		const uint32_t csize = (uint32_t)a.frame[p + 1] | ((uint32_t)a.frame[p + 2] << 8) | ((uint32_t)a.frame[p + 3] << 16);
		p += 4 + (uint64_t)csize;
	}
	off[a.nsb] = p;
	if (p > a.size)
		atomicOr(a.status, DECODE_STATUS_TRUNCATED);
}

// The item's arguments come out of memory, not in as kernel arguments as decode_superblocks' do, and a pointer loaded as a plain
// one is a flat pointer: what is loaded through it may be private to a lane, so the compiler would take everything derived from
// it for divergent and rebuild the decoder's control flow around lane masks.  The table is read as what it is, DecodeArgs with
// pointers into global memory (the same layout), which keeps that control flow on the scalar unit.
#define GLOBAL __attribute__((address_space(1)))
struct GlobalDecodeArgs {
	const GLOBAL uint8_t* frame;
	uint64_t size;
	const GLOBAL uint64_t* sb_off;
	const GLOBAL uint32_t* sb_ids;
	GLOBAL uint8_t* dst;
	uint64_t total_bytes;
	uint64_t nsb;
	uint32_t sb_bytes;
	uint32_t T;
	GLOBAL uint32_t* status;
	GLOBAL uint8_t* wide_scratch;
	uint64_t wide_scratch_bytes;
};
static_assert(sizeof(GlobalDecodeArgs) == sizeof(DecodeArgs) && offsetof(GlobalDecodeArgs, status) == offsetof(DecodeArgs, status), "");
#undef GLOBAL

template <uint32_t TT>
__global__ __launch_bounds__(64, DECODE_BATCH_OCCUPANCY) void decode_frames_batch(const GlobalDecodeArgs* __restrict__ args, const uint64_t* __restrict__ spre, uint32_t n)
{
	const uint32_t i = stenos_b_find_item(spre, n, blockIdx.x);
	const GlobalDecodeArgs& g = args[i];
	DecodeArgs a;
	a.frame = (const uint8_t*)g.frame;
	a.size = g.size;
	a.sb_off = (const uint64_t*)g.sb_off;
	a.sb_ids = nullptr;
	a.dst = (uint8_t*)g.dst;
	a.total_bytes = g.total_bytes;
	a.nsb = g.nsb;
	a.sb_bytes = g.sb_bytes;
	a.T = g.T;
	a.status = (uint32_t*)g.status;
	decode_superblock_entry<TT>(g_lds, a, (uint32_t)(blockIdx.x - spre[i]));
}

} // namespace

hipError_t stenos_b_launch_heads(const uint8_t* const* frames, const uint64_t* sizes, uint32_t n, uint8_t* heads, hipStream_t stream)
{
	hipLaunchKernelGGL(frame_heads_batch, dim3((n + 255) / 256), dim3(256), 0, stream, frames, sizes, n, heads);
	return hipGetLastError();
}

hipError_t stenos_b_launch_walk(const DecodeArgs* args, const uint64_t* first, const uint8_t* walk, uint32_t n, hipStream_t stream)
{
	hipLaunchKernelGGL(walk_frames_batch, dim3((n + 63) / 64), dim3(64), 0, stream, args, first, walk, n);
	return hipGetLastError();
}

hipError_t stenos_b_launch_decode(const DecodeArgs* args, const uint64_t* spre, uint32_t n, uint64_t nsb, uint32_t T, hipStream_t stream)
{
	if (nsb == 0)
		return hipSuccess;
	return stenos_k_decode_variant(T, [&](auto tt) {
		return stenos_k_launch_decoder(decode_frames_batch<decltype(tt)::value>, (uint32_t)nsb, T, stream, (const GlobalDecodeArgs*)args, spre, n);
	});
}
