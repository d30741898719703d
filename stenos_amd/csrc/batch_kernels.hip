// batch_kernels.hip -- gfx950 kernels that compress many independent items into many frames in one pass (batch.h):
//   encode_blocks_batch   one wavefront per 256-element block of all items (the body of encode_blocks, kernels.hip)
//   plan_frames_batch     one wavefront per superblock of all items -> plan_superblock (pipeline.h)
//   scan_frames_batch     one wavefront per item: superblock offsets in rounds of 64 (wave prefix sum), frame header of an
//                         empty item
//   resolve_frames_batch  one wavefront per item -> resolve_capacity (returns at once when the plan flagged nothing)
//   tiny_gather / tiny_apply  the last superblocks under 128 bytes, around zstd on the host (capi.cpp)
//   pack_frames_batch     PACK_WAVES wavefronts per superblock of all items -> pack_superblock
// The per-frame kernels of kernels.hip are not used here and not changed by it.
#include <hip/hip_runtime.h>

#include "batch.h"

using namespace codec;
using namespace wv;

namespace {

extern __shared__ __attribute__((aligned(16))) uint8_t g_lds[];

// A pointer field of the item table read as what it is, a pointer into global memory: loaded as a plain (flat) pointer, what is
// loaded through it could be private to a lane, and the compiler would take everything derived from it for divergent.
template <class P>
__device__ __forceinline__ P* global_field(P* const& field)
{
	return (P*)*(__attribute__((address_space(1))) P* const*)&field;
}

template <uint32_t TT>
__global__ __launch_bounds__(64) void encode_blocks_batch(const FrameJob* __restrict__ jobs, const uint64_t* __restrict__ bpre, uint32_t n)
{
	const uint32_t i = stenos_b_find_item(bpre, n, blockIdx.x);
	const FrameJob& j = jobs[i];
	const uint64_t b = blockIdx.x - bpre[i];
	const uint32_t T = TT ? TT : j.T;
	const Layout L = make_layout(T, true);
	const uint8_t* src = global_field(j.src);
	uint8_t* slots = global_field(j.slots);
	BlockInfo r;
	if (b < j.nfull)
		r = encode_block_job(g_lds, L, T, src + b * (uint64_t)(256 * T), slots + b * (uint64_t)j.slot_stride, true);
	else
		r = encode_tail_job(g_lds, L, T, src + j.nfull * (uint64_t)(256 * T), j.tail_bytes, slots + j.nfull * (uint64_t)j.slot_stride);
	if (threadIdx.x == 0) {
		global_field(j.bsize)[b] = r.size;
		global_field(j.binfo)[b] = r.info;
		global_field(j.bneed)[b] = r.need;
	}
}

__global__ __launch_bounds__(64) void plan_frames_batch(const FrameJob* __restrict__ jobs, const uint64_t* __restrict__ spre, uint32_t n)
{
	const uint32_t i = stenos_b_find_item(spre, n, blockIdx.x);
	const FrameJob& j = jobs[i];
	const Layout L = make_layout(j.T, true);
	plan_superblock(g_lds, L, j, blockIdx.x - spre[i]);
}

// sb_off[0 .. nsb] and *total of item blockIdx.x, from its header bytes on.  An item of 0 bytes gets its frame header here
// (stenos.cpp:876-878); an item the host refused (shift_byte 0xFFFFFFFF, no superblocks) is left alone.
__global__ __launch_bounds__(64) void scan_frames_batch(const FrameJob* __restrict__ jobs)
{
	const FrameJob& j = jobs[blockIdx.x];
	const uint32_t lane = threadIdx.x;
	if (j.nsb == 0) {
		if (j.shift_byte == 0xFFFFFFFFu)
			return;
		if (lane < j.header_bytes)
			j.dst[lane] = (uint8_t)(lane == 0 ? j.shift_byte : lane < 8 ? 0u : j.sb_bytes >> (8 * (lane - 8)));
		if (lane == 0)
			*j.total = j.header_bytes;
		return;
	}
	uint64_t running = j.header_bytes;
	for (uint64_t base = 0; base < j.nsb; base += 64) {
		const uint64_t s = base + lane;
		const uint32_t v = s < j.nsb ? j.sb_csize[s] + 4 : 0; // (64 superblocks of at most 2^24 + 4 bytes: 32 bits hold the sum)
		uint32_t incl = v;
		for (uint32_t o = 1; o < 64; o <<= 1) {
			const uint32_t up = __shfl_up(incl, o);
			if (lane >= o)
				incl += up;
		}
		if (s < j.nsb)
			j.sb_off[s] = running + incl - v;
		running += (uint32_t)__shfl((int)incl, 63);
	}
	if (lane == 0) {
		j.sb_off[j.nsb] = running;
		*j.total = running;
	}
}

__global__ __launch_bounds__(64) void resolve_frames_batch(const FrameJob* __restrict__ jobs)
{
	const FrameJob& j = jobs[blockIdx.x];
	const Layout L = make_layout(j.T, true);
	resolve_capacity(g_lds, L, j);
}

// the k-th tiny last superblock: its offset, the item's status and its input bytes, for the host's zstd
__global__ __launch_bounds__(64) void tiny_gather(const FrameJob* __restrict__ jobs, const uint32_t* __restrict__ tiny, BatchTinyIn* __restrict__ out)
{
	const FrameJob& j = jobs[tiny[blockIdx.x]];
	BatchTinyIn& o = out[blockIdx.x];
	const uint32_t lane = threadIdx.x;
	const uint64_t begin = (j.nsb - 1) * (uint64_t)j.sb_bytes;
	const uint32_t last = (uint32_t)(j.total_bytes - begin);
	for (uint32_t k = lane; k < 128; k += 64)
		o.raw[k] = k < last ? j.src[begin + k] : 0;
	if (lane == 0) {
		o.off_last = j.sb_off[j.nsb - 1];
		o.status = *j.status;
		o.pad = 0;
	}
}

// ... and the host's verdict on it (one thread per tiny superblock): code, size and end of the frame, or an overflow
__global__ __launch_bounds__(64) void tiny_apply(const FrameJob* __restrict__ jobs, const uint32_t* __restrict__ tiny, uint32_t ntiny, const BatchTinyOut* __restrict__ in)
{
	const uint32_t k = blockIdx.x * 64 + threadIdx.x;
	if (k >= ntiny)
		return;
	const FrameJob& j = jobs[tiny[k]];
	const BatchTinyOut& t = in[k];
	if (t.code == 0) {
		*j.status |= ENCODE_STATUS_DST_OVERFLOW;
		return;
	}
	j.sb_code[j.nsb - 1] = (uint8_t)t.code;
	j.sb_csize[j.nsb - 1] = t.csize;
	j.sb_off[j.nsb] = t.end;
	*j.total = t.end;
}

__global__ __launch_bounds__(64) void pack_frames_batch(const FrameJob* __restrict__ jobs, const uint64_t* __restrict__ spre, uint32_t n)
{
	const uint64_t g = blockIdx.x / PACK_WAVES;
	const uint32_t i = stenos_b_find_item(spre, n, g);
	pack_superblock(g_lds, jobs[i], g - spre[i], blockIdx.x % PACK_WAVES);
}

} // namespace

template <uint32_t TT>
static hipError_t launch_encode_batch_t(const FrameJob* jobs, const uint64_t* bpre, uint32_t n, uint64_t nblocks, uint32_t T, hipStream_t stream)
{
	const size_t lds = stenos_k_encode_lds_bytes(T);
	hipError_t e = hipFuncSetAttribute((const void*)encode_blocks_batch<TT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
	if (e != hipSuccess)
		return e;
	hipLaunchKernelGGL(encode_blocks_batch<TT>, dim3((uint32_t)nblocks), dim3(64), lds, stream, jobs, bpre, n);
	return hipGetLastError();
}

hipError_t stenos_b_launch_encode(const FrameJob* jobs, const uint64_t* bpre, uint32_t n, uint64_t nblocks, uint32_t T, hipStream_t stream)
{
	if (nblocks == 0)
		return hipSuccess;
	switch (T) {
		case 2: return launch_encode_batch_t<2>(jobs, bpre, n, nblocks, T, stream);
		case 4: return launch_encode_batch_t<4>(jobs, bpre, n, nblocks, T, stream);
		case 8: return launch_encode_batch_t<8>(jobs, bpre, n, nblocks, T, stream);
		default: return launch_encode_batch_t<0>(jobs, bpre, n, nblocks, T, stream);
	}
}

hipError_t stenos_b_launch_plan(const FrameJob* jobs, const uint64_t* spre, uint32_t n, uint64_t nsb, hipStream_t stream)
{
	if (nsb == 0)
		return hipSuccess;
	hipLaunchKernelGGL(plan_frames_batch, dim3((uint32_t)nsb), dim3(64), 0, stream, jobs, spre, n);
	return hipGetLastError();
}

hipError_t stenos_b_launch_scan(const FrameJob* jobs, uint32_t n, hipStream_t stream)
{
	hipLaunchKernelGGL(scan_frames_batch, dim3(n), dim3(64), 0, stream, jobs);
	return hipGetLastError();
}

hipError_t stenos_b_launch_resolve(const FrameJob* jobs, uint32_t n, uint32_t T, hipStream_t stream)
{
	const size_t lds = stenos_k_encode_lds_bytes(T); // (the replay re-encodes blocks)
	hipError_t e = hipFuncSetAttribute((const void*)resolve_frames_batch, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
	if (e != hipSuccess)
		return e;
	hipLaunchKernelGGL(resolve_frames_batch, dim3(n), dim3(64), lds, stream, jobs);
	return hipGetLastError();
}

hipError_t stenos_b_launch_tiny_gather(const FrameJob* jobs, const uint32_t* tiny, uint32_t ntiny, BatchTinyIn* out, hipStream_t stream)
{
	hipLaunchKernelGGL(tiny_gather, dim3(ntiny), dim3(64), 0, stream, jobs, tiny, out);
	return hipGetLastError();
}

hipError_t stenos_b_launch_tiny_apply(const FrameJob* jobs, const uint32_t* tiny, uint32_t ntiny, const BatchTinyOut* in, hipStream_t stream)
{
	hipLaunchKernelGGL(tiny_apply, dim3((ntiny + 63) / 64), dim3(64), 0, stream, jobs, tiny, ntiny, in);
	return hipGetLastError();
}

hipError_t stenos_b_launch_pack(const FrameJob* jobs, const uint64_t* spre, uint32_t n, uint64_t nsb, uint32_t bps, hipStream_t stream)
{
	if (nsb == 0)
		return hipSuccess;
	hipLaunchKernelGGL(pack_frames_batch, dim3((uint32_t)(nsb * PACK_WAVES)), dim3(64), pack_lds_bytes(bps), stream, jobs, spre, n);
	return hipGetLastError();
}
