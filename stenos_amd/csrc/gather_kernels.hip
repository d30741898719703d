// gather_kernels.hip -- gfx950 kernels behind stenos_hip_gather_rows (gather.h):
//   gather_count, gather_scan, gather_fill   the pieces of all rows, ordered by superblock, on the device
//   gather_decode  one wavefront per (superblock, chunk of up to 64 of its pieces): one walk over the superblock's chain of
//                  blocks delivers them all (gather_codec.h: decode_gather_chunk, the rule gather_batch_decode follows too)
// Compiled with the decoder's options (csrc/Makefile, decode_kernels.hip): gather_decode has no divergent branch.
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "gather.h"
#include "gather_codec.h"

using namespace codec;
using namespace wv;

namespace {

extern __shared__ __attribute__((aligned(16))) uint8_t g_lds[];

constexpr uint32_t SCAN_THREADS = 1024;

// The piece of thread t = i * P + j; false: none (beyond the table, an invalid row -- flagged --, a row that ends in front).
__device__ __forceinline__ bool piece_of_thread(const GatherArgs& a, uint64_t* s, GatherPiece* p)
{
	const uint64_t t = (uint64_t)blockIdx.x * PIECE_THREADS + threadIdx.x;
	if (t >= a.npieces)
		return false;
	const uint64_t i = a.P == 1 ? t : t / a.P, j = t - i * a.P;
	const uint64_t row = a.rows[i];
	if (row >= a.valid_rows) {
		if (j == 0)
			atomicOr(a.status, (uint32_t)DECODE_STATUS_BAD_ROW);
		return false;
	}
	return gather_cut(a.shape, row, i, j, s, p);
}

__global__ __launch_bounds__(PIECE_THREADS) void gather_count(GatherArgs a)
{
	uint64_t s;
	GatherPiece p;
	if (piece_of_thread(a, &s, &p))
		atomicAdd(a.count + s, 1u);
}

// One workgroup: thread k sums the counts of its run of superblocks, the runs' sums are scanned in LDS, then every thread
// writes the prefixes of its run and clears its counts for gather_fill.
__global__ __launch_bounds__(SCAN_THREADS) void gather_scan(GatherArgs a)
{
	__shared__ uint32_t sp[SCAN_THREADS], sw[SCAN_THREADS];
	const uint32_t k = threadIdx.x;
	const uint32_t run = (a.nsb + SCAN_THREADS - 1) / SCAN_THREADS;
	const uint64_t b0 = (uint64_t)k * run, e0 = b0 + run;
	const uint32_t begin = (uint32_t)(b0 < a.nsb ? b0 : a.nsb), end = (uint32_t)(e0 < a.nsb ? e0 : a.nsb);
	uint32_t p = 0, w = 0;
	for (uint32_t s = begin; s < end; ++s) {
		const uint32_t c = a.count[s];
		p += c;
		w += (c + 63u) >> 6;
	}
	sp[k] = p;
	sw[k] = w;
	__syncthreads();
	for (uint32_t d = 1; d < SCAN_THREADS; d <<= 1) {
		const uint32_t tp = k >= d ? sp[k - d] : 0u, tw = k >= d ? sw[k - d] : 0u;
		__syncthreads();
		sp[k] += tp;
		sw[k] += tw;
		__syncthreads();
	}
	p = sp[k] - p;
	w = sw[k] - w;
	for (uint32_t s = begin; s < end; ++s) {
		const uint32_t c = a.count[s];
		a.ppre[s] = p;
		a.wpre[s] = w;
		a.count[s] = 0;
		p += c;
		w += (c + 63u) >> 6;
	}
	if (k == SCAN_THREADS - 1) {
		a.ppre[a.nsb] = sp[k];
		a.wpre[a.nsb] = sw[k];
	}
}

__global__ __launch_bounds__(PIECE_THREADS) void gather_fill(GatherArgs a)
{
	uint64_t s;
	GatherPiece p;
	if (piece_of_thread(a, &s, &p))
		a.pieces[a.ppre[s] + atomicAdd(a.count + s, 1u)] = p;
}

static_assert(GATHER_ST_TRUNCATED == DECODE_STATUS_TRUNCATED && GATHER_ST_INVALID == DECODE_STATUS_INVALID && GATHER_ST_HOST_CODES == DECODE_STATUS_HOST_CODES, "");

template <uint32_t TT>
__global__ __launch_bounds__(64, gather_decode_occupancy(TT)) void gather_decode(GatherArgs a)
{
	const uint32_t w = blockIdx.x;
	if (w >= a.wpre[a.nsb])
		return;
	const uint32_t s = gather_find32(a.wpre, a.nsb, w);
	const uint32_t first = a.ppre[s] + 64u * (w - a.wpre[s]), left = a.ppre[s + 1] - first;
	const uint32_t st = decode_gather_chunk<TT>(g_lds, a.T, a.frame, a.size, a.shape.total, a.shape.sb, s, a.sb_off[s], (const uint8_t*)(a.pieces + first),
						left < 64u ? left : 64u, a.dst, a.sb_flags + s);
	if (st)
		status_or(a.status, st);
}

} // namespace

static uint32_t piece_grid(const GatherArgs& a) { return (uint32_t)((a.npieces + PIECE_THREADS - 1) / PIECE_THREADS); }

hipError_t stenos_g_launch_count(const GatherArgs& a, hipStream_t stream)
{
	hipLaunchKernelGGL(gather_count, dim3(piece_grid(a)), dim3(PIECE_THREADS), 0, stream, a);
	return hipGetLastError();
}
hipError_t stenos_g_launch_scan(const GatherArgs& a, hipStream_t stream)
{
	hipLaunchKernelGGL(gather_scan, dim3(1), dim3(SCAN_THREADS), 0, stream, a);
	return hipGetLastError();
}
hipError_t stenos_g_launch_fill(const GatherArgs& a, hipStream_t stream)
{
	hipLaunchKernelGGL(gather_fill, dim3(piece_grid(a)), dim3(PIECE_THREADS), 0, stream, a);
	return hipGetLastError();
}

hipError_t stenos_g_launch_decode(const GatherArgs& a, hipStream_t stream)
{
	if (a.waves == 0)
		return hipSuccess;
	if (a.T == 0 || a.T > STENOS_K_LDS_MAX_T)
		return hipErrorInvalidValue;
	return stenos_k_decode_variant(a.T, [&](auto tt) { return stenos_k_launch_decoder(gather_decode<decltype(tt)::value>, a.waves, a.T, stream, a); });
}
