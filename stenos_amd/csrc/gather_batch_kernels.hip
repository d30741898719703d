// gather_batch_kernels.hip -- gfx950 kernels behind stenos_hip_gather_rows_batch (gather_batch.h):
//   gather_batch_count, gather_batch_fill   the pieces of all pairs, ordered by the batch's superblock numbers, on the device
//                                           (gather_scan of gather_kernels.hip runs between them)
//   gather_batch_decode  one wavefront per (superblock of the batch, chunk of up to 64 of its pieces): decode_gather_chunk of
//                        gather_codec.h, which gather_decode calls too, on what the frame table says
// Compiled with the decoder's options (csrc/Makefile, decode_kernels.hip): gather_batch_decode has no divergent branch.
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "gather_batch.h"
#include "gather_codec.h"

using namespace codec;
using namespace wv;

namespace {

extern __shared__ __attribute__((aligned(16))) uint8_t g_lds[];

// The piece of thread t = i * P + j; false: none (beyond the table, an invalid pair -- flagged --, a j beyond the frame's own
// piece count, a row that ends in front).
__device__ __forceinline__ bool piece_of_thread(const GatherBatchArgs& a, uint64_t* g, GatherPiece* p)
{
	const uint64_t t = (uint64_t)blockIdx.x * PIECE_THREADS + threadIdx.x;
	if (t >= a.npieces)
		return false;
	const uint64_t i = a.P == 1 ? t : t / a.P, j = t - i * a.P;
	const int r = gather_cut_pair(a.frames, a.m, a.row_bytes, a.dst_stride, a.frame_ids[i], a.rows[i], i, j, g, p);
	if (r == GATHER_PAIR_INVALID && j == 0)
		atomicOr(a.status, (uint32_t)DECODE_STATUS_BAD_ROW);
	return r == GATHER_PAIR_PIECE;
}

__global__ __launch_bounds__(PIECE_THREADS) void gather_batch_count(GatherBatchArgs a)
{
	uint64_t g;
	GatherPiece p;
	if (piece_of_thread(a, &g, &p))
		atomicAdd(a.count + g, 1u);
}

__global__ __launch_bounds__(PIECE_THREADS) void gather_batch_fill(GatherBatchArgs a)
{
	uint64_t g;
	GatherPiece p;
	if (piece_of_thread(a, &g, &p))
		a.pieces[a.ppre[g] + atomicAdd(a.count + g, 1u)] = p;
}

// The frame's entry comes out of memory, and a pointer loaded as a plain one is a flat pointer: what is loaded through it may be
// private to a lane, so the compiler would take everything read from the frame for divergent (batch_decode_kernels.hip,
// GlobalDecodeArgs).  The table is read as what it is: GatherFrame with a pointer into global memory, the same layout.
#define GLOBAL __attribute__((address_space(1)))
struct GlobalGatherFrame {
	const GLOBAL uint8_t* frame;
	uint64_t size, total, valid_rows, sb, first;
	uint32_t nsb, pieces;
};
static_assert(sizeof(GlobalGatherFrame) == sizeof(GatherFrame) && offsetof(GlobalGatherFrame, nsb) == offsetof(GatherFrame, nsb), "");
#undef GLOBAL

// g: the superblock's number in the batch, f: its frame, whose pointer, size and shape come out of the table
template <uint32_t TT>
__global__ __launch_bounds__(64, gather_decode_occupancy(TT)) void gather_batch_decode(GatherBatchArgs a)
{
	const uint32_t w = blockIdx.x;
	if (w >= a.wpre[a.S])
		return;
	const uint32_t g = gather_find32(a.wpre, a.S, w);
	const uint32_t f = gather_find64(a.first, a.m, g);
	const uint32_t first = a.ppre[g] + 64u * (w - a.wpre[g]), left = a.ppre[g + 1] - first;
	const GlobalGatherFrame& fr = ((const GlobalGatherFrame*)a.frames)[f];
	const uint32_t st = decode_gather_chunk<TT>(g_lds, a.T, (const uint8_t*)fr.frame, fr.size, fr.total, fr.sb, g - fr.first, a.sb_off[(uint64_t)g + f],
						(const uint8_t*)(a.pieces + first), left < 64u ? left : 64u, a.dst, a.sb_flags + g);
	if (st)
		status_or(a.status, st);
}

} // namespace

static uint32_t piece_grid(const GatherBatchArgs& a) { return (uint32_t)((a.npieces + PIECE_THREADS - 1) / PIECE_THREADS); }

hipError_t stenos_gb_launch_count(const GatherBatchArgs& a, hipStream_t stream)
{
	hipLaunchKernelGGL(gather_batch_count, dim3(piece_grid(a)), dim3(PIECE_THREADS), 0, stream, a);
	return hipGetLastError();
}
hipError_t stenos_gb_launch_fill(const GatherBatchArgs& a, hipStream_t stream)
{
	hipLaunchKernelGGL(gather_batch_fill, dim3(piece_grid(a)), dim3(PIECE_THREADS), 0, stream, a);
	return hipGetLastError();
}

hipError_t stenos_gb_launch_decode(const GatherBatchArgs& a, hipStream_t stream)
{
	if (a.waves == 0)
		return hipSuccess;
	if (a.T == 0 || a.T > STENOS_K_LDS_MAX_T)
		return hipErrorInvalidValue;
	return stenos_k_decode_variant(a.T, [&](auto tt) { return stenos_k_launch_decoder(gather_batch_decode<decltype(tt)::value>, a.waves, a.T, stream, a); });
}
