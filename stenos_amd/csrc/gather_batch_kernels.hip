// gather_batch_kernels.hip -- gfx950 kernels behind stenos_hip_gather_rows_batch (gather_batch.h):
//   gather_batch_count, gather_batch_fill   the pieces of all pairs, ordered by the batch's superblock numbers, on the device
//                                           (gather_scan of gather_kernels.hip runs between them)
//   gather_batch_decode  one wavefront per (superblock of the batch, chunk of up to 64 of its pieces), through the functions of
//                        gather_codec.h that gather_decode uses
// Compiled with the decoder's options (csrc/Makefile, decode_kernels.hip): gather_batch_decode has no divergent branch.
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "gather_batch.h"
#include "gather_codec.h"

using namespace codec;
using namespace wv;

namespace {

extern __shared__ __attribute__((aligned(16))) uint8_t g_lds[];

constexpr uint32_t PIECE_THREADS = 256;

// Waves per SIMD, by the rule of gather_decode (gather_kernels.hip): the mini-LZ decoder of 32-bit elements spills at eight.
constexpr uint32_t gather_batch_decode_occupancy(uint32_t TT) { return TT == 4 ? 7 : 8; }

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

// DECODE_STATUS_* bits of one chunk (0: its pieces are in place): decode_gather_chunk of gather_kernels.hip with the frame's
// pointer, size and shape out of the table.  g: the superblock's number in the batch, f: its frame.
template <uint32_t TT>
__device__ __forceinline__ uint32_t decode_gather_batch_chunk(const GatherBatchArgs& a, uint32_t g, uint32_t f, const uint8_t* tab, uint32_t count)
{
	const uint32_t T = TT ? TT : a.T;
	const GlobalGatherFrame& fr = ((const GlobalGatherFrame*)a.frames)[f];
	const uint8_t* const frame = (const uint8_t*)fr.frame;
	const uint64_t size = fr.size, total = fr.total, sb = fr.sb;
	const uint64_t p = a.sb_off[(uint64_t)g + f];
	if (p > size || size - p < 4) // (written without sums: an index entry may hold anything)
		return DECODE_STATUS_TRUNCATED;
	const uint32_t code = frame[p];
	const uint32_t csize = (uint32_t)frame[p + 1] | ((uint32_t)frame[p + 2] << 8) | ((uint32_t)frame[p + 3] << 16);
	const uint64_t begin = (g - fr.first) * sb;
	if (begin >= total) // (the host's table: first[f] <= g < first[f] + nsb_f)
		return DECODE_STATUS_INVALID;
	const uint32_t dsize = (uint32_t)((total - begin) < sb ? (total - begin) : sb);
	if (size - p - 4 < csize) // stenos.cpp:1133-1134
		return DECODE_STATUS_TRUNCATED;
	const LanePieces q = load_pieces(tab, count);
	if (ballot((q.lo > q.hi) | (q.hi > U32(dsize)))) // (gather_batch_fill writes no such piece)
		return DECODE_STATUS_INVALID;
	const uint8_t* payload = frame + p + 4;
	if (code == 1)
		return decode_superblock_pieces(g_lds, make_dec_layout(T), T, payload, csize, dsize, q, a.dst) == DEC_ERROR ? DECODE_STATUS_INVALID : 0u;
	if (code == 6) { // stenos.cpp:741-746
		if (csize != dsize)
			return DECODE_STATUS_INVALID;
		copy_superblock_pieces(payload, q, a.dst);
		return 0;
	}
	if (code >= 2 && code <= 5) { // zstd based codes are finished by the host
		gstore_uniform(a.sb_flags + g, 1u);
		return DECODE_STATUS_HOST_CODES;
	}
	return DECODE_STATUS_INVALID;
}

template <uint32_t TT>
__global__ __launch_bounds__(64, gather_batch_decode_occupancy(TT)) void gather_batch_decode(GatherBatchArgs a)
{
	const uint32_t w = blockIdx.x;
	if (w >= a.wpre[a.S])
		return;
	const uint32_t g = gather_find32(a.wpre, a.S, w);
	const uint32_t f = gather_find64(a.first, a.m, g);
	const uint32_t first = a.ppre[g] + 64u * (w - a.wpre[g]), left = a.ppre[g + 1] - first;
	const uint32_t st = decode_gather_batch_chunk<TT>(a, g, f, (const uint8_t*)(a.pieces + first), left < 64u ? left : 64u);
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
