// gather_kernels.hip -- gfx950 kernels behind stenos_hip_gather_rows (gather.h):
//   gather_count, gather_scan, gather_fill   the pieces of all rows, ordered by superblock, on the device
//   gather_decode  one wavefront per (superblock, chunk of up to 64 of its pieces): one walk over the superblock's chain of
//                  blocks delivers them all (gather_codec.h, decode_superblock_pieces)
// Compiled with the decoder's options (csrc/Makefile, decode_kernels.hip): gather_decode has no divergent branch.
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "gather.h"
#include "gather_codec.h"

using namespace codec;
using namespace wv;

namespace {

extern __shared__ __attribute__((aligned(16))) uint8_t g_lds[];

constexpr uint32_t PIECE_THREADS = 256, SCAN_THREADS = 1024;

// Waves per SIMD the kernel for bytesoftype TT is compiled for: eight, as decode_superblocks (decode_kernels.hip).  The kernel
// holds one decoder (the LDS-image path; whole superblocks take it too) and the lane's piece in four registers across it.
// Bytesoftype 4 (the mini-LZ decoder of 32-bit elements is the widest) spills eight registers at eight (64 vector registers);
// at seven it has 72 and spills none.
constexpr uint32_t gather_decode_occupancy(uint32_t TT) { return TT == 4 ? 7 : 8; }

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

// superblock of wavefront x: pre[s] <= x < pre[s + 1] (superblocks without pieces are passed over).  Every lane searches for
// the same x, so the loads are scalar (batch.h, stenos_b_find_item).
__device__ __forceinline__ uint32_t find_superblock(const uint32_t* __restrict__ pre, uint32_t n, uint32_t x)
{
	uint32_t lo = 0, hi = n;
	while (hi - lo > 1) {
		const uint32_t mid = (lo + hi) >> 1;
		if (pre[mid] <= x)
			lo = mid;
		else
			hi = mid;
	}
	return lo;
}

// DECODE_STATUS_* bits of one chunk (0: its pieces are in place)
template <uint32_t TT>
__device__ __forceinline__ uint32_t decode_gather_chunk(const GatherArgs& a, uint32_t s, const uint8_t* tab, uint32_t count)
{
	const uint32_t T = TT ? TT : a.T;
	const uint64_t p = a.sb_off[s];
	if (p > a.size || a.size - p < 4) // (written without sums: an index entry may hold anything)
		return DECODE_STATUS_TRUNCATED;
	const uint32_t code = a.frame[p];
	const uint32_t csize = (uint32_t)a.frame[p + 1] | ((uint32_t)a.frame[p + 2] << 8) | ((uint32_t)a.frame[p + 3] << 16);
	const uint64_t begin = (uint64_t)s * a.shape.sb;
	const uint32_t dsize = (uint32_t)((a.shape.total - begin) < a.shape.sb ? (a.shape.total - begin) : a.shape.sb);
	if (a.size - p - 4 < csize) // stenos.cpp:1133-1134
		return DECODE_STATUS_TRUNCATED;
	const LanePieces q = load_pieces(tab, count);
	if (ballot((q.lo > q.hi) | (q.hi > U32(dsize)))) // (gather_fill writes no such piece)
		return DECODE_STATUS_INVALID;
	const uint8_t* payload = a.frame + p + 4;
	if (code == 1)
		return decode_superblock_pieces(g_lds, make_dec_layout(T), T, payload, csize, dsize, q, a.dst) == DEC_ERROR ? DECODE_STATUS_INVALID : 0u;
	if (code == 6) { // stenos.cpp:741-746
		if (csize != dsize)
			return DECODE_STATUS_INVALID;
		copy_superblock_pieces(payload, q, a.dst);
		return 0;
	}
	if (code >= 2 && code <= 5) { // zstd based codes are finished by the host
		gstore_uniform(a.sb_flags + s, 1u);
		return DECODE_STATUS_HOST_CODES;
	}
	return DECODE_STATUS_INVALID;
}

template <uint32_t TT>
__global__ __launch_bounds__(64, gather_decode_occupancy(TT)) void gather_decode(GatherArgs a)
{
	const uint32_t w = blockIdx.x;
	if (w >= a.wpre[a.nsb])
		return;
	const uint32_t s = find_superblock(a.wpre, a.nsb, w);
	const uint32_t first = a.ppre[s] + 64u * (w - a.wpre[s]), left = a.ppre[s + 1] - first;
	const uint32_t st = decode_gather_chunk<TT>(a, s, (const uint8_t*)(a.pieces + first), left < 64u ? left : 64u);
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
