// range_decode_kernels.hip -- gfx950 kernel behind stenos_hip_decompress_ranges (range.h):
//   decode_ranges  one wavefront per unit: bytes [lo, hi) of one superblock of a frame -> the unit's destination
// A unit that covers its whole superblock takes the decoder of decode_superblocks (decode_superblock, registers to HBM for
// bytesoftype 2, 4, 8); a partial one takes the window decoder of range_codec.h, which stops behind the block that holds
// byte hi - 1.  Compiled with the decoder's options (csrc/Makefile, decode_kernels.hip): no divergent branch.
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "range.h"
#include "range_codec.h"

using namespace codec;
using namespace wv;

namespace {

extern __shared__ __attribute__((aligned(16))) uint8_t g_lds[];

// Waves per SIMD the kernel for bytesoftype TT is compiled for: eight, as decode_superblocks (decode_kernels.hip).  Bytesoftype 4
// holds two decoders -- the register path of whole superblocks and the window decoder -- and spills four registers at eight
// (64 vector registers); at seven it has 72 and spills none.
constexpr uint32_t decode_ranges_occupancy(uint32_t TT) { return TT == 4 ? 7 : 8; }

// The unit comes out of memory: its destination is read as a pointer into global memory, not as a flat one, so that what is
// derived from it stays wave-uniform for the compiler (batch_decode_kernels.hip, GlobalDecodeArgs).
#define GLOBAL __attribute__((address_space(1)))
struct GlobalRangeUnit {
	GLOBAL uint8_t* dst;
	uint32_t sb, lo, hi, unused;
};
static_assert(sizeof(GlobalRangeUnit) == sizeof(RangeUnit) && offsetof(GlobalRangeUnit, lo) == offsetof(RangeUnit, lo), "");
#undef GLOBAL

// DECODE_STATUS_* bits of one unit (0: its bytes are in place)
template <uint32_t TT>
__device__ __forceinline__ uint32_t decode_range_unit(const RangeArgs& a, const GlobalRangeUnit& u)
{
	const uint32_t T = TT ? TT : a.T;
	const uint64_t s = u.sb;
	const uint32_t lo = u.lo, hi = u.hi;
	uint8_t* dst = (uint8_t*)u.dst;
	const uint64_t p = a.sb_off ? a.sb_off[s] : a.direct_off;
	if (p > a.size || a.size - p < 4) // (written without sums: an index entry may hold anything)
		return DECODE_STATUS_TRUNCATED;
	const uint32_t code = a.frame[p];
	const uint32_t csize = (uint32_t)a.frame[p + 1] | ((uint32_t)a.frame[p + 2] << 8) | ((uint32_t)a.frame[p + 3] << 16);
	const uint64_t begin = s * (uint64_t)a.sb_bytes;
	const uint32_t dsize = (uint32_t)((a.total_bytes - begin) < a.sb_bytes ? (a.total_bytes - begin) : a.sb_bytes);
	if (a.size - p - 4 < csize) // stenos.cpp:1133-1134
		return DECODE_STATUS_TRUNCATED;
	if (lo >= hi || hi > dsize) // (the host builds no such unit)
		return DECODE_STATUS_INVALID;
	const uint8_t* payload = a.frame + p + 4;
	if (code == 1) {
		const DecLayout L = make_dec_layout(T);
		uint32_t r;
		if (lo == 0 && hi == dsize)
			r = decode_superblock(g_lds, L, T, payload, csize, dst, dsize, TT != 0);
		else
			r = decode_superblock_window(g_lds, L, T, payload, csize, dsize, lo, hi, dst);
		return r == DEC_ERROR ? DECODE_STATUS_INVALID : 0u;
	}
	if (code == 6) { // stenos.cpp:741-746
		if (csize != dsize)
			return DECODE_STATUS_INVALID;
		copy_g2g_wide<COPY_ROUNDS>(dst, payload + lo, hi - lo);
		return 0;
	}
	if (code >= 2 && code <= 5) // zstd based codes are finished by the host
		return DECODE_STATUS_HOST_CODES;
	return DECODE_STATUS_INVALID;
}

template <uint32_t TT>
__global__ __launch_bounds__(64, decode_ranges_occupancy(TT)) void decode_ranges(RangeArgs a)
{
	const GlobalRangeUnit* units = (const GlobalRangeUnit*)a.units;
	const uint32_t st = decode_range_unit<TT>(a, units[blockIdx.x]);
	gstore_uniform(a.unit_status + blockIdx.x, st);
	if (st)
		status_or(a.status, st);
}

} // namespace

hipError_t stenos_r_launch_decode(const RangeArgs& a, hipStream_t stream)
{
	if (a.nunits == 0)
		return hipSuccess;
	if (a.T == 0 || a.T > STENOS_K_LDS_MAX_T)
		return hipErrorInvalidValue;
	return stenos_k_decode_variant(a.T, [&](auto tt) { return stenos_k_launch_decoder(decode_ranges<decltype(tt)::value>, a.nunits, a.T, stream, a); });
}
