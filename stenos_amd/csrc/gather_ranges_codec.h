// gather_ranges_codec.h -- variable-length ranges gathered out of one frame by offsets and lengths that live on the device
// (stenos_hip_gather_ranges, gather_ranges.h): which ranges are valid, how many pieces a range has, where the packed output of
// range i begins (the exclusive prefix sums D of the lengths, formed by three passes that the stream orders: no workgroup waits
// for another), and how piece slot t finds its range and is cut at the frame's superblock boundaries.  The piece table that
// comes out is the one gather_scan and gather_decode consume (gather.h); nothing of the decoder is in here.
// The per-thread rules are plain C++ in the vocabulary of gather_codec.h (GATHER_HD): the kernels (gather_ranges_kernels.hip),
// the host unit (gather_ranges_host.cpp: the pieces of superblocks the host finishes) and the host emulation
// (tests/emul_gather_ranges) include the one copy.  The block steps are templates over the block width W and over `each`, which
// runs a step for every thread of the block and ends it with a barrier: in a kernel each(f) is f(threadIdx.x); __syncthreads(),
// in the emulation a loop over k < W -- so the emulation runs the same steps at a width of 4.
#ifndef STENOS_GATHER_RANGES_CODEC_H
#define STENOS_GATHER_RANGES_CODEC_H
#ifndef STENOS_GATHER_CUT_H
#define GATHER_CUT_ONLY
#include "gather_codec.h"
#undef GATHER_CUT_ONLY
#endif

#if defined(__HIPCC__) && !defined(WV_HOST_EMULATION)
#define RANGES_FN static __device__ __forceinline__
#else
#define RANGES_FN static inline
#endif

namespace codec {

// DECODE_STATUS_BAD_ROW and DECODE_STATUS_DST_OVERFLOW (kernels.h, which the emulation cannot include;
// gather_ranges_kernels.hip asserts that they are the same).  With one of them set the call makes no piece.
enum : uint32_t { RANGES_ST_BAD_RANGE = 8, RANGES_ST_DST_OVERFLOW = 16, RANGES_ST_GATE = RANGES_ST_BAD_RANGE | RANGES_ST_DST_OVERFLOW };

// The words at the start of the call's buffer (zero on entry); they come back to the host in one copy.
struct RangesWords {
	uint32_t status;  // DECODE_STATUS_* of the call
	uint32_t npieces; // pieces of all ranges
	uint64_t total;   // D[n]
};

struct RangesArgs {
	const uint64_t* offsets; // n (device)
	const uint64_t* lengths; // n (device)
	uint64_t n;
	uint64_t total;          // bytes of the original array
	uint64_t sb;             // superblock bytes of the frame (1 for an empty array: never a piece)
	uint64_t dst_size;       // capacity of the packed output
	uint64_t pmax;           // ranges_piece_bound(): piece slots of the call
	uint32_t nblocks;        // ceil(n / W) of the sums and apply passes
	RangesWords* words;
	uint64_t* D;             // n + 1: where range i begins in the packed output; D[n]: the bytes of all ranges
	uint32_t* pstart;        // n + 1: the first piece slot of range i; pstart[n]: the pieces of all ranges
	uint64_t* block_bytes;   // nblocks: the sums of the blocks, then their exclusive prefixes
	uint32_t* block_pieces;  // nblocks
	uint32_t* count;         // the tables of gather.h: nsb counts (zero on entry) ...
	const uint32_t* ppre;    // ... their prefixes (gather_scan)
	GatherPiece* pieces;     // pmax entries
};

// ---- one range ----
// A valid range has offset <= total and length <= total - offset (no sum that may wrap is formed).  Its pieces are its
// intersections with the superblocks it touches, in order: non-empty, disjoint, their lengths sum to the length.  A range of
// length 0 has none.  False: invalid, and it counts as 0 bytes and 0 pieces.
GATHER_HD bool ranges_measure(uint64_t total, uint64_t sb, uint64_t off, uint64_t len, uint64_t* bytes, uint32_t* pieces)
{
	*bytes = 0;
	*pieces = 0;
	if (off > total || len > total - off)
		return false;
	if (len) {
		*bytes = len;
		*pieces = (uint32_t)((off + len - 1) / sb - off / sb + 1);
	}
	return true;
}

// A range of length L >= 1 touches at most floor((L - 1) / sb) + 2 superblocks, so ranges whose lengths sum to at most dst_size
// have at most 2 n + floor(dst_size / sb) pieces.  0: beyond 2^31 - 1 (32-bit piece starts, one thread per slot).
GATHER_HD uint64_t ranges_piece_bound(uint64_t n, uint64_t dst_size, uint64_t sb)
{
	const uint64_t lim = 0x7FFFFFFFull;
	if (n > lim / 2 || dst_size / sb > lim - 2 * n)
		return 0;
	return 2 * n + dst_size / sb;
}

// Piece j (below the range's count) of the valid range [off, off + len), whose packed output begins at d: the part inside
// superblock off / sb + j.  lo = j ? 0 : off % sb;  hi: the end of the range, clipped to the superblock;  destination d + (piece
// begin - off).
GATHER_HD void ranges_cut(uint64_t sb, uint64_t off, uint64_t len, uint64_t d, uint64_t j, uint64_t* sbn, GatherPiece* p)
{
	const uint64_t end = off + len; // (<= total)
	const uint64_t s = off / sb + j, begin = s * sb;
	const uint64_t lo = j ? 0 : off - begin;
	const uint64_t hi = end - begin < sb ? end - begin : sb;
	*sbn = s;
	p->lo = (uint32_t)lo;
	p->hi = (uint32_t)hi;
	p->dst = d + (begin + lo - off);
}

// Sums of lengths stop at 2^64 - 1 instead of wrapping (n lengths of up to 2^56 - 1 may pass 2^64); a sum that stands there
// counts as beyond every dst_size.  min(a + b, 2^64 - 1) is associative, so the scan may group as it likes.
GATHER_HD uint64_t ranges_add(uint64_t a, uint64_t b)
{
	const uint64_t r = a + b;
	return r < a ? ~(uint64_t)0 : r;
}
GATHER_HD bool ranges_overflow(uint64_t sum, uint64_t dst_size) { return sum > dst_size || sum == ~(uint64_t)0; }

} // namespace codec

// ---- the block steps: the kernels, and the emulation (which has no atomics and no device) ----
#if (defined(__HIPCC__) && !defined(WV_HOST_EMULATION)) || defined(RANGES_HOST_STEPS)
namespace codec {

#if defined(__HIP_DEVICE_COMPILE__)
RANGES_FN uint32_t ranges_fetch_add(uint32_t* p, uint32_t v) { return atomicAdd(p, v); }
RANGES_FN void ranges_or(uint32_t* p, uint32_t v) { atomicOr(p, v); }
#else
RANGES_FN uint32_t ranges_fetch_add(uint32_t* p, uint32_t v)
{
	const uint32_t r = *p;
	*p = r + v;
	return r;
}
RANGES_FN void ranges_or(uint32_t* p, uint32_t v) { *p |= v; }
#endif

// What a block of W threads scans: (bytes, pieces) per thread, two sides that take turns so that a step is one barrier.
template <uint32_t W>
struct RangesTile {
	uint64_t bytes[2][W];
	uint32_t pieces[2][W];
};

// Inclusive sums over side 0 (Hillis-Steele: log2 W steps, every thread reads one side and writes the other); returns the side
// that holds them.  The exclusive sum of thread k is entry k - 1 of that side (0 for k == 0).
template <uint32_t W, class Each>
RANGES_FN uint32_t ranges_tile_scan(RangesTile<W>& t, Each& each)
{
	uint32_t side = 0;
	for (uint32_t d = 1; d < W; d <<= 1, side ^= 1)
		each([&](uint32_t k) {
			t.bytes[side ^ 1][k] = ranges_add(t.bytes[side][k], k >= d ? t.bytes[side][k - d] : 0);
			t.pieces[side ^ 1][k] = t.pieces[side][k] + (k >= d ? t.pieces[side][k - d] : 0u);
		});
	return side;
}
template <uint32_t W>
RANGES_FN uint64_t ranges_tile_bytes_before(const RangesTile<W>& t, uint32_t side, uint32_t k) { return k ? t.bytes[side][k - 1] : 0; }
template <uint32_t W>
RANGES_FN uint32_t ranges_tile_pieces_before(const RangesTile<W>& t, uint32_t side, uint32_t k) { return k ? t.pieces[side][k - 1] : 0u; }

// stage 1, measure: thread k of block `block` takes range block * W + k (beyond n: nothing) into side 0 of the tile
template <uint32_t W>
RANGES_FN void ranges_measure_thread(const RangesArgs& a, uint32_t block, uint32_t k, RangesTile<W>& t, bool flag_invalid)
{
	const uint64_t i = (uint64_t)block * W + k;
	uint64_t bytes = 0;
	uint32_t pieces = 0;
	if (i < a.n && !ranges_measure(a.total, a.sb, a.offsets[i], a.lengths[i], &bytes, &pieces) && flag_invalid)
		ranges_or(&a.words->status, RANGES_ST_BAD_RANGE);
	t.bytes[0][k] = bytes;
	t.pieces[0][k] = pieces;
}

// stage 2, first pass (one block per W ranges): the block's sums
template <uint32_t W, class Each>
RANGES_FN void ranges_block_sums(const RangesArgs& a, uint32_t block, RangesTile<W>& t, Each& each)
{
	each([&](uint32_t k) { ranges_measure_thread<W>(a, block, k, t, true); });
	const uint32_t side = ranges_tile_scan<W>(t, each);
	each([&](uint32_t k) {
		if (k == W - 1) {
			a.block_bytes[block] = t.bytes[side][k];
			a.block_pieces[block] = t.pieces[side][k];
		}
	});
}

// stage 2, second pass (ONE block): thread k sums its run of the blocks' sums, the runs' sums are scanned, then every thread
// turns its run into exclusive prefixes in place (gather_scan's way).  The last thread publishes D[n] and the piece total and
// sets the overflow bit.
template <uint32_t W, class Each>
RANGES_FN void ranges_scan_sums(const RangesArgs& a, RangesTile<W>& t, Each& each)
{
	const uint32_t run = (a.nblocks + W - 1) / W;
	auto begin_of = [&](uint32_t k) {
		const uint64_t b = (uint64_t)k * run;
		return (uint32_t)(b < a.nblocks ? b : a.nblocks);
	};
	each([&](uint32_t k) {
		uint64_t bytes = 0;
		uint32_t pieces = 0;
		for (uint32_t s = begin_of(k), e = begin_of(k + 1); s < e; ++s) {
			bytes = ranges_add(bytes, a.block_bytes[s]);
			pieces += a.block_pieces[s];
		}
		t.bytes[0][k] = bytes;
		t.pieces[0][k] = pieces;
	});
	const uint32_t side = ranges_tile_scan<W>(t, each);
	each([&](uint32_t k) {
		uint64_t bytes = ranges_tile_bytes_before<W>(t, side, k);
		uint32_t pieces = ranges_tile_pieces_before<W>(t, side, k);
		for (uint32_t s = begin_of(k), e = begin_of(k + 1); s < e; ++s) {
			const uint64_t b = a.block_bytes[s];
			const uint32_t p = a.block_pieces[s];
			a.block_bytes[s] = bytes;
			a.block_pieces[s] = pieces;
			bytes = ranges_add(bytes, b);
			pieces += p;
		}
		if (k == W - 1) {
			const uint64_t sum = t.bytes[side][k];
			a.words->total = sum;
			a.words->npieces = t.pieces[side][k];
			a.D[a.n] = sum;
			a.pstart[a.n] = t.pieces[side][k];
			if (ranges_overflow(sum, a.dst_size))
				ranges_or(&a.words->status, RANGES_ST_DST_OVERFLOW);
		}
	});
}

// stage 2, third pass (one block per W ranges): D[i] and pstart[i] = the block's prefix + the sums in front of i in the block
template <uint32_t W, class Each>
RANGES_FN void ranges_block_apply(const RangesArgs& a, uint32_t block, RangesTile<W>& t, Each& each)
{
	each([&](uint32_t k) { ranges_measure_thread<W>(a, block, k, t, false); });
	const uint32_t side = ranges_tile_scan<W>(t, each);
	each([&](uint32_t k) {
		const uint64_t i = (uint64_t)block * W + k;
		if (i < a.n) {
			a.D[i] = ranges_add(a.block_bytes[block], ranges_tile_bytes_before<W>(t, side, k));
			a.pstart[i] = a.block_pieces[block] + ranges_tile_pieces_before<W>(t, side, k);
		}
	});
}

// stage 3: the piece of slot t.  False: none -- a gating bit is set (then no slot has one), or t is at or beyond the piece total.
// The slot finds its range by pstart[i] <= t < pstart[i + 1] (empty ranges span nothing and are passed over) and cuts piece
// t - pstart[i] of it.
RANGES_FN bool ranges_piece_of_slot(const RangesArgs& a, uint64_t t, uint64_t* s, GatherPiece* p)
{
	if ((a.words->status & RANGES_ST_GATE) || t >= a.words->npieces)
		return false;
	const uint32_t i = gather_find32(a.pstart, (uint32_t)a.n, (uint32_t)t);
	ranges_cut(a.sb, a.offsets[i], a.lengths[i], a.D[i], t - a.pstart[i], s, p);
	return true;
}
// ... counted (gather_count's part), and, after gather_scan, put in its superblock's run of the table (gather_fill's)
RANGES_FN void ranges_count_slot(const RangesArgs& a, uint64_t t)
{
	uint64_t s;
	GatherPiece p;
	if (ranges_piece_of_slot(a, t, &s, &p))
		ranges_fetch_add(a.count + s, 1u);
}
RANGES_FN void ranges_fill_slot(const RangesArgs& a, uint64_t t)
{
	uint64_t s;
	GatherPiece p;
	if (ranges_piece_of_slot(a, t, &s, &p))
		a.pieces[a.ppre[s] + ranges_fetch_add(a.count + s, 1u)] = p;
}

} // namespace codec
#endif
#endif
