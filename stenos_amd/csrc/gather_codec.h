// gather_codec.h -- rows gathered by row number out of one frame (stenos_hip_gather_rows, gather.h) or many
// (stenos_hip_gather_rows_batch, gather_batch.h): how a row is cut into pieces at the frame's superblock boundaries, what a
// wavefront does with its superblock (decode_gather_chunk: the index entry and the header checked, the dispatch on the code), and
// how it delivers up to 64 pieces of one BLOCK superblock (code 1) with one walk over its chain of blocks.  The cutting is plain
// C++: the kernels (gather_kernels.hip, gather_batch_kernels.hip), the host units (which define GATHER_CUT_ONLY and get nothing
// else) and the host emulations (tests/emul_gather, tests/emul_gather_batch) include the one copy.  The chunk rule and the decoder
// are written in the wavevec.h vocabulary, so the emulation runs the same code as both kernels.
// (two include guards: gather.h takes the cutting alone, a kernel file that includes it takes the rest afterwards)
#ifndef STENOS_GATHER_CUT_H
#define STENOS_GATHER_CUT_H
#include <stdint.h>

#if defined(__HIPCC__) && !defined(WV_HOST_EMULATION)
#define GATHER_HD static __host__ __device__ __forceinline__
#else
#define GATHER_HD static inline
#endif

namespace codec {

// One piece as it stands in the superblock-ordered table: bytes [lo, hi) of its superblock go to dst[d, d + hi - lo), d counted
// from the call's d_dst.  lo == hi: an empty piece (an idle lane).
struct GatherPiece {
	uint32_t lo, hi;
	uint64_t dst;
};

struct GatherShape {
	uint64_t row_bytes;  // >= 1
	uint64_t dst_stride; // >= row_bytes
	uint64_t total;      // bytes of the original array
	uint64_t sb;         // superblock bytes of the frame
};

// Pieces per row, fixed for a call: 1 when no row can straddle a superblock boundary (rows start at multiples of row_bytes,
// so that is when row_bytes divides the superblock size), else ceil((row_bytes - 1) / sb) + 1 -- a row that starts on the last
// byte of a superblock.  (Written without row_bytes + sb: that sum may wrap.)
GATHER_HD uint64_t gather_pieces_per_row(uint64_t row_bytes, uint64_t sb)
{
	if (sb % row_bytes == 0)
		return 1;
	return (row_bytes - 2) / sb + 2; // (row_bytes >= 2 here)
}

// Rows the array holds: a valid row number is below this.  The host computes it and hands it to the kernels, which never
// form row * row_bytes for a number that has not passed this test.
GATHER_HD uint64_t gather_valid_rows(uint64_t total, uint64_t row_bytes) { return total / row_bytes; }

// Piece j of the row `row` (valid, see above) that goes to slot i: the part of the row inside superblock off / sb + j,
// off = row * row_bytes.  False: the row does not reach that superblock (an empty piece; *sbn and p are not written).
//   lo = j ? 0 : off % sb;  hi: the end of the row, clipped to the superblock's decoded size;
//   destination offset i * dst_stride + (piece start - off).
GATHER_HD bool gather_cut(const GatherShape& g, uint64_t row, uint64_t i, uint64_t j, uint64_t* sbn, GatherPiece* p)
{
	const uint64_t off = row * g.row_bytes, end = off + g.row_bytes;
	const uint64_t s = off / g.sb + j, begin = s * g.sb;
	const uint64_t lo = j ? 0 : off - begin;
	if (begin + lo >= end)
		return false;
	const uint64_t dsize = g.total - begin < g.sb ? g.total - begin : g.sb; // (begin < end <= total)
	const uint64_t hi = end - begin < dsize ? end - begin : dsize;
	*sbn = s;
	p->lo = (uint32_t)lo;
	p->hi = (uint32_t)hi;
	p->dst = i * g.dst_stride + (begin + lo - off);
	return true;
}

// ---- rows of many frames in one call (stenos_hip_gather_rows_batch, gather_batch.h) ----
// The superblocks of the batch are numbered through: superblock s of frame f is first_f + s, first_f = the superblocks of the
// frames in front of it.  One entry per frame, made by the host (gather_frame below) and read by every kernel of the call:
struct GatherFrame {
	const uint8_t* frame; // device pointer
	uint64_t size;        // frame bytes
	uint64_t total;       // bytes of the original array (0: no row is valid)
	uint64_t valid_rows;  // gather_valid_rows(total, row_bytes)
	uint64_t sb;          // superblock bytes of the frame (1 for an empty array: never divided by)
	uint64_t first;       // number of its superblock 0 in the batch
	uint32_t nsb;
	uint32_t pieces;      // gather_pieces_per_row(row_bytes, sb) of this frame: at most the call's P (0 for an empty array)
};

GATHER_HD GatherFrame gather_frame(const uint8_t* frame, uint64_t size, uint64_t total, uint64_t sb, uint64_t nsb, uint64_t first, uint64_t row_bytes)
{
	GatherFrame f;
	f.frame = frame;
	f.size = size;
	f.total = total;
	f.valid_rows = total ? gather_valid_rows(total, row_bytes) : 0;
	f.sb = total ? sb : 1;
	f.first = first;
	f.nsb = (uint32_t)(total ? nsb : 0);
	f.pieces = (uint32_t)(total ? gather_pieces_per_row(row_bytes, sb) : 0);
	return f;
}

enum { GATHER_PAIR_NONE = 0, GATHER_PAIR_PIECE = 1, GATHER_PAIR_INVALID = -1 };

// Piece j (of the call's P) of the pair (frame number fid, row number row) that goes to slot i, cut with that frame's own shape:
//   GATHER_PAIR_INVALID  fid >= m or row >= the frame's valid rows: the pair makes no piece (the caller flags it, once per pair);
//   GATHER_PAIR_NONE     j is beyond the frame's own piece count, or the row does not reach that superblock;
//   GATHER_PAIR_PIECE    *gsb = first_f + superblock, *p as gather_cut leaves it.
// The frame's entry is read only after fid has passed its test, row * row_bytes is formed only after row has passed its own.
GATHER_HD int gather_cut_pair(const GatherFrame* frames, uint64_t m, uint64_t row_bytes, uint64_t dst_stride, uint64_t fid, uint64_t row, uint64_t i, uint64_t j,
			      uint64_t* gsb, GatherPiece* p)
{
	if (fid >= m)
		return GATHER_PAIR_INVALID;
	const GatherFrame& f = frames[fid];
	if (row >= f.valid_rows)
		return GATHER_PAIR_INVALID;
	if (j >= f.pieces)
		return GATHER_PAIR_NONE;
	const GatherShape g = { row_bytes, dst_stride, f.total, f.sb };
	uint64_t s;
	if (!gather_cut(g, row, i, j, &s, p))
		return GATHER_PAIR_NONE;
	*gsb = f.first + s;
	return GATHER_PAIR_PIECE;
}

// The entry of wavefront / superblock x in exclusive prefix sums: pre[k] <= x < pre[k + 1], entries that span nothing are passed
// over (batch.h, stenos_b_find_item: in a kernel every lane searches for the same x, so the loads are scalar).  pre has n + 1
// entries and x < pre[n].
GATHER_HD uint32_t gather_find32(const uint32_t* pre, uint32_t n, uint32_t x)
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
GATHER_HD uint32_t gather_find64(const uint64_t* pre, uint32_t n, uint64_t x)
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

} // namespace codec
#endif

#if !defined(GATHER_CUT_ONLY) && !defined(STENOS_GATHER_CODEC_H)
#define STENOS_GATHER_CODEC_H
#include "range_codec.h"

namespace codec {

// The lane's piece of a chunk: `count` (1..64) consecutive entries of the piece table at tab (16-byte entries); the lanes
// from count on hold an empty piece.  (The destination is read by all lanes: the idle ones read entry 0's and ignore it.)
struct LanePieces {
	U32 lo, hi, dlo, dhi;
};
WV_FN LanePieces load_pieces(const uint8_t* tab, uint32_t count)
{
	const U32 lane = lane_id_plain();
	const Pred p = lane < U32(count);
	const U32 at = sel(p, lane, U32(0u)) * 16u;
	LanePieces q;
	q.lo = gld32(tab, at, p);
	q.hi = gld32(tab, at + 4u, p);
	gld64(tab, at + 8u, q.dlo, q.dhi);
	return q;
}

// where piece `l` of the chunk wants the byte at superblock offset `from` (>= its lo): a wave-uniform pointer
WV_FN uint8_t* piece_target(uint8_t* dst, const LanePieces& q, uint32_t l, uint32_t from)
{
	const uint64_t d = (uint64_t)readlane(q.dlo, l) | ((uint64_t)readlane(q.dhi, l) << 32);
	return dst + d + (from - readlane(q.lo, l));
}

// The pieces of one chunk out of the superblock whose payload is `csize` bytes at src and which decodes to dsize bytes (every
// lane: lo == hi, or lo < hi <= dsize) -> dst + the piece's offset.  One walk over the chain from block 0, as
// decode_superblock_window's (range_codec.h: the same window, the same step over copied blocks that nothing wants): every
// block is decoded into the LDS image, one ballot tells which pieces it holds bytes of, and a scalar loop over those lanes
// stores each intersection (store_image_window).  The walk ends behind the block that holds the largest hi - 1 of the chunk:
// nothing behind it is read or checked.  Returns 0, or DEC_ERROR under the conditions of decode_superblock for the blocks up
// to that one.  Nothing in here branches on a lane-dependent value.
WV_FN uint32_t decode_superblock_pieces(Lds lds, const DecLayout& L, uint32_t T, const uint8_t* src, uint32_t csize, uint32_t dsize, const LanePieces& q, uint8_t* dst)
{
	const U32 lane = lane_id_plain();
	const uint32_t bs = 256 * T, hs = header_bytes(T);
	const uint32_t top = wave_max(q.hi); // (an empty piece has hi <= lo; its hi counts for nothing below: it holds no byte of any block)
	if (ballot(q.hi > q.lo) == 0)
		return 0;
	if (dsize == 0 || csize == 0)
		return DEC_ERROR;
	const uint32_t nblocks = dsize / bs;
	if (csize < hs + T && nblocks) // block_compress.h:1813-1815
		return DEC_ERROR;
	dec_write_lut(lds, L);
	const uint32_t wcap = window_bytes(T);
	const uint32_t mis = (uint32_t)((uintptr_t)src & 15u); // the window is filled from the 16-byte aligned address below src
	const uint8_t* abase = src - mis;
	uint32_t wstart = 0, wfill = 0, wend = 0; // window holds abase[wstart, wend), wend = wstart + wfill
	uint32_t consumed = 0;          // payload bytes consumed so far

	// (decode_superblock_window's: the window only moves forward; a block that was stepped over may lie behind its end, then nothing is kept)
	auto ensure = [&](uint32_t need) {
		uint32_t a = consumed + mis;
		if (a >= wstart && a + need <= wend)
			return;
		const uint32_t nstart = a & ~15u;
		const uint32_t endoff = csize + mis;
		const uint32_t nfill = endoff - nstart < wcap ? endoff - nstart : wcap;
		uint32_t keep = 0;
		if (wfill && nstart >= wstart && nstart < wstart + wfill && ((wstart + wfill) & 15u) == 0) {
			keep = wstart + wfill - nstart;
			const uint32_t d = nstart - wstart;
			for (uint32_t o = 0; o < keep; o += 1024) {
				U32 off = U32(o) + lane * 16u;
				Pred p = off < U32(keep);
				U128 v = lds_ld128(lds, U32(L.win + d) + sel(p, off, U32(0u)));
				wave_sync();
				lds_st128(lds, U32(L.win) + off, v, p);
				wave_sync();
			}
		}
		wstart = nstart;
		wfill = nfill;
		wend = nstart + nfill;
		if (nfill > keep)
			copy_g2l(lds, L.win + keep, abase + wstart + keep, nfill - keep);
		wave_sync();
	};
	// image bytes [at, at + len) of the superblock are in the LDS image: every piece of `want` takes what it holds of them
	auto deliver = [&](uint64_t want, uint32_t at, uint32_t len) {
		for (uint64_t m = want; m; m &= m - 1) {
			const uint32_t l = (uint32_t)__builtin_ctzll(m);
			const uint32_t plo = readlane(q.lo, l), phi = readlane(q.hi, l);
			const uint32_t a = plo > at ? plo : at, e = phi < at + len ? phi : at + len;
			store_image_window(piece_target(dst, q, l, a), lds, L.img, a - at, e - at);
		}
	};

	const uint32_t last = (top - 1u) / bs; // the block that holds the chunk's last byte (nblocks: the tail)
	for (uint32_t b = 0; b < nblocks && b <= last; ++b) {
		const uint32_t at = b * bs;
		const uint32_t left = csize - consumed;
		const uint32_t need = left < max_stream_block_bytes(T) ? left : max_stream_block_bytes(T);
		const uint64_t want = ballot((q.lo < U32(at + bs)) & (q.hi > U32(at)) & (q.hi > q.lo));
		if (!want && left) { // no piece holds a byte of it: a copied block needs its length checked, not its bytes
			ensure(1);
			if (win_u8(lds + L.win, consumed + mis - wstart) == BLOCK_COPY) {
				if (left < 1 + bs)
					return DEC_ERROR;
				consumed += 1 + bs;
				continue;
			}
		}
		ensure(need);
		const uint32_t n = decode_block(lds, L, T, consumed + mis - wstart, need, 16, true);
		if (n == DEC_ERROR)
			return DEC_ERROR;
		if (want) { // (every predicated store is waited for, wavevec.h)
			deliver(want, at, bs);
			wave_sync();
		}
		consumed += n;
	}
	const uint32_t tail = dsize - nblocks * bs, tb = nblocks * bs;
	if (tail && top > tb) { // [254] + partial block, as in decode_superblock
		if (consumed == csize)
			return DEC_ERROR;
		const uint32_t left = csize - consumed;
		const uint32_t need = left < max_stream_tail_bytes(T) ? left : max_stream_tail_bytes(T);
		ensure(need);
		const uint32_t cur = consumed + mis - wstart;
		if (win_u8(lds + L.win, cur) != BLOCK_PARTIAL)
			return DEC_ERROR;
		const uint32_t lines = tail / (16 * T);
		uint32_t n = 0;
		if (lines) {
			n = decode_block(lds, L, T, cur + 1, need - 1, lines, false);
			if (n == DEC_ERROR)
				return DEC_ERROR;
		}
		const uint32_t rem = tail - lines * 16 * T;
		if (1 + n + rem > need)
			return DEC_ERROR;
		for (uint32_t o = 0; o < rem; o += 64) {
			Pred p = (U32(o) + lane) < U32(rem);
			U32 v = lds_ld8(lds + L.win, U32(cur + 1 + n + o) + sel(p, lane, U32(0u)));
			lds_st8(lds, U32(L.img + lines * 16 * T + o) + lane, v, p);
		}
		wave_sync();
		deliver(ballot((q.hi > U32(tb)) & (q.hi > q.lo)), tb, tail);
	}
	return 0;
}

// The same chunk out of a superblock that is stored as it is (code 6): per piece a copy of its slice of the payload.
WV_FN void copy_superblock_pieces(const uint8_t* payload, const LanePieces& q, uint8_t* dst)
{
	for (uint64_t m = ballot(q.hi > q.lo); m; m &= m - 1) {
		const uint32_t l = (uint32_t)__builtin_ctzll(m);
		const uint32_t plo = readlane(q.lo, l);
		copy_g2g_wide<COPY_ROUNDS>(piece_target(dst, q, l, plo), payload + plo, readlane(q.hi, l) - plo);
	}
}

// ---- what a gather wavefront does with its superblock (gather_decode, gather_batch_decode, tests/emul_gather) ----
// DECODE_STATUS_* (kernels.h, which the emulation cannot include; gather_kernels.hip asserts that they are the same)
enum : uint32_t { GATHER_ST_TRUNCATED = 1, GATHER_ST_INVALID = 2, GATHER_ST_HOST_CODES = 4 };

// a byte of the frame, the same for every lane (the emulation's accessor is the audited one)
#ifdef WV_HOST_EMULATION
WV_FN uint32_t frame_u8(const uint8_t* p) { return gload_uniform8(p); }
#else
WV_FN uint32_t frame_u8(const uint8_t* p) { return *p; }
#endif

// One chunk: `count` (1..64) entries of the piece table at tab, all of superblock s of the frame (`size` bytes; the array has
// `total` bytes in superblocks of sb) whose header the index puts at p.  The status bits of the chunk; 0: its pieces are in place
// at dst + their offsets.  A superblock that went through zstd (codes 2-5) sets *flag and is left to the host.
// TT: the bytesoftype the caller is compiled for, 0: the one in `bytesoftype` (kernels.h, stenos_k_decode_variant).  (A template
// for the registers' sake as well: as a plain function, called from all four kernels of a unit, it leaves the one for bytesoftype
// 8 a spilled vector register.)
template <uint32_t TT>
WV_FN uint32_t decode_gather_chunk(Lds lds, uint32_t bytesoftype, const uint8_t* frame, uint64_t size, uint64_t total, uint64_t sb, uint64_t s, uint64_t p,
				   const uint8_t* tab, uint32_t count, uint8_t* dst, uint32_t* flag)
{
	const uint32_t T = TT ? TT : bytesoftype;
	if (p > size || size - p < 4) // (written without sums: an index entry may hold anything)
		return GATHER_ST_TRUNCATED;
	const uint32_t code = frame_u8(frame + p);
	const uint32_t csize = frame_u8(frame + p + 1) | (frame_u8(frame + p + 2) << 8) | (frame_u8(frame + p + 3) << 16);
	const uint64_t begin = s * sb;
	if (begin >= total) // (the host's tables: s is a superblock of the frame)
		return GATHER_ST_INVALID;
	const uint32_t dsize = (uint32_t)((total - begin) < sb ? (total - begin) : sb);
	if (size - p - 4 < csize) // stenos.cpp:1133-1134
		return GATHER_ST_TRUNCATED;
	const LanePieces q = load_pieces(tab, count);
	if (ballot((q.lo > q.hi) | (q.hi > U32(dsize)))) // (the fill kernels write no such piece)
		return GATHER_ST_INVALID;
	const uint8_t* payload = frame + p + 4;
	if (code == 1)
		return decode_superblock_pieces(lds, make_dec_layout(T), T, payload, csize, dsize, q, dst) == DEC_ERROR ? GATHER_ST_INVALID : 0u;
	if (code == 6) { // stenos.cpp:741-746
		if (csize != dsize)
			return GATHER_ST_INVALID;
		copy_superblock_pieces(payload, q, dst);
		return 0;
	}
	if (code >= 2 && code <= 5) { // zstd based codes are finished by the host
		gstore_uniform(flag, 1u);
		return GATHER_ST_HOST_CODES;
	}
	return GATHER_ST_INVALID;
}

// ---- what the two translation units share besides (each defines its kernels in its own unnamed namespace) ----
constexpr uint32_t PIECE_THREADS = 256; // of the count and fill kernels: one thread per (row or pair, piece)

// Waves per SIMD gather_decode and gather_batch_decode are compiled for at bytesoftype TT: eight, as decode_superblocks
// (decode_kernels.hip).  The kernel holds one decoder (the LDS-image path; whole superblocks take it too) and the lane's piece in
// four registers across it.  Bytesoftype 4 (the mini-LZ decoder of 32-bit elements is the widest) spills eight registers at
// eight (64 vector registers); at seven it has 72 and spills none.
constexpr uint32_t gather_decode_occupancy(uint32_t TT) { return TT == 4 ? 7 : 8; }

} // namespace codec
#endif
