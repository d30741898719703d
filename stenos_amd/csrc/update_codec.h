// update_codec.h -- rows of one frame replaced by row number (stenos_hip_update_rows, update.h): the argument block of the
// kernels, and what one thread or one wavefront of each of them does.  The planning steps are plain C++ over runs of
// superblocks, the copies are written in the wavevec.h vocabulary: the kernels (update_kernels.hip) and the host emulation
// (tests/emul_update, with the access audit) run this one copy.  update_decode is not in here: it is decode_superblock_entry
// (decode_body.h), called from the kernel file.
// (two include guards, as gather_codec.h: update.h takes the argument block alone)
#ifndef STENOS_UPDATE_ARGS_H
#define STENOS_UPDATE_ARGS_H
#include <stdint.h>

#define GATHER_CUT_ONLY
#include "gather_codec.h" // GatherPiece
#undef GATHER_CUT_ONLY

constexpr uint32_t UPDATE_NO_SLOT = 0xFFFFFFFFu;
// words the kernels share with the host (the first 64 bytes of the update's table buffer, zero on entry)
enum : uint32_t {
	UPDATE_W_STATUS = 0, // DECODE_STATUS_* of the call
	UPDATE_W_K = 1,      // touched superblocks
	UPDATE_W_LAST = 2,   // the largest touched superblock number
	UPDATE_W_TOTAL = 4,  // (64 bits, words 4 and 5) bytes of the new frame
	UPDATE_WORDS = 16,
};
// wavefronts that apply the pieces of one touched superblock: a piece belongs to the wavefront its offset in the superblock
// hashes to, so that the sources of a repeated row meet in one wavefront, which takes them one after the other
constexpr uint32_t UPDATE_APPLY_WAVES = 8;
// wavefronts (of one workgroup) that copy one superblock in update_splice
constexpr uint32_t UPDATE_SPLICE_WAVES = 4;
// threads of the one workgroup of update_plan and of update_splice_plan
constexpr uint32_t UPDATE_PLAN_THREADS = 1024;

struct UpdateArgs {
	const uint8_t* frame;     // the old frame
	uint64_t size;            // its bytes
	const uint64_t* idx;      // nsb + 1 header offsets of the old frame (the update's own copy)
	uint64_t* new_idx;        // nsb + 1 header offsets of the new frame
	const uint8_t* enc;       // the touched superblocks, encoded again, back to back
	const uint64_t* enc_off;  // k + 1 offsets into enc
	const uint8_t* src;       // source rows
	uint8_t* raw;             // decoded touched superblocks: slot c at c * sb
	uint8_t* out;             // the new frame
	uint64_t total;           // bytes of the original array
	uint32_t sb;              // superblock bytes
	uint32_t nsb;
	uint32_t T;
	uint32_t header;          // frame header bytes
	uint32_t k;               // touched superblocks (update_plan tells the host)
	uint32_t* words;          // UPDATE_W_*
	const uint32_t* ppre;     // nsb + 1: pieces in front of superblock s (gather_scan)
	uint32_t* slot;           // nsb
	uint32_t* touched;        // min(nsb, pieces)
	uint32_t* flags;          // nsb, zero on entry: 1 where a touched superblock has a zstd-based code
	const codec::GatherPiece* pieces;
};
#endif

#if !defined(UPDATE_ARGS_ONLY) && !defined(STENOS_UPDATE_CODEC_H)
#define STENOS_UPDATE_CODEC_H
#include "gather_codec.h" // load_pieces, copy_g2g_wide (range_codec.h)

namespace codec {

// DECODE_STATUS_* (kernels.h, which the emulation cannot include; update_kernels.hip asserts that they are the same)
enum : uint32_t { UPDATE_ST_TRUNCATED = 1, UPDATE_ST_INVALID = 2, UPDATE_ST_HOST_CODES = 4 };
// a superblock in a frame: its 4-byte header and a payload whose size the header holds in three bytes
constexpr uint64_t UPDATE_MAX_SB_FRAME_BYTES = 4 + 0xFFFFFFull;

// what one thread does with words of its own (the emulation's accessors are the audited ones)
#ifdef WV_HOST_EMULATION
#define UPD_FN static inline
UPD_FN uint32_t upd_ld8(const uint8_t* p) { return wv::gload_uniform8(p); }
UPD_FN uint32_t upd_ld32(const uint32_t* p) { return wv::gload_uniform(p); }
UPD_FN uint64_t upd_ld64(const uint64_t* p) { return wv::gload_uniform64(p); }
UPD_FN void upd_st32(uint32_t* p, uint32_t v) { wv::gstore_uniform(p, v); }
UPD_FN void upd_st64(uint64_t* p, uint64_t v) { wv::gstore_uniform64(p, v); }
#else
#define UPD_FN static __device__ __forceinline__
UPD_FN uint32_t upd_ld8(const uint8_t* p) { return *p; }
UPD_FN uint32_t upd_ld32(const uint32_t* p) { return *p; }
UPD_FN uint64_t upd_ld64(const uint64_t* p) { return *p; }
UPD_FN void upd_st32(uint32_t* p, uint32_t v) { *p = v; }
UPD_FN void upd_st64(uint64_t* p, uint64_t v) { *p = v; }
#endif

// the run of superblocks of thread k of the one-workgroup kernels update_plan and update_splice_plan (gather_scan's)
UPD_FN void update_run_of_thread(uint32_t nsb, uint32_t k, uint32_t* begin, uint32_t* end)
{
	const uint32_t run = (nsb + UPDATE_PLAN_THREADS - 1) / UPDATE_PLAN_THREADS;
	const uint64_t b0 = (uint64_t)k * run, e0 = b0 + run;
	*begin = (uint32_t)(b0 < nsb ? b0 : nsb);
	*end = (uint32_t)(e0 < nsb ? e0 : nsb);
}

// ---- update_plan: a thread's run [begin, end) of superblocks ----
// the touched superblocks among them
UPD_FN uint32_t update_plan_count(const UpdateArgs& a, uint32_t begin, uint32_t end)
{
	uint32_t t = 0;
	for (uint32_t s = begin; s < end; ++s)
		t += upd_ld32(a.ppre + s + 1) > upd_ld32(a.ppre + s);
	return t;
}
// c touched superblocks stand in front of the run: slot and touched, the flags of zstd-based codes.  Returns UPDATE_ST_* bits;
// *last: the largest touched superblock of the run (not written when there is none).
UPD_FN uint32_t update_plan_write(const UpdateArgs& a, uint32_t begin, uint32_t end, uint32_t c, uint32_t* last)
{
	uint32_t st = 0;
	for (uint32_t s = begin; s < end; ++s) {
		if (upd_ld32(a.ppre + s + 1) == upd_ld32(a.ppre + s)) {
			upd_st32(a.slot + s, UPDATE_NO_SLOT);
			continue;
		}
		upd_st32(a.slot + s, c);
		upd_st32(a.touched + c, s);
		++c;
		*last = s;
		const uint64_t p = upd_ld64(a.idx + s);
		if (p > a.size || a.size - p < 4) { // (written without sums: an index entry may hold anything)
			st |= UPDATE_ST_TRUNCATED;
			continue;
		}
		const uint32_t code = upd_ld8(a.frame + p);
		if (code >= 2 && code <= 5) { // the host decodes it (update_decode passes it over)
			upd_st32(a.flags + s, 1u);
			st |= UPDATE_ST_HOST_CODES;
		}
	}
	return st;
}

// ---- update_splice_plan: a thread's run [begin, end) of superblocks ----
// Bytes superblock s takes in the new frame.  The old index is checked for every superblock, touched or not: offsets must
// not decrease, a superblock has its header at least and at most the payload a header can announce, and the last entry
// lies inside the frame -- so every untouched superblock that update_splice copies lies inside [frame, frame + size).
UPD_FN uint64_t update_new_length(const UpdateArgs& a, uint32_t s, uint32_t* st)
{
	const uint64_t p = upd_ld64(a.idx + s), q = upd_ld64(a.idx + s + 1);
	if (q < p || q - p < 4 || q - p > UPDATE_MAX_SB_FRAME_BYTES) {
		*st |= UPDATE_ST_INVALID;
		return 0;
	}
	if (s + 1 == a.nsb && q > a.size) {
		*st |= UPDATE_ST_TRUNCATED;
		return 0;
	}
	const uint32_t c = upd_ld32(a.slot + s);
	if (c == UPDATE_NO_SLOT)
		return q - p;
	const uint64_t e0 = upd_ld64(a.enc_off + c), e1 = upd_ld64(a.enc_off + c + 1);
	if (e1 < e0 || e1 - e0 < 4 || e1 - e0 > UPDATE_MAX_SB_FRAME_BYTES) { // (the encoder writes no such offsets)
		*st |= UPDATE_ST_INVALID;
		return 0;
	}
	return e1 - e0;
}
UPD_FN uint64_t update_splice_sum(const UpdateArgs& a, uint32_t begin, uint32_t end, uint32_t* st)
{
	uint64_t sum = 0;
	for (uint32_t s = begin; s < end; ++s)
		sum += update_new_length(a, s, st);
	return sum;
}
// `at`: where the run's first superblock stands in the new frame; returns the end of its last
UPD_FN uint64_t update_splice_write(const UpdateArgs& a, uint32_t begin, uint32_t end, uint64_t at)
{
	uint32_t st = 0;
	for (uint32_t s = begin; s < end; ++s) {
		upd_st64(a.new_idx + s, at);
		at += update_new_length(a, s, &st);
	}
	return at;
}

// ---- update_apply: wavefront w (of UPDATE_APPLY_WAVES) of the touched superblock in place c ----
// The wavefront a piece belongs to, from its first byte's offset in the superblock.  The pieces of one superblock that start
// at the same byte are the same piece of the same row, named more than once: they meet in one wavefront.
WV_FN U32 update_apply_wave_of(const U32& lo) { return (lo * U32(2654435761u)) >> U32(29u); }
static_assert(UPDATE_APPLY_WAVES == 8, "update_apply_wave_of keeps three bits");

// All pieces of the superblock pass by, 64 at a time; those of this wavefront are copied one after the other, in the order
// of the table: source bytes [d, d + hi - lo) -> bytes [lo, hi) of the slot.  A wavefront's stores complete in order
// (wavevec.h, gst128_streamed), so where pieces repeat the last one of the table stands whole.  No byte outside a piece's
// source bytes is read, none outside [lo, hi) of the slot written; a piece that does not lie inside the superblock
// (gather_fill writes none) is passed over.
WV_FN void update_apply_wave(const UpdateArgs& a, uint32_t c, uint32_t w)
{
	const uint32_t s = upd_ld32(a.touched + c);
	const uint32_t first = upd_ld32(a.ppre + s), end = upd_ld32(a.ppre + s + 1);
	const uint64_t begin = (uint64_t)s * a.sb;
	const uint32_t dsize = (uint32_t)(a.total - begin < a.sb ? a.total - begin : a.sb);
	uint8_t* const slot = a.raw + (uint64_t)c * a.sb;
	for (uint32_t at = first; at < end; at += 64) {
		const uint32_t left = end - at;
		const LanePieces q = load_pieces((const uint8_t*)(a.pieces + at), left < 64u ? left : 64u);
		const Pred mine = (q.hi > q.lo) & (q.hi <= U32(dsize)) & (update_apply_wave_of(q.lo) == U32(w));
		for (uint64_t m = ballot(mine); m; m &= m - 1) {
			const uint32_t l = (uint32_t)__builtin_ctzll(m);
			const uint32_t plo = readlane(q.lo, l);
			const uint64_t d = (uint64_t)readlane(q.dlo, l) | ((uint64_t)readlane(q.dhi, l) << 32);
			copy_g2g_wide<COPY_ROUNDS>(slot + plo, a.src + d, readlane(q.hi, l) - plo);
		}
	}
}

// ---- update_splice: wavefront w (of UPDATE_SPLICE_WAVES) of the workgroup of superblock s ----
// The superblock's bytes in the new frame come from the encoded stream (touched) or from the old frame, in
// UPDATE_SPLICE_WAVES parts of a multiple of 16 bytes; wavefront 0 of workgroup 0 copies the frame header as well.  Exact
// bounds on both sides (copy_g2g_wide), any alignment.  (update_splice_plan has checked every length.)
WV_FN void update_splice_wave(const UpdateArgs& a, uint32_t s, uint32_t w)
{
	if (s == 0 && w == 0)
		copy_g2g_wide<COPY_ROUNDS>(a.out, a.frame, a.header);
	if (s >= a.nsb)
		return;
	const uint64_t n0 = upd_ld64(a.new_idx + s);
	const uint32_t len = (uint32_t)(upd_ld64(a.new_idx + s + 1) - n0);
	const uint32_t c = upd_ld32(a.slot + s);
	const uint8_t* const from = c == UPDATE_NO_SLOT ? a.frame + upd_ld64(a.idx + s) : a.enc + upd_ld64(a.enc_off + c);
	const uint32_t part = ((len + UPDATE_SPLICE_WAVES - 1) / UPDATE_SPLICE_WAVES + 15u) & ~15u;
	const uint32_t lo = w * part < len ? w * part : len, hi = len - lo < part ? len : lo + part;
	if (hi > lo)
		copy_g2g_wide<COPY_ROUNDS>(a.out + n0 + lo, from + lo, hi - lo);
}

} // namespace codec
#endif
