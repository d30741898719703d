// update_codec.h -- rows of one frame replaced by row number (stenos_hip_update_rows, update.h): the argument block of the
// kernels, and what one thread or one wavefront of each of them does.  The planning steps are plain C++ over runs of
// superblocks, the copies are written in the wavevec.h vocabulary: the kernels (update_kernels.hip) and the host emulation
// (tests/emul_update, with the access audit) run this one copy.  update_decode is not in here: it is decode_superblock_entry
// (decode_body.h), called from the kernel file.
// The forms for many frames in one call (stenos_hip_update_rows_batch, update_batch.h: UpdateBatchArgs and update_batch_*) stand
// beside the single ones; what does not depend on the numbering of the superblocks is one function for both
// (update_run_of_thread, update_plan_count, update_apply_pieces, update_splice_part).  update_batch_kernels.hip and
// tests/emul_update_batch run them.
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

// ---- rows of many frames in one call (stenos_hip_update_rows_batch, update_batch.h) ----
// The superblocks of all frames are numbered through (gather_codec.h, GatherFrame: g = first_f + s) and every table of the
// single call is indexed by g; the two indices have the layout of every call over many frames (frame_batch.h): the header of
// superblock g of frame f is entry g + f, frame f's end entry first[f + 1] + f.  All frames have superblocks of `sb` bytes.
// words: UPDATE_W_STATUS and UPDATE_W_K (the touched superblocks of all frames) as above.
struct UpdateBatchArgs {
	const codec::GatherFrame* frames; // m entries: pointer, bytes, array bytes, first, nsb
	const uint64_t* first;    // m + 1: first[f] = frames[f].first, first[m] = S
	const uint64_t* header;   // m: frame header bytes
	uint8_t* const* outs;     // m: the new frames
	const uint64_t* idx;      // S + m header offsets of the old frames (the update's own copy)
	uint64_t* new_idx;        // S + m header offsets of the new frames
	uint64_t* gpre;           // S + 1: bytes the superblocks in front of g take in the new frames, over all frames
	uint64_t* totals;         // m: bytes of the new frames
	const uint8_t* enc;       // the touched superblocks, encoded again: frame f's stream at enc + enc_base[f]
	const uint64_t* enc_base; // m
	const uint64_t* enc_off;  // K + m offsets into the frames' streams: those of frame f's k_f superblocks start at entry c_f + f,
	                          // c_f = the place of its first touched superblock in the compact list
	const uint8_t* src;       // source rows
	uint8_t* raw;             // decoded touched superblocks: slot c at c * sb
	uint32_t sb;              // superblock bytes, of every frame
	uint32_t m;
	uint32_t S;               // superblocks of all frames
	uint32_t T;
	uint32_t K;               // touched superblocks of all frames (update_batch_plan tells the host)
	uint32_t* words;          // UPDATE_W_*
	const uint32_t* ppre;     // S + 1: pieces in front of superblock g (gather_scan)
	uint32_t* slot;           // S
	uint32_t* touched;        // min(S, pieces): ascending, so a frame's touched superblocks are one run of the list
	uint32_t* flags;          // S, zero on entry: 1 where a touched superblock has a zstd-based code
	uint32_t* kf;             // 2 m, zero on entry: (k_f, the largest touched superblock number of frame f) for the host
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
UPD_FN void upd_add32(uint32_t* p, uint32_t v) { wv::gstore_uniform(p, wv::gload_uniform(p) + v); } // (the threads run one after the other)
UPD_FN void upd_max32(uint32_t* p, uint32_t v) { wv::gstore_uniform(p, wv::gload_uniform(p) > v ? wv::gload_uniform(p) : v); }
#else
#define UPD_FN static __device__ __forceinline__
UPD_FN uint32_t upd_ld8(const uint8_t* p) { return *p; }
UPD_FN uint32_t upd_ld32(const uint32_t* p) { return *p; }
UPD_FN uint64_t upd_ld64(const uint64_t* p) { return *p; }
UPD_FN void upd_st32(uint32_t* p, uint32_t v) { *p = v; }
UPD_FN void upd_st64(uint64_t* p, uint64_t v) { *p = v; }
UPD_FN void upd_add32(uint32_t* p, uint32_t v) { atomicAdd(p, v); }
UPD_FN void upd_max32(uint32_t* p, uint32_t v) { atomicMax(p, v); }
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
// the touched superblocks among them (A: UpdateArgs, or UpdateBatchArgs with the batch's numbering)
template <class A>
UPD_FN uint32_t update_plan_count(const A& a, uint32_t begin, uint32_t end)
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
// (pieces [first, end) of the table are the superblock's, which decodes to dsize bytes at `slot`)
WV_FN void update_apply_pieces(const GatherPiece* pieces, uint32_t first, uint32_t end, uint32_t dsize, uint8_t* slot, const uint8_t* src, uint32_t w)
{
	for (uint32_t at = first; at < end; at += 64) {
		const uint32_t left = end - at;
		const LanePieces q = load_pieces((const uint8_t*)(pieces + at), left < 64u ? left : 64u);
		const Pred mine = (q.hi > q.lo) & (q.hi <= U32(dsize)) & (update_apply_wave_of(q.lo) == U32(w));
		for (uint64_t m = ballot(mine); m; m &= m - 1) {
			const uint32_t l = (uint32_t)__builtin_ctzll(m);
			const uint32_t plo = readlane(q.lo, l);
			const uint64_t d = (uint64_t)readlane(q.dlo, l) | ((uint64_t)readlane(q.dhi, l) << 32);
			copy_g2g_wide<COPY_ROUNDS>(slot + plo, src + d, readlane(q.hi, l) - plo);
		}
	}
}
WV_FN void update_apply_wave(const UpdateArgs& a, uint32_t c, uint32_t w)
{
	const uint32_t s = upd_ld32(a.touched + c);
	const uint32_t first = upd_ld32(a.ppre + s), end = upd_ld32(a.ppre + s + 1);
	const uint64_t begin = (uint64_t)s * a.sb;
	const uint32_t dsize = (uint32_t)(a.total - begin < a.sb ? a.total - begin : a.sb);
	update_apply_pieces(a.pieces, first, end, dsize, a.raw + (uint64_t)c * a.sb, a.src, w);
}

// ---- update_splice: wavefront w (of UPDATE_SPLICE_WAVES) of the workgroup of superblock s ----
// The superblock's bytes in the new frame come from the encoded stream (touched) or from the old frame, in
// UPDATE_SPLICE_WAVES parts of a multiple of 16 bytes; wavefront 0 of workgroup 0 copies the frame header as well.  Exact
// bounds on both sides (copy_g2g_wide), any alignment.  (update_splice_plan has checked every length.)
// (wavefront w's part of the len bytes at `from` -> `to`)
WV_FN void update_splice_part(uint8_t* to, const uint8_t* from, uint32_t len, uint32_t w)
{
	const uint32_t part = ((len + UPDATE_SPLICE_WAVES - 1) / UPDATE_SPLICE_WAVES + 15u) & ~15u;
	const uint32_t lo = w * part < len ? w * part : len, hi = len - lo < part ? len : lo + part;
	if (hi > lo)
		copy_g2g_wide<COPY_ROUNDS>(to + lo, from + lo, hi - lo);
}
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
	update_splice_part(a.out + n0, from, len, w);
}

// ---- many frames in one call: the same rules on the batch's numbering (UpdateBatchArgs) ----
// update_batch_plan, a thread's run [begin, end) of the S superblocks: update_plan_count above, then, c touched superblocks
// standing in front of the run: slot and touched, per frame k_f and its largest touched superblock, the flags of zstd-based codes.
// The code byte is read inside its own frame only.  Returns UPDATE_ST_* bits.
UPD_FN uint32_t update_batch_plan_write(const UpdateBatchArgs& a, uint32_t begin, uint32_t end, uint32_t c)
{
	uint32_t st = 0;
	for (uint32_t g = begin; g < end; ++g) {
		if (upd_ld32(a.ppre + g + 1) == upd_ld32(a.ppre + g)) {
			upd_st32(a.slot + g, UPDATE_NO_SLOT);
			continue;
		}
		upd_st32(a.slot + g, c);
		upd_st32(a.touched + c, g);
		++c;
		const uint32_t f = gather_find64(a.first, a.m, g);
		const GatherFrame& fr = a.frames[f];
		upd_add32(a.kf + 2 * f, 1u);
		upd_max32(a.kf + 2 * f + 1, (uint32_t)(g - fr.first));
		const uint64_t p = upd_ld64(a.idx + (uint64_t)g + f);
		if (p > fr.size || fr.size - p < 4) { // (written without sums: an index entry may hold anything)
			st |= UPDATE_ST_TRUNCATED;
			continue;
		}
		const uint32_t code = upd_ld8(fr.frame + p);
		if (code >= 2 && code <= 5) { // the host decodes it (update_batch_decode passes it over)
			upd_st32(a.flags + g, 1u);
			st |= UPDATE_ST_HOST_CODES;
		}
	}
	return st;
}

// update_batch_splice_plan.  Bytes superblock g takes in its new frame: update_new_length's rule, frame by frame -- the old
// index of frame f is checked against that frame's size, so an entry that points into another frame's slice is refused as one that
// points anywhere else outside its own.
UPD_FN uint64_t update_batch_new_length(const UpdateBatchArgs& a, uint32_t g, uint32_t* st)
{
	const uint32_t f = gather_find64(a.first, a.m, g);
	const uint64_t p = upd_ld64(a.idx + (uint64_t)g + f), q = upd_ld64(a.idx + (uint64_t)g + f + 1);
	if (q < p || q - p < 4 || q - p > UPDATE_MAX_SB_FRAME_BYTES) {
		*st |= UPDATE_ST_INVALID;
		return 0;
	}
	if ((uint64_t)g + 1 == a.first[f + 1] && q > a.frames[f].size) {
		*st |= UPDATE_ST_TRUNCATED;
		return 0;
	}
	const uint32_t c = upd_ld32(a.slot + g);
	if (c == UPDATE_NO_SLOT)
		return q - p;
	const uint64_t e0 = upd_ld64(a.enc_off + (uint64_t)c + f), e1 = upd_ld64(a.enc_off + (uint64_t)c + f + 1);
	if (e1 < e0 || e1 - e0 < 4 || e1 - e0 > UPDATE_MAX_SB_FRAME_BYTES) { // (the encoder writes no such offsets)
		*st |= UPDATE_ST_INVALID;
		return 0;
	}
	return e1 - e0;
}
// a thread's run [begin, end): the bytes its superblocks take ...
UPD_FN uint64_t update_batch_splice_sum(const UpdateBatchArgs& a, uint32_t begin, uint32_t end, uint32_t* st)
{
	uint64_t sum = 0;
	for (uint32_t g = begin; g < end; ++g)
		sum += update_batch_new_length(a, g, st);
	return sum;
}
// ... gpre over the run, `at` bytes standing in front of it over all frames; returns the end of its last superblock ...
UPD_FN uint64_t update_batch_splice_write(const UpdateBatchArgs& a, uint32_t begin, uint32_t end, uint64_t at)
{
	uint32_t st = 0;
	for (uint32_t g = begin; g < end; ++g) {
		upd_st64(a.gpre + g, at);
		at += update_batch_new_length(a, g, &st);
	}
	return at;
}
// ... and, once gpre is whole (gpre[S] included): the sums start again at every frame's header size
UPD_FN void update_batch_splice_index(const UpdateBatchArgs& a, uint32_t begin, uint32_t end)
{
	for (uint32_t g = begin; g < end; ++g) {
		const uint32_t f = gather_find64(a.first, a.m, g);
		upd_st64(a.new_idx + (uint64_t)g + f, a.header[f] + upd_ld64(a.gpre + g) - upd_ld64(a.gpre + a.first[f]));
	}
}
// frame f's end entry and its new size (the frame of an empty array: its header, which is all of it)
UPD_FN void update_batch_splice_total(const UpdateBatchArgs& a, uint32_t f)
{
	const uint64_t total = a.header[f] + upd_ld64(a.gpre + a.first[f + 1]) - upd_ld64(a.gpre + a.first[f]);
	upd_st64(a.new_idx + a.first[f + 1] + f, total);
	upd_st64(a.totals + f, total);
}

// update_batch_apply: wavefront w (of UPDATE_APPLY_WAVES) of the touched superblock in place c
WV_FN void update_batch_apply_wave(const UpdateBatchArgs& a, uint32_t c, uint32_t w)
{
	const uint32_t g = upd_ld32(a.touched + c);
	const uint32_t f = gather_find64(a.first, a.m, g);
	const uint32_t first = upd_ld32(a.ppre + g), end = upd_ld32(a.ppre + g + 1);
	const uint64_t begin = (g - a.first[f]) * (uint64_t)a.sb, total = a.frames[f].total;
	const uint32_t dsize = (uint32_t)(total - begin < a.sb ? total - begin : a.sb);
	update_apply_pieces(a.pieces, first, end, dsize, a.raw + (uint64_t)c * a.sb, a.src, w);
}

// update_batch_splice: wavefront w (of UPDATE_SPLICE_WAVES) of workgroup x.  x < S: superblock x of the batch to its place in
// its frame's output, from the frame's encoded stream (touched) or from the old frame; S <= x < S + m: wavefront 0 copies the
// header of frame x - S.  (update_batch_splice_plan has checked every length.)
WV_FN void update_batch_splice_wave(const UpdateBatchArgs& a, uint32_t x, uint32_t w)
{
	if (x >= a.S) {
		const uint32_t f = x - a.S;
		if (f < a.m && w == 0)
			copy_g2g_wide<COPY_ROUNDS>(a.outs[f], a.frames[f].frame, (uint32_t)a.header[f]);
		return;
	}
	const uint32_t f = gather_find64(a.first, a.m, x);
	const uint64_t n0 = upd_ld64(a.new_idx + (uint64_t)x + f);
	const uint32_t len = (uint32_t)(upd_ld64(a.new_idx + (uint64_t)x + f + 1) - n0);
	const uint32_t c = upd_ld32(a.slot + x);
	const uint8_t* const from =
		c == UPDATE_NO_SLOT ? a.frames[f].frame + upd_ld64(a.idx + (uint64_t)x + f) : a.enc + a.enc_base[f] + upd_ld64(a.enc_off + (uint64_t)c + f);
	update_splice_part(a.outs[f] + n0, from, len, w);
}

} // namespace codec
#endif
