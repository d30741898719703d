// append_batch_codec.h -- bytes appended in place to many frames in device memory in one call (stenos_hip_append_batch,
// append_batch.h): the argument block of the kernels, and what one thread or one wavefront of each of them does.  The rules are
// append_codec.h's, frame by frame: every step here makes the single call's argument block (AppendArgs) of one frame out of the
// call's tables and runs the single call's function on it -- the index-entry checks (append_plan_thread), the length checks and
// the new index entries (append_commit_plan_at), the chunk copy (append_commit_chunk), the size field
// (append_commit_size_field).  What is new is the numbering: which frame a thread or a wavefront belongs to, where a frame's
// entries lie in the old and in the new index, and the compact tables the host reads.  The kernels (append_batch_kernels.hip)
// and the host emulation (tests/emul_append_batch, with the access audit) run this one copy.  The decode of the partial last
// superblocks is not in here: it is decode_superblock_entry (decode_body.h), called from the kernel file.
// (two include guards, as append_codec.h: append_batch.h takes the argument block alone)
#ifndef STENOS_APPEND_BATCH_ARGS_H
#define STENOS_APPEND_BATCH_ARGS_H
#include <stdint.h>

#define APPEND_ARGS_ONLY
#include "append_codec.h" // AppendArgs, APPEND_W_*, APPEND_PLAN_THREADS, APPEND_COMMIT_*
#undef APPEND_ARGS_ONLY

// Frame f of the call, as the host knows it after the heads have come back.  Its array A_f has `keep` whole superblocks and r more
// bytes; B_f are the caller's bytes.  Its k new superblocks come out of the one encoder pass as one or two streams (AppendArgs):
// the stitched superblock (r > 0: k0 = 1), then the rest of B_f.  The frame of an empty array has one stream, which carries a
// frame header of `start` bytes: its offsets start there, not at 0, and it is written from the frame's first byte (p = 0).
struct AppendBatchFrame {
	uint8_t* frame;       // the frame; only append_batch_commit writes to it
	uint64_t size;        // its bytes before the call
	const uint8_t* src;   // B_f
	uint64_t total;       // bytes of A_f
	uint64_t new_bytes;   // bytes of A_f||B_f: the header's size field
	uint64_t first;       // number of its superblock 0 among the old superblocks of all frames: its old entries start at first + f
	uint64_t first_new;   // the same among the new ones
	uint64_t stitch;      // r > 0: where its stitch slot of r + n0 bytes starts in the stitch buffer
	uint64_t enc_base0;   // where its first stream starts in the encodings ...
	uint64_t enc_base1;   // ... and its second
	uint64_t enc_first;   // the entry of the encoder's offsets its first stream's start at
	uint32_t keep;        // whole superblocks of A_f
	uint32_t r;           // bytes of A_f behind them
	uint32_t k;           // new superblocks (0: nothing is appended, the frame is checked and left alone)
	uint32_t k0;          // of them in the first stream
	uint32_t header;      // bytes of the old frame header
	uint32_t n0;          // r > 0: min(|B_f|, sb - r), the bytes of B_f that fill the stitched superblock
	uint32_t start;       // bytes of the new frame header in front of the stream (the frame of an empty array), else 0
	uint32_t unused;
};

// The old index (the call's own copy) and the new one have the layout of every call over many frames (frame_batch.h).
struct AppendBatchArgs {
	const AppendBatchFrame* frames; // m
	const uint64_t* kpre;    // m + 1: new superblocks of the frames in front of f
	const uint64_t* mpre;    // m + 1: index entries that move unchanged (append_batch_index), of the frames in front of f
	const uint64_t* spre;    // m + 1: stitch chunks of the frames in front of f
	const uint64_t* cpre;    // 2 m + 1: commit chunks in front of stream 2 f + (0: the first, 1: the second) -- the host makes it
	                         // from lens[], after append_batch_commit_plan
	const uint32_t* dec;     // ndec: the frames with r > 0, ascending
	uint64_t* idx;           // S + m: the old frames' entries
	uint64_t* new_idx;       // S' + m: the new frames'
	uint8_t* raw;            // the stitch slots
	const uint8_t* enc;      // the encodings
	const uint64_t* enc_off; // the encoder's offsets
	uint32_t* words;         // APPEND_WORDS for the call (APPEND_W_STATUS), then APPEND_WORDS per frame: zero on entry
	uint32_t* flags;         // m, zero on entry: 1 where the partial last superblock has a zstd-based code
	uint64_t* ends;          // m: k == 0: the end of the frame's chain
	uint64_t* lens;          // 2 m, zero on entry: bytes of the frame's streams
	uint64_t* totals;        // m: bytes of the new frame (k > 0)
	uint32_t m;
	uint32_t ndec;
	uint32_t sb;             // superblock bytes, of every frame
	uint32_t T;
};
#endif

#if !defined(APPEND_BATCH_ARGS_ONLY) && !defined(STENOS_APPEND_BATCH_CODEC_H)
#define STENOS_APPEND_BATCH_CODEC_H
#include "append_codec.h"

namespace codec {

UPD_FN uint32_t* append_batch_words(const AppendBatchArgs& a, uint32_t f) { return a.words + (uint64_t)APPEND_WORDS * (f + 1); }

// The single call's argument block of frame f.  new_layout: idx are the frame's entries of the new index (what
// append_commit_plan writes), else of the old one (what append_plan reads).
UPD_FN AppendArgs append_batch_view(const AppendBatchArgs& a, uint32_t f, bool new_layout)
{
	const AppendBatchFrame& fr = a.frames[f];
	AppendArgs v = AppendArgs();
	v.frame = fr.frame;
	v.size = fr.size;
	v.idx = new_layout ? a.new_idx + fr.first_new + f : a.idx + fr.first + f;
	v.enc = a.enc + fr.enc_base0;
	v.enc_off = a.enc_off + fr.enc_first;
	v.enc_base1 = fr.enc_base1 - fr.enc_base0;
	v.new_bytes = fr.new_bytes;
	v.keep = fr.keep;
	v.r = fr.r;
	v.k = fr.k;
	v.k0 = fr.k0;
	v.header = fr.header;
	v.words = append_batch_words(a, f);
	return v;
}

// ---- append_batch_plan: thread f of the m frames ----
// append_plan_thread on the frame's own entries, size and words: the code byte is read inside that frame only.  A zstd-based
// code is flagged for the frame; a frame nothing is appended to publishes the end of its chain (an entry that has passed the
// checks).  The frame of an empty array has no entry the call uses: its p stays 0, and where nothing is appended its one entry
// of the new index is written here.  Returns UPDATE_ST_* bits for the call's status word.
UPD_FN uint32_t append_batch_plan_thread(const AppendBatchArgs& a, uint32_t f)
{
	const AppendBatchFrame& fr = a.frames[f];
	if (fr.total == 0) {
		if (fr.k == 0) {
			upd_st64(a.new_idx + fr.first_new + f, fr.header);
			upd_st64(a.ends + f, fr.header);
		}
		return 0;
	}
	const AppendArgs v = append_batch_view(a, f, false);
	append_plan_thread(v);
	const uint32_t st = upd_ld32(v.words + APPEND_W_STATUS);
	if (st & UPDATE_ST_HOST_CODES)
		upd_st32(a.flags + f, 1u);
	if (fr.k == 0 && !(st & (UPDATE_ST_TRUNCATED | UPDATE_ST_INVALID)))
		upd_st64(a.ends + f, fr.r ? upd_ld64(v.idx + fr.keep + 1) : append_word64(v.words, APPEND_W_P));
	return st;
}

// ---- append_batch_index: thread x of the entries that move ----
// Old entries 0 .. keep - 1 of a frame (all nsb + 1 of a frame nothing is appended to) go from first + f to first' + f unchanged.
UPD_FN void append_batch_index_thread(const AppendBatchArgs& a, uint64_t x)
{
	if (x >= a.mpre[a.m])
		return;
	const uint32_t f = gather_find64(a.mpre, a.m, x);
	const AppendBatchFrame& fr = a.frames[f];
	const uint64_t e = x - a.mpre[f];
	upd_st64(a.new_idx + fr.first_new + f + e, upd_ld64(a.idx + fr.first + f + e));
}

// ---- append_batch_stitch: wavefront g of the stitch chunks ----
// Chunk c of the first n0 bytes of B_f goes behind the r decoded bytes of the frame's slot: append_commit_chunk, exact bounds on
// both sides, any alignment.
WV_FN void append_batch_stitch_wave(const AppendBatchArgs& a, uint64_t g)
{
	if (g >= a.spre[a.m])
		return;
	const uint32_t f = gather_find64(a.spre, a.m, g);
	const AppendBatchFrame& fr = a.frames[f];
	const uint64_t c = g - a.spre[f];
	if (c < append_commit_chunks(fr.n0))
		append_commit_chunk(a.raw + fr.stitch + fr.r, fr.src, fr.n0, c);
}

// ---- append_batch_commit_plan: thread x of the new superblocks of all frames ----
// append_commit_plan_at for superblock j = x - kpre[f] of frame f, on the frame's entries of the new index; the thread of a
// frame's last new superblock copies the streams' bytes and the new total, which that function has just published in the
// frame's words, into the compact tables the host reads.  Returns UPDATE_ST_* bits.
UPD_FN uint32_t append_batch_commit_plan_thread(const AppendBatchArgs& a, uint64_t x)
{
	if (x >= a.kpre[a.m])
		return 0;
	const uint32_t f = gather_find64(a.kpre, a.m, x);
	const uint32_t j = (uint32_t)(x - a.kpre[f]);
	const AppendArgs v = append_batch_view(a, f, true);
	const uint32_t st = append_commit_plan_at(v, j, a.frames[f].start);
	if (j + 1 == v.k) {
		upd_st64(a.lens + 2 * (uint64_t)f, append_word64(v.words, APPEND_W_LEN0));
		upd_st64(a.lens + 2 * (uint64_t)f + 1, append_word64(v.words, APPEND_W_LEN1));
		upd_st64(a.totals + f, append_word64(v.words, APPEND_W_TOTAL));
	}
	return st;
}

// ---- append_batch_commit: wavefront g of the commit chunks, the only writer to the frames ----
// The streams of all frames are cut into chunks of APPEND_COMMIT_CHUNK bytes; chunk g belongs to the stream it falls into in
// cpre, and goes to its place behind the frame's p.  The wavefront of the first chunk of a frame also stores the 7 size bytes.
// All offsets are 64-bit.  (append_batch_commit_plan has checked every length, the host every capacity.)
// (chunk g: stream *s = 2 f + (0: the first, 1: the second) of frame f, chunk *c of it; false: behind the last chunk)
UPD_FN bool append_batch_commit_chunk_of(const AppendBatchArgs& a, uint64_t g, uint32_t* s, uint64_t* c)
{
	if (g >= a.cpre[2 * (uint64_t)a.m])
		return false;
	*s = gather_find64(a.cpre, 2 * a.m, g);
	*c = g - a.cpre[*s];
	return true;
}
// the 7 size bytes, by the wavefront of the first chunk of the frame
WV_FN void append_batch_commit_size_field(const AppendBatchArgs& a, uint32_t s, uint64_t c)
{
	if (c == 0 && (!(s & 1u) || upd_ld64(a.lens + (s - 1u)) == 0))
		append_commit_size_field(append_batch_view(a, s >> 1, true));
}
WV_FN void append_batch_commit_copy(const AppendBatchArgs& a, uint32_t s, uint64_t c)
{
	const uint32_t f = s >> 1;
	const AppendArgs v = append_batch_view(a, f, true);
	const uint64_t p = append_word64(v.words, APPEND_W_P), len0 = upd_ld64(a.lens + 2 * (uint64_t)f), len1 = upd_ld64(a.lens + 2 * (uint64_t)f + 1);
	const bool second = s & 1u;
	const uint64_t len = second ? len1 : len0;
	if (c < append_commit_chunks(len))
		append_commit_chunk(v.frame + p + (second ? len0 : 0), v.enc + (second ? v.enc_base1 : 0), len, c);
}
WV_FN void append_batch_commit_wave(const AppendBatchArgs& a, uint64_t g)
{
	uint32_t s;
	uint64_t c;
	if (!append_batch_commit_chunk_of(a, g, &s, &c))
		return;
	append_batch_commit_size_field(a, s, c);
	append_batch_commit_copy(a, s, c);
}

} // namespace codec
#endif
