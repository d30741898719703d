// append_codec.h -- bytes appended in place to a frame in device memory (stenos_hip_append, append.h): the argument block of
// the kernels, and what one thread or one wavefront of each of them does.  The planning steps are plain C++ in the UPD_FN
// vocabulary of update_codec.h, the copy is written in the wavevec.h vocabulary: the kernels (append_kernels.hip) and the host
// emulation (tests/emul_append, with the access audit) run this one copy.  The decode of the partial last superblock is not
// in here: it is decode_superblock_entry (decode_body.h), called from the kernel file.
// (two include guards, as update_codec.h: append.h takes the argument block alone)
#ifndef STENOS_APPEND_ARGS_H
#define STENOS_APPEND_ARGS_H
#include <stdint.h>

// words the kernels share with the host (the first 64 bytes of the append's table buffer, zero on entry)
enum : uint32_t {
	APPEND_W_STATUS = 0, // DECODE_STATUS_* of the call
	APPEND_W_P = 2,      // (64 bits, words 2 and 3) offset of the header of superblock `keep`: where the new stream starts
	APPEND_W_TOTAL = 4,  // (64 bits, words 4 and 5) bytes of the new frame
	APPEND_W_LEN0 = 6,   // (64 bits) bytes of the first encoded stream
	APPEND_W_LEN1 = 8,   // (64 bits) bytes of the second
	APPEND_WORDS = 16,
};
// threads of a workgroup of append_commit_plan (one thread per new superblock)
constexpr uint32_t APPEND_PLAN_THREADS = 256;
// wavefronts of a workgroup of append_commit, and the bytes of a stream one wavefront copies
constexpr uint32_t APPEND_COMMIT_WAVES = 4;
constexpr uint32_t APPEND_COMMIT_CHUNK = 16384;

// The array A of `keep` whole superblocks and r more bytes grows by the caller's bytes B.  The k new superblocks, which hold
// (last r bytes of A)||B, come out of one encoder pass as one or two streams without a frame header: the first of k0
// superblocks (with r > 0 the stitched superblock, k0 = 1; else k0 = 0), the second of the k - k0 others, read straight from
// B.  The encoder's offsets of a stream count from the stream's start; those of the first stream are entries [0, k0] of
// enc_off, those of the second stand behind them.
struct AppendArgs {
	uint8_t* frame;          // the frame; only append_commit writes to it
	uint64_t size;           // its bytes before the call
	uint64_t* idx;           // the call's own index: the old frame's entries on entry, entries [keep, keep + k] of the new frame from append_commit_plan
	const uint8_t* enc;      // the encoded streams: the first at enc, the second at enc + enc_base1
	const uint64_t* enc_off; // the encoder's offsets
	uint64_t enc_base1;
	uint64_t new_bytes;      // bytes of the array after the call: the header's size field
	uint32_t keep;           // whole superblocks of A: they stay where and what they are
	uint32_t r;              // bytes of A behind them
	uint32_t k;              // new superblocks (the host knows it from the sizes)
	uint32_t k0;             // of them in the first stream
	uint32_t header;         // frame header bytes
	uint32_t* words;         // APPEND_W_*
};
#endif

#if !defined(APPEND_ARGS_ONLY) && !defined(STENOS_APPEND_CODEC_H)
#define STENOS_APPEND_CODEC_H
#include "update_codec.h" // UPD_FN and the upd_* accessors, UPDATE_ST_*, UPDATE_MAX_SB_FRAME_BYTES, copy_g2g_wide

namespace codec {

UPD_FN uint64_t append_word64(const uint32_t* words, uint32_t w) { return (uint64_t)upd_ld32(words + w) | ((uint64_t)upd_ld32(words + w + 1) << 32); }
UPD_FN void append_set_word64(uint32_t* words, uint32_t w, uint64_t v)
{
	upd_st32(words + w, (uint32_t)v);
	upd_st32(words + w + 1, (uint32_t)(v >> 32));
}

// ---- append_plan: one thread ----
// The two index entries the call uses, checked without sums (an entry may hold anything): header <= idx[keep]; with a partial
// last superblock idx[keep] + 4 <= idx[keep + 1] <= size, else idx[keep] <= size.  Only then is the code byte of superblock
// `keep` read, inside the frame; a zstd-based code is left to the host.  Publishes p = idx[keep] and the status bits.
UPD_FN void append_plan_thread(const AppendArgs& a)
{
	const uint64_t p = upd_ld64(a.idx + a.keep);
	uint32_t st = 0;
	if (p < a.header)
		st = UPDATE_ST_INVALID;
	else if (a.r == 0)
		st = p > a.size ? UPDATE_ST_TRUNCATED : 0u;
	else {
		const uint64_t q = upd_ld64(a.idx + a.keep + 1);
		if (q < p || q - p < 4)
			st = UPDATE_ST_INVALID;
		else if (q > a.size)
			st = UPDATE_ST_TRUNCATED;
		else {
			const uint32_t code = upd_ld8(a.frame + p);
			if (code >= 2 && code <= 5) // the host decodes it (append_decode passes it over)
				st = UPDATE_ST_HOST_CODES;
		}
	}
	append_set_word64(a.words, APPEND_W_P, p);
	if (st)
		upd_st32(a.words + APPEND_W_STATUS, upd_ld32(a.words + APPEND_W_STATUS) | st); // (the walk may have left a bit; one thread runs)
}

// ---- append_commit_plan: thread j of the k new superblocks ----
// Superblock keep + j of the new frame stands at p + (bytes of the new stream in front of it): the encoder's offsets are sums
// already, so every thread finds its own place.  Every length is checked as update_new_length checks the encoder's (a
// superblock has its header at least, and at most the payload a header can announce; a stream's offsets start at 0), the
// last thread publishes both streams' bytes and the new total.  Returns UPDATE_ST_* bits.
// (start: where the offsets of the first stream that has superblocks start -- 0 for a stream without a frame header, which is
// all stenos_hip_append has; the many-frame call hands in a stream with one, append_batch_codec.h)
UPD_FN uint32_t append_commit_plan_at(const AppendArgs& a, uint32_t j, uint64_t start)
{
	if (j >= a.k)
		return 0;
	const uint64_t p = append_word64(a.words, APPEND_W_P);
	const uint64_t len0 = a.k0 ? upd_ld64(a.enc_off + a.k0) : 0;
	const bool second = j >= a.k0;
	const uint64_t* const e = second ? a.enc_off + (a.k0 ? a.k0 + 1 : 0) + (j - a.k0) : a.enc_off + j;
	const uint64_t e0 = upd_ld64(e), e1 = upd_ld64(e + 1);
	uint32_t st = 0;
	if (e1 < e0 || e1 - e0 < 4 || e1 - e0 > UPDATE_MAX_SB_FRAME_BYTES) // (the encoder writes no such offsets)
		st = UPDATE_ST_INVALID;
	if ((j == 0 || j == a.k0) && e0 != (j == 0 ? start : 0))
		st = UPDATE_ST_INVALID;
	const uint64_t base = p + (second ? len0 : 0);
	upd_st64(a.idx + a.keep + j, base + e0);
	if (j + 1 == a.k) {
		upd_st64(a.idx + a.keep + a.k, base + e1);
		append_set_word64(a.words, APPEND_W_TOTAL, base + e1);
		append_set_word64(a.words, APPEND_W_LEN0, second ? len0 : e1);
		append_set_word64(a.words, APPEND_W_LEN1, second ? e1 : 0);
	}
	return st;
}
UPD_FN uint32_t append_commit_plan_thread(const AppendArgs& a, uint32_t j) { return append_commit_plan_at(a, j, 0); }

// ---- append_commit: wavefront g of the grid, the only writer to the frame ----
// The two streams are cut into chunks of APPEND_COMMIT_CHUNK bytes, the first stream's first; wavefront g copies chunk g to
// its place behind p.  Exact bounds on both sides (copy_g2g_wide), any alignment.  Wavefront 0 also stores the 7 bytes of the
// header's size field.  (append_commit_plan has checked every length, the host the capacity.)
WV_FN void append_commit_chunk(uint8_t* to, const uint8_t* from, uint64_t len, uint64_t c)
{
	const uint64_t lo = c * APPEND_COMMIT_CHUNK;
	const uint32_t n = (uint32_t)(len - lo < APPEND_COMMIT_CHUNK ? len - lo : APPEND_COMMIT_CHUNK);
	copy_g2g_wide<COPY_ROUNDS>(to + lo, from + lo, n);
}
UPD_FN uint64_t append_commit_chunks(uint64_t len) { return (len + APPEND_COMMIT_CHUNK - 1) / APPEND_COMMIT_CHUNK; }
// bytes 1 .. 7 of the frame header := the new array size, little-endian, one lane each
WV_FN void append_commit_size_field(const AppendArgs& a)
{
	using namespace wv;
	const U32 lane = lane_id(), sh = (lane & U32(3u)) * U32(8u);
	const U32 v = sel(lane < U32(4u), U32((uint32_t)a.new_bytes) >> sh, U32((uint32_t)(a.new_bytes >> 32)) >> sh) & U32(0xFFu);
	gst8(a.frame + 1, lane, v, lane < U32(7u));
}
WV_FN void append_commit_copy(const AppendArgs& a, uint64_t g)
{
	const uint64_t p = append_word64(a.words, APPEND_W_P), len0 = append_word64(a.words, APPEND_W_LEN0), len1 = append_word64(a.words, APPEND_W_LEN1);
	const uint64_t c0 = append_commit_chunks(len0), c1 = append_commit_chunks(len1);
	if (g < c0)
		append_commit_chunk(a.frame + p, a.enc, len0, g);
	else if (g - c0 < c1)
		append_commit_chunk(a.frame + p + len0, a.enc + a.enc_base1, len1, g - c0);
}
WV_FN void append_commit_wave(const AppendArgs& a, uint64_t g)
{
	if (g == 0)
		append_commit_size_field(a);
	append_commit_copy(a, g);
}

} // namespace codec
#endif
