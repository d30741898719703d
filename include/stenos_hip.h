/*
 * stenos_hip.h -- device-resident entry points of libstenos.so (additions next to the frozen ABI of
 * stenos.h; the reference has no counterpart: its hot loop stenos_compress_generic,
 * stenos/internal/stenos.cpp:884-1010, and stenos_decompress_generic, :1118-1202, only take host
 * pointers).  Source and destination are DEVICE pointers; nothing crosses PCIe except the 8-byte
 * result.  Plain C: pointers and sizes only, `stream` is a hipStream_t passed as void* (NULL = the
 * default stream).
 */
#ifndef STENOS_HIP_H
#define STENOS_HIP_H
#include "stenos.h"

#ifdef __cplusplus
extern "C" {
#endif

/* number of HIP devices visible, 0 when the runtime is unusable */
STENOS_EXPORT int stenos_hip_device_count(void);

/* Bytes of device workspace the two calls below need for `bytes` of input (scratch slots, size and
 * offset tables) when the destination holds stenos_bound(bytes).  With a smaller destination every block goes through
 * a scratch slot instead of the fused kernel's staging buffers and the figure is up to about 1.03 x bytes higher.
 * The context allocates and keeps it; this is for capacity planning. */
STENOS_EXPORT size_t stenos_hip_workspace_bytes(size_t bytesoftype, size_t bytes);

/* Compress `bytes` of device memory into a Stenos frame in device memory.  The bytes of d_dst behind the returned frame size
 * (and inside dst_size) are scratch: incompressible stretches are put in place before their offsets are final
 * (csrc/kernels.hip, speculative copy), so that range may hold leftovers.  Nothing is written at or past dst_size, and
 * the host-pointer calls of stenos.h only copy the frame back.  Uses ctx's level and
 * block-size settings; a time limit (stenos_set_max_nanoseconds) is a feature of the host-pointer calls only:
 * with one set these entry points return STENOS_ERROR_INVALID_PARAMETER.  Enqueues on `stream`, then waits for the 8-byte size to come back.
 * Returns the frame size or an error code (test with stenos_has_error). */
STENOS_EXPORT size_t stenos_hip_compress(stenos_context* ctx, const void* d_src, size_t bytesoftype, size_t bytes, void* d_dst, size_t dst_size, void* stream);

/* Same, without waiting: the result is read by stenos_hip_finish().  The frame bytes in d_dst and
 * the index are valid once the stream has executed the enqueued work. */
STENOS_EXPORT size_t stenos_hip_compress_async(stenos_context* ctx, const void* d_src, size_t bytesoftype, size_t bytes, void* d_dst, size_t dst_size, void* stream);
STENOS_EXPORT size_t stenos_hip_finish(stenos_context* ctx);

/* Superblock index of the last compression on ctx: device array of nsb + 1 uint64 byte offsets of the
 * superblock headers inside the frame (the last entry is the frame size).  Valid until the next call on ctx;
 * stenos_hip_decompress_ranges calls that are given this pointer leave it as it is, any number of them. */
STENOS_EXPORT const uint64_t* stenos_hip_last_index(stenos_context* ctx, size_t* nsb);

/* Superblock index of any frame held in device memory: the chain of [code][csize:3] headers (reference
 * stenos.cpp:1126-1134, 1166-1182) is walked on the device -- by segments of the frame in parallel, with a result that is
 * proven equal to the serial walk's before it is used (csrc/walk.h).  Returns a device array of *nsb + 1 uint64 byte offsets
 * (the last entry is the end of the last superblock), valid until the next call on ctx; NULL for an empty, malformed or
 * truncated frame.  stenos_hip_decompress_ranges calls that are given this pointer leave it as it is, any number of them.
 * Waits for the walk.  What a multi-GPU decoder cuts the frame with. */
STENOS_EXPORT const uint64_t* stenos_hip_frame_index(stenos_context* ctx, const void* d_src, size_t bytesoftype, size_t bytes, size_t* nsb, void* stream);

/* Decompress a frame held in device memory.  d_index may be NULL: the superblock chain
 * ([code][csize:3] headers, reference stenos.cpp:1129-1134) is then walked on the device first (in parallel,
 * csrc/walk.h: tens of microseconds); passing the index produced by stenos_hip_last_index() skips that walk.
 * Returns the decompressed size or an error code. */
STENOS_EXPORT size_t stenos_hip_decompress(stenos_context* ctx, const void* d_src, size_t bytesoftype, size_t bytes, void* d_dst, size_t dst_size, const uint64_t* d_index, void* stream);
STENOS_EXPORT size_t stenos_hip_decompress_async(stenos_context* ctx, const void* d_src, size_t bytesoftype, size_t bytes, void* d_dst, size_t dst_size, const uint64_t* d_index, void* stream);

/* Batches: n independent arrays -> n independent frames, and back, in one pass of kernels (the fixed cost of a call is paid
 * once per batch instead of once per array).  d_srcs, d_dsts: host arrays of n DEVICE pointers; bytes / src_sizes, dst_sizes:
 * host arrays of n sizes.  results[i] receives item i's frame size (decompressed size) or an error code (test with
 * stenos_has_error): exactly what stenos_hip_compress (stenos_hip_decompress without an index) returns for that item alone,
 * and compressed frames are byte-identical to that call's.  Nothing is written at or past dst_sizes[i]; items' destinations
 * must not overlap.  Waits for completion.  Returns 0 when the batch ran (per-item outcomes in results[]; n == 0 returns 0),
 * or an error code for the call as a whole, with results[] and the destinations untouched:
 *   STENOS_ERROR_INVALID_INSTRUCTION_SET  no usable device;
 *   STENOS_ERROR_INVALID_PARAMETER        compression at level >= 2, bytesoftype 1 at level 1 (both take the host strategy
 *                                         layer), a time limit set on ctx; either direction with bytesoftype outside 1..64,
 *                                         or while an _async job on ctx is unfinished (that job is left alone).
 * Every item uses ctx's level and block-size settings and the one bytesoftype of the call.  Decompression accepts any frame
 * stenos_hip_decompress accepts; superblocks with zstd-based codes (levels >= 2, the last superblock under 128 bytes of a level-1
 * frame) are finished on the host item by item, which is slow.  Measured on MI355X (int32, level 1, profiles/batch_rate.txt):
 * 4096 items of 64 KiB compress at 436 GB/s and decompress at 821 GB/s, 390x and 1100x a loop of single calls; the batch has
 * no fused encoder, so for items between 64 MiB (batch 759 GB/s, loop 447) and 256 MiB (batch 770, single call 1 716) and above,
 * compression becomes faster through stenos_hip_compress; decompression in a batch is never slower.  After a batch (either direction), stenos_hip_last_index returns NULL
 * with *nsb = 0. */
STENOS_EXPORT size_t stenos_hip_compress_batch(stenos_context* ctx, size_t n, size_t bytesoftype, const void* const* d_srcs, const size_t* bytes,
					       void* const* d_dsts, const size_t* dst_sizes, size_t* results, void* stream);
STENOS_EXPORT size_t stenos_hip_decompress_batch(stenos_context* ctx, size_t n, size_t bytesoftype, const void* const* d_srcs, const size_t* src_sizes,
						 void* const* d_dsts, const size_t* dst_sizes, size_t* results, void* stream);
/* Device workspace a compress batch of these n sizes needs (capacity planning, like stenos_hip_workspace_bytes); 0 for a
 * bytesoftype outside 1..64. */
STENOS_EXPORT size_t stenos_hip_batch_workspace_bytes(size_t bytesoftype, size_t n, const size_t* bytes);

/* Random access: n byte ranges of the ORIGINAL array out of one frame in device memory, without inflating the rest: bytes
 * [offsets[i], offsets[i] + lengths[i]) go to d_dsts[i][0 .. lengths[i]).  offsets, lengths, d_dsts: host arrays of n.
 * Ranges are in bytes: any offset, any length (0 allowed: nothing is delivered, d_dsts[i] is not looked at), any alignment of
 * d_dsts[i].  Ranges may overlap or repeat in the source; destinations must not overlap each other.  Returns the sum of the
 * lengths, or an error code for the call as a whole; n == 0 returns 0.  Nothing is ever written outside
 * [d_dsts[i], d_dsts[i] + lengths[i]), neither on success nor on any error.  Waits for completion (there is no _async form).
 * Refused on the host, before any launch, with nothing written:
 *   STENOS_ERROR_INVALID_INSTRUCTION_SET  no usable device;
 *   STENOS_ERROR_INVALID_PARAMETER        a range with offset + length beyond the array's size (the frame header's, parsed as
 *                                         stenos_hip_decompress parses it; the sum is not formed, it may wrap), bytesoftype
 *                                         outside 1..64, more than 2^31 - 1 pieces (below), or while an _async job on ctx is
 *                                         unfinished (that job is left alone);
 *   a frame header stenos_hip_decompress refuses: its error code.
 * d_index is as for stenos_hip_decompress: NULL has the chain walked first (into the context's own index); an index that is
 * given is used as it is.  It may be the context's own, from stenos_hip_frame_index / stenos_hip_last_index: this call leaves
 * that buffer intact (its tables live in a buffer of their own), so the intended use is to index a frame once and read ranges
 * many times with the same pointer.
 * Every range is cut at the frame's superblock boundaries and one wavefront delivers each piece; pieces that share a superblock
 * are decoded each on its own, nothing is merged.  A superblock is a chain of blocks that has to be parsed from its start, so a
 * piece costs the decoding of its superblock up to the block that holds its last byte; a piece that is a whole superblock takes
 * the path of stenos_hip_decompress.  The number of launches and host round trips does not depend on n.
 * WHAT IS CHECKED: only the superblocks a range touches are read, and of those only the blocks up to the last byte asked
 * for.  Damage anywhere else in the frame is NOT detected by this call (with d_index == NULL the walk still sees every
 * superblock header).  A truncated or malformed superblock or block that is decoded gives STENOS_ERROR_SRC_OVERFLOW /
 * STENOS_ERROR_INVALID_INPUT as in stenos_hip_decompress; destinations may then be partly written, inside their bounds.
 * Superblocks with zstd-based codes (every superblock of a level >= 2 frame and of bytesoftype 1, the last superblock under
 * 128 bytes of a level-1 frame) are fetched and inflated on the host piece by piece, which is slow. */
STENOS_EXPORT size_t stenos_hip_decompress_ranges(stenos_context* ctx, const void* d_src, size_t bytesoftype, size_t bytes, size_t n, const uint64_t* offsets,
						  const uint64_t* lengths, void* const* d_dsts, const uint64_t* d_index, void* stream);

/* Gather: n rows of the ORIGINAL array out of one frame in device memory, by row numbers that live in DEVICE memory.  Row r is
 * bytes [r * row_bytes, (r + 1) * row_bytes) of the array; row d_rows[i] goes to d_dst + i * dst_stride, for i in 0..n.  The
 * host never reads d_rows on the common path, and every enqueued step is ordered on `stream`: row numbers written by earlier
 * work on that stream (a kernel, a torch op) need no synchronisation by the caller.  row_bytes >= 1 may be any value (not a
 * multiple of bytesoftype, larger than a superblock), d_dst may have any alignment, dst_stride >= row_bytes; rows may repeat,
 * in any order.  Returns n * row_bytes, or an error code for the call as a whole; n == 0 returns 0 before the devices are
 * looked at.  Nothing is ever written outside the n slots [d_dst + i * dst_stride, + row_bytes) -- nothing in the dst_stride -
 * row_bytes bytes between them either --, neither on success nor on any error.  Waits for completion (there is no _async form).
 * Refused on the host, before any launch, with nothing written:
 *   STENOS_ERROR_INVALID_INSTRUCTION_SET  no usable device;
 *   STENOS_ERROR_INVALID_PARAMETER        row_bytes == 0, dst_stride < row_bytes, n * row_bytes or (n - 1) * dst_stride +
 *                                         row_bytes not representable, bytesoftype outside 1..64, more than 2^31 - 1 pieces
 *                                         (n times the pieces per row, below), or while an _async job on ctx is unfinished
 *                                         (that job is left alone);
 *   a frame header stenos_hip_decompress refuses: its error code.
 * ROW NUMBERS ARE CHECKED ON THE DEVICE: a valid row has d_rows[i] < floor(array size / row_bytes) (the host computes that
 * bound, no product that may wrap is formed on the device).  An invalid row makes no piece -- its slot is not touched -- and the
 * call then returns STENOS_ERROR_INVALID_PARAMETER, in front of any decode error; what the other slots hold after that return
 * is unspecified.
 * d_index is as for stenos_hip_decompress_ranges: NULL has the chain walked first (into the context's own index); an index that
 * is given is used as it is.  It may be the context's own, from stenos_hip_frame_index / stenos_hip_last_index: this call leaves
 * that buffer intact (its tables live in a buffer of their own), any number of calls.
 * Every row is cut at the frame's superblock boundaries on the device -- a fixed number of pieces per row: 1 when row_bytes
 * divides the superblock size, else ceil((row_bytes - 1) / superblock size) + 1, some of them empty --, the pieces are
 * grouped by superblock there, and one wavefront walks a superblock's chain of blocks once for up to 64 of its pieces, up to
 * the block that holds the last byte any of them asks for.  The number of launches and host round trips depends neither on n
 * nor on the number of superblocks: at most min(superblocks, pieces) + pieces / 64 wavefronts decode.  Pieces that cover a
 * whole superblock take the same path through the wavefront's LDS image: a caller with rows of a superblock or more is better
 * served by stenos_hip_decompress_ranges.  A single row costs four launches where the ranges call has one and is slower than
 * it (profiles/gather_rate.txt).
 * WHAT IS CHECKED: only the superblocks a row touches are read, and of those only the blocks up to the last byte asked
 * for.  Damage anywhere else in the frame is NOT detected by this call (with d_index == NULL the walk still sees every
 * superblock header).  A truncated or malformed superblock or block that is decoded gives STENOS_ERROR_SRC_OVERFLOW /
 * STENOS_ERROR_INVALID_INPUT as in stenos_hip_decompress; slots may then be partly written, inside their bounds.
 * Superblocks with zstd-based codes (every superblock of a level >= 2 frame and of bytesoftype 1, the last superblock under
 * 128 bytes of a level-1 frame) are finished on the host: d_rows comes down, the pieces of those superblocks are cut again
 * there and inflated piece by piece, which is slow. */
STENOS_EXPORT size_t stenos_hip_gather_rows(stenos_context* ctx, const void* d_src, size_t bytesoftype, size_t bytes, size_t row_bytes, size_t n,
					    const uint64_t* d_rows, void* d_dst, size_t dst_stride, const uint64_t* d_index, void* stream);

/* Gather of VARIABLE-LENGTH ranges: n byte ranges of the ORIGINAL array out of one frame in device memory, by offsets and lengths
 * that live in DEVICE memory -- the device-resident form of stenos_hip_decompress_ranges, with a packed, CSR-style output.
 * d_offsets and d_lengths have n entries each; bytes [d_offsets[i], d_offsets[i] + d_lengths[i]) go to d_dst + D[i], where D is the
 * exclusive prefix sum of the lengths.  d_dst_offsets may be NULL; where it is not, it receives the n + 1 entries of D, D[n] being
 * the total: what the caller indexes the packed output with.  It must not overlap d_dst, d_offsets or d_lengths (the offsets and
 * lengths are read again after D has been written: in place is not supported).  The host never reads d_offsets or
 * d_lengths on the common path, and every enqueued step is ordered on `stream`: offsets written by earlier work on that stream (a
 * kernel, a torch op) need no synchronisation by the caller.  Any offset and any length; length 0 is allowed (it delivers nothing
 * and makes no piece); ranges may overlap and repeat, in any order; d_dst may have any alignment.  Returns D[n], or an error code
 * for the call as a whole; n == 0 returns 0 before the devices are looked at.  Waits for completion (there is no _async form).
 * dst_size is the REAL capacity of d_dst in bytes, not a "large enough" constant: it sizes the call's tables and grids (below).
 * On success nothing outside [d_dst, d_dst + D[n]) is written.  On a host-side refusal, an invalid range or an overflow (all
 * below) NO BYTE of d_dst is written.  After a decode error d_dst may be partly written, inside [d_dst, d_dst + D[n]).  What
 * d_dst_offsets holds after an error is unspecified.
 * Refused on the host, before any launch:
 *   STENOS_ERROR_INVALID_INSTRUCTION_SET  no usable device;
 *   STENOS_ERROR_INVALID_PARAMETER        bytesoftype outside 1..64, a piece bound (below) or the decode grid for it above
 *                                         2^31 - 1, or while an _async job on ctx is unfinished (that job is left alone);
 *   a frame header stenos_hip_decompress refuses: its error code.
 * The frame of an EMPTY array is accepted: only ranges of length 0 at offset 0 are valid in it.  It has no superblock and so no
 * piece: its Pmax is 0 whatever dst_size is, no table or grid is sized by dst_size and no dst_size is refused.
 * RANGES ARE CHECKED ON THE DEVICE: a valid range has offset <= array size and length <= array size - offset (no sum that may
 * wrap is formed).  Any invalid range gives STENOS_ERROR_INVALID_PARAMETER; otherwise D[n] > dst_size gives
 * STENOS_ERROR_DST_OVERFLOW.  Both come in front of any decode error and both leave d_dst untouched: the stage that forms D leaves
 * a status bit, with such a bit set no piece is made and every decoding wavefront leaves at its first test.  No extra host round
 * trip is spent on this.
 * d_index is as for stenos_hip_gather_rows: NULL has the chain walked first (into the context's own index); an index that is
 * given is used as it is.  It may be the context's own, from stenos_hip_frame_index / stenos_hip_last_index: this call leaves
 * that buffer intact (its tables live in a buffer of their own), any number of calls.
 * HOW: the pieces of a range are its intersections with the superblocks it touches, in order: non-empty, disjoint, their lengths
 * sum to the length.  One thread per range tests it and counts its bytes and pieces; three passes ordered by the stream (sums per
 * block of 256 ranges, one workgroup over the sums, apply -- no workgroup waits for another) form D and the first piece slot of
 * every range; one thread per piece slot finds its range by binary search and cuts its piece, so a long range is not serial
 * work; the pieces are grouped by superblock, and stenos_hip_gather_rows's decoder, unchanged, walks a superblock's chain of
 * blocks once for up to 64 of its pieces, up to the block that holds the last byte any of them asks for.  A range of length
 * L >= 1 touches at most floor((L - 1) / superblock size) + 2 superblocks, so a call that fits dst_size has at most
 *   Pmax = 2 n + floor(dst_size / superblock size)
 * pieces: Pmax sizes the piece table and the grids; threads and wavefronts beyond the real counts leave at once.  Host round trips:
 * the frame header, then the status together with D[n].  Launches and round trips depend neither on n, nor on the lengths, nor
 * on the number of superblocks.  A piece that is a whole superblock takes the same path through the wavefront's LDS image: a
 * caller with ranges of a superblock or more is better served by stenos_hip_decompress_ranges.
 * DEVICE MEMORY the context keeps for this call (it grows to the largest call and is freed with the context): 16 bytes per
 * bounded piece (16 Pmax); per range 4 bytes (its first piece slot), 8 more where d_dst_offsets is NULL (D), and 12 bytes per
 * 256 ranges (the blocks' sums); per superblock of the frame 16 bytes (counts, flags, two prefix tables); 64 bytes of words.
 * WHO IS SERVED BY WHAT (MI355X, int32, level 1, 1 GiB frame, index passed in, medians of 20 after 3 untimed rounds; tools/gather_ranges_rate.py,
 * profiles/gather_ranges_rate.txt; the other side is the only way without this call: offsets and lengths to the
 * host, destination addresses formed there, one stenos_hip_decompress_ranges):
 * Many short ranges are what this call is for.  It WINS: 65 536 ranges of 1..8 KiB at uniform random offsets take 0.55 ms (485 GB/s
 * delivered, 2.4 MiB of device memory held) against 1.91 ms, x3.5; 2^20 ranges of 1..512 B take 1.16 ms (36 MiB held) against
 * 26.1 ms, x22; 65 536 ranges of exactly 4 KiB take 0.53 ms against 1.85 ms, x3.5 -- and 0.52 ms through stenos_hip_gather_rows,
 * so raggedness itself (the measuring, the scan and the binary search per piece) costs under 3 % there.  It LOSES with a few long
 * ranges: 16 ranges of 16 MiB take 0.42 ms against 0.34 ms (x0.83; every piece is a whole superblock, which the ranges call
 * decodes by the path of stenos_hip_decompress).  ONE range of 4 KiB is a tie inside the noise (0.196 against 0.198 ms, the two
 * series of the other side 6 us apart): seven kernel launches and the larger tables on this side, the copies of offset and length to
 * the host on the other.
 * WHAT IS CHECKED: only the superblocks a range touches are read, and of those only the blocks up to the last byte asked
 * for.  Damage anywhere else in the frame is NOT detected by this call (with d_index == NULL the walk still sees every
 * superblock header).  A truncated or malformed superblock or block that is decoded gives STENOS_ERROR_SRC_OVERFLOW /
 * STENOS_ERROR_INVALID_INPUT as in stenos_hip_decompress.
 * Superblocks with zstd-based codes (every superblock of a level >= 2 frame and of bytesoftype 1, the last superblock under
 * 128 bytes of a level-1 frame) are finished on the host: d_offsets and d_lengths come down, the host forms D, cuts the pieces
 * of those superblocks again with the same cutting function and inflates them piece by piece, which is slow. */
STENOS_EXPORT size_t stenos_hip_gather_ranges(stenos_context* ctx, const void* d_src, size_t bytesoftype, size_t bytes, size_t n, const uint64_t* d_offsets,
					      const uint64_t* d_lengths, void* d_dst, size_t dst_size, uint64_t* d_dst_offsets, const uint64_t* d_index, void* stream);

/* Gather from MANY frames in one call: n rows, each out of one of m frames in device memory, by (frame number, row number)
 * pairs that live in DEVICE memory.  d_frames and sizes are HOST arrays of m: the frames' device pointers and their sizes in
 * bytes.  Slot i, [d_dst + i * dst_stride, + row_bytes), receives row d_rows[i] of the original array of frame d_frame_ids[i];
 * row r of a frame is bytes [r * row_bytes, (r + 1) * row_bytes) of that frame's array: the semantics of
 * stenos_hip_gather_rows, row for row.  One bytesoftype and one row_bytes hold for the call; the frames may differ in size and
 * in superblock size (each frame's own header decides).  row_bytes >= 1 may be any value, d_dst may have any alignment,
 * dst_stride >= row_bytes; pairs may repeat, in any order, and two entries of d_frames may name the same frame.  The host
 * never reads d_frame_ids and d_rows on the common path, and every enqueued step is ordered on `stream`.  Returns n *
 * row_bytes, or an error code for the call as a whole; n == 0 returns 0 before anything is looked at.  Nothing is ever written
 * outside the n slots, neither on success nor on any error.  Waits for completion (there is no _async form).
 * Refused on the host, before any launch that writes to d_dst, with nothing written:
 *   STENOS_ERROR_INVALID_INSTRUCTION_SET  no usable device;
 *   STENOS_ERROR_INVALID_PARAMETER        what stenos_hip_gather_rows refuses (row_bytes == 0, dst_stride < row_bytes, n *
 *                                         row_bytes or (n - 1) * dst_stride + row_bytes not representable, bytesoftype outside
 *                                         1..64, an unfinished _async job on ctx); m == 0; m, the superblocks of all frames
 *                                         together, n times the pieces per pair (below) or the decode grid above 2^31 - 1;
 *   a frame header stenos_hip_decompress refuses: its error code, for the first such frame in the order of d_frames.
 * UNLIKE stenos_hip_gather_rows, the frame of an EMPTY array is accepted: it has no valid row and does not fail the call by
 * being listed.
 * PAIRS ARE CHECKED ON THE DEVICE: a valid pair has d_frame_ids[i] < m and d_rows[i] < floor(array size / row_bytes) of that
 * frame (the host computes the bounds).  An invalid pair makes no piece -- its slot is not touched -- and the call then returns
 * STENOS_ERROR_INVALID_PARAMETER, in front of any decode error; what the other slots hold after that return is unspecified.
 * d_index: NULL has every chain walked first, into the context's own index (chains of up to 256 superblocks all in one launch,
 * longer ones by the parallel walk, one launch each).  An index that is given is used as it is.  Its layout: frame f's
 * superblocks + 1 header offsets start at entry f + (superblocks of the frames in front of f) -- what stenos_hip_frames_index
 * returns.  The call keeps its tables in a buffer of its own and leaves the context's index intact: index once, gather any
 * number of times.
 * The superblocks of all frames are numbered through; every pair is cut at its frame's superblock boundaries on the device (P
 * pieces per pair, the largest of the frames' own counts, see stenos_hip_gather_rows), the pieces are grouped by superblock
 * there, and one wavefront walks a superblock's chain of blocks once for up to 64 of its pieces.  Launches and host round trips
 * depend neither on n nor on the number of superblocks, and on m only through the parallel walks above; the host's own work
 * and the table it uploads are O(m).
 * WHO IS SERVED BY WHAT (MI355X, int32, level 1, index passed in; tools/gather_batch_rate.py, profiles/gather_batch_rate.txt,
 * DESIGN.md 14).  Many frames with a few rows each are what this call is for: 65 536 uniform random pairs of 256 B over 4 096
 * frames of 64 KiB take 0.27 ms, where a loop of stenos_hip_gather_rows over the 4 096 frames takes 478 ms with the pairs already
 * grouped on the host -- x1759, all of it the single call's fixed cost of about 117 us per frame.  With the pairs inside 16 frames
 * the loop of 16 calls is still 11.6 times slower, over 8 frames of 128 MiB a loop of 8 calls 3.6 times (1.68 against 0.47 ms).
 * With m = 1 this call and stenos_hip_gather_rows cost the same (ratio 1.00 and 0.99 on the 1 GiB frame, inside the noise): a
 * store that fits one large frame loses nothing by staying one and calling stenos_hip_gather_rows, which needs no frame table.
 * A loop of single calls serves only a caller whose rows are grouped by frame on the host anyway and touch very few frames.
 * WHAT IS CHECKED: only the superblocks a row touches are read, and of those only the blocks up to the last byte asked
 * for.  Damage anywhere else in any frame is NOT detected by this call (with d_index == NULL the walks still see every
 * superblock header).  A truncated or malformed superblock or block that is decoded gives STENOS_ERROR_SRC_OVERFLOW /
 * STENOS_ERROR_INVALID_INPUT as in stenos_hip_decompress, for the call as a whole (there are no per-frame results); slots may
 * then be partly written, inside their bounds.
 * Superblocks with zstd-based codes (see stenos_hip_gather_rows) are finished on the host: the pairs come down, the pieces of
 * those superblocks are cut again there, grouped by frame and inflated piece by piece, which is slow. */
STENOS_EXPORT size_t stenos_hip_gather_rows_batch(stenos_context* ctx, size_t m, size_t bytesoftype, const void* const* d_frames, const size_t* sizes,
							  size_t row_bytes, size_t n, const uint64_t* d_frame_ids, const uint64_t* d_rows, void* d_dst, size_t dst_stride,
							  const uint64_t* d_index, void* stream);

/* The index stenos_hip_gather_rows_batch takes, for m frames in device memory (d_frames, sizes: host arrays of m): every chain
 * is walked on `stream` and a pointer to DEVICE memory is returned, *entries = its length = the superblocks of all frames + m.
 * Frame f's slice is what stenos_hip_frame_index gives for that frame (the frame of an empty array has one entry, its end).
 * NULL for a malformed or truncated frame, m == 0, or whatever the gather call refuses about ctx and bytesoftype.  The array is
 * the context's own index: valid until the next call on ctx that is not a stenos_hip_gather_rows_batch given this pointer. */
STENOS_EXPORT const uint64_t* stenos_hip_frames_index(stenos_context* ctx, size_t m, size_t bytesoftype, const void* const* d_frames, const size_t* sizes,
							      size_t* entries, void* stream);

/* Update: the mirror image of the gather call.  n rows of the ORIGINAL array are replaced, by row numbers that live in DEVICE
 * memory, and the frame of the updated array is written to a second buffer; the array's size, its superblock size and its
 * header never change, and the input frame is never modified.  Row r is bytes [r * row_bytes, (r + 1) * row_bytes) of the
 * array, as in stenos_hip_gather_rows; the row_bytes bytes at d_src + i * src_stride replace row d_rows[i], for i in 0..n.
 * d_out receives a complete frame; the call returns its size, or an error code for the call as a whole.  d_rows is read on the
 * device only, and every enqueued step is ordered on `stream`: row numbers and source rows written by earlier work on that
 * stream need no synchronisation by the caller.  row_bytes >= 1 may be any value (not a multiple of bytesoftype, larger than
 * a superblock), src_stride >= row_bytes, d_src and d_out may have any alignment.  Bytes of the array behind the last whole
 * row cannot be addressed and stay as they are.  d_out must overlap neither d_frame nor the source rows.  Waits for completion
 * (there is no _async form).  n == 0 gives a byte copy of the frame, after the header and index checks below.
 * THE OUTPUT FRAME is the frame stenos_hip_compress produces for the updated array at the frame's own geometry (the shift or
 * custom superblock size of its header, not ctx's block-size setting) and ctx's level into a destination of
 * stenos_bound(array size) bytes: superblocks no row touches are the input's bytes as they are, the touched ones are decoded,
 * overlaid and encoded again at ctx's level, each on its own -- so if the input frame was made by stenos_hip_compress at that
 * level into a destination of the bound's size, the whole output is byte-identical to compressing the updated array.  If it
 * does not fit in out_size the call returns STENOS_ERROR_DST_OVERFLOW (the reference's behaviour for tight destinations is not
 * imitated).
 * WRITES TO d_out: on success nothing outside [d_out, d_out + returned size).  Nothing at all on a host-side refusal, an
 * invalid row number, STENOS_ERROR_DST_OVERFLOW, a refused index or a decode error of a touched superblock: every byte of d_out
 * is written by the last kernel (update_splice), which is launched only after the status and the new size have come back.
 * REPEATED ROW NUMBERS: each piece of such a row (a row is cut at superblock boundaries) ends up holding the bytes of one of
 * its sources, whole; which one is unspecified, and two pieces of one row may hold different sources.
 * Refused on the host, before any launch, with nothing written:
 *   STENOS_ERROR_INVALID_INSTRUCTION_SET  no usable device;
 *   STENOS_ERROR_INVALID_PARAMETER        row_bytes == 0, src_stride < row_bytes, n * row_bytes or (n - 1) * src_stride +
 *                                         row_bytes not representable, bytesoftype outside 1..64, more than 2^31 - 1 pieces
 *                                         (n times the pieces per row of the gather call), while an _async job on ctx is
 *                                         unfinished, and whatever stenos_hip_compress_batch refuses to compress: ctx's level
 *                                         >= 2, bytesoftype 1 at level 1, a time limit on ctx;
 *   a frame header stenos_hip_decompress refuses: its error code.
 * ROW NUMBERS ARE CHECKED ON THE DEVICE as in the gather call (valid: d_rows[i] < floor(array size / row_bytes)); an invalid
 * one gives STENOS_ERROR_INVALID_PARAMETER, in front of any decode error.
 * d_index is as for the gather call: NULL has the chain walked first; an index that is given is used as it is, after a check
 * that is made before anything is written: offsets must not decrease, every superblock takes at least its 4 header bytes
 * (and at most what a header can announce), the last entry is at most `bytes` -- else STENOS_ERROR_INVALID_INPUT /
 * STENOS_ERROR_SRC_OVERFLOW.  No kernel reads outside [d_frame, d_frame + bytes), whatever the index or a size field says.
 * After a successful call stenos_hip_last_index returns the index of the NEW frame (its superblocks + 1 offsets): the next
 * gather or update on d_out needs no walk.  A pointer obtained earlier is invalid after the call (after an unsuccessful one
 * too); an index passed in may be the context's own: it is copied before the context's buffer is written.
 * HOW: the rows are cut and grouped by superblock on the device (the gather call's kernels); update_plan lists the k
 * superblocks that hold pieces; update_decode decodes them whole, one wavefront each, into k slots; update_apply copies the
 * pieces' source bytes in; the slots are encoded as k independent superblocks by the kernels of stenos_hip_compress;
 * update_splice_plan makes the new index and size; update_splice copies every superblock to its place, one workgroup each.
 * Host round trips are three -- the header, k with the status, the new size with the status -- and the wait for completion;
 * launches and round trips depend neither on n nor on the number of superblocks.
 * DEVICE MEMORY kept by ctx: 40 bytes per superblock of the frame + 16 per piece (tables and both indices); k * superblock
 * size (the slots); k * (superblock size + 4) + one superblock (their encodings); and the unfused encoder's workspace for k
 * superblocks -- one padded slot per block of 256 * bytesoftype bytes (about 1.14 x the block for int32), 16 bytes of tables per
 * block, 37 per superblock: together about 3.2 * k * superblock size.  Proportional to k, never to the array -- but with every
 * superblock touched that is three times the array.  The buffers never shrink: they stay at the largest size a call needed
 * until the context is destroyed.
 * MEASURED on MI355X (profiles/update_rate.txt: 1 GiB int32 frame of 8 192 superblocks, level 1, index passed in, unique uniform
 * random 4 KiB rows, medians of 20; against stenos_hip_decompress into a scratch tensor + index_copy_ + stenos_hip_compress,
 * which leave the same frame), update / baseline in microseconds, superblocks touched, device memory held:
 *        1 row          490 /    785   x1.60      1 superblock     14 MiB against 1030 MiB
 *      256 rows         538 /    782   x1.45    253 superblocks  116 MiB against 1030 MiB
 *    4 096 rows       1 015 /    816   x0.80  3 247             1300 MiB
 *   65 536 rows       2 028 /  1 355   x0.67  8 191             3248 MiB
 *   every row         2 375 /  3 021   x1.27  8 192             3264 MiB
 * The whole-frame splice reads and writes the compressed size; decoding and encoding scale with k, and the encode is by the
 * unfused kernels.  The call wins while the rows touch a small share of the superblocks; scattered rows that touch a third of
 * them or more while changing little of each are served faster, and with less memory, by stenos_hip_decompress + a write +
 * stenos_hip_compress; replacing every row is ahead again because the baseline then moves the whole array once more.
 * WHAT IS CHECKED: touched superblocks are decoded completely; damage in them gives STENOS_ERROR_SRC_OVERFLOW /
 * STENOS_ERROR_INVALID_INPUT as in stenos_hip_decompress.  Untouched superblocks are copied, not parsed: damage in them is
 * NOT detected by this call (with d_index == NULL the walk still sees every superblock header) and arrives in d_out.
 * Touched superblocks with zstd-based codes (the last superblock under 128 bytes of a level-1 frame; every superblock of a
 * level >= 2 frame, which a level-0/1 context may update) are fetched and inflated on the host, one whole superblock at a
 * time, which is slow, and encoded again at ctx's level. */
STENOS_EXPORT size_t stenos_hip_update_rows(stenos_context* ctx, const void* d_frame, size_t bytesoftype, size_t bytes, size_t row_bytes, size_t n,
					    const uint64_t* d_rows, const void* d_src, size_t src_stride, void* d_out, size_t out_size, const uint64_t* d_index,
					    void* stream);

/* Rows of MANY frames replaced in one call: the mirror image of stenos_hip_gather_rows_batch, with the rules of
 * stenos_hip_update_rows applied frame by frame.  d_frames, sizes, d_outs, out_sizes and results are host arrays of m;
 * d_frame_ids, d_rows (n each) and the source rows are device memory, which the host never reads on the common path; every
 * enqueued step is ordered on `stream`.  The row_bytes bytes at d_src + i * src_stride replace row d_rows[i] of the array of
 * frame d_frame_ids[i].  d_outs[f] receives a complete frame for EVERY listed frame -- one that no pair names gets a byte copy
 * of its input -- and results[f] its size; the call returns 0 when it ran, or an error code for the call as a whole (there is
 * no success of some frames).  n == 0 copies every frame, after the header and index checks.  Input frames are never modified;
 * the outputs must overlap nothing: no input frame, no source row, no other output.  Two entries of d_frames may name the same
 * frame: each entry is updated on its own, by the pairs that carry its number.  The frame of an empty array is accepted: it has
 * no valid row and is copied.
 * THE OUTPUT FRAMES: d_outs[f] holds, byte for byte and in size, what stenos_hip_update_rows leaves for frame f given only the
 * pairs that name f -- so for inputs made by stenos_hip_compress or stenos_hip_compress_batch at ctx's level into destinations
 * of the bound's size, the frame stenos_hip_compress makes of the updated array (the conditions are the single call's).
 * WRITES TO d_outs: all or nothing.  On success nothing outside [d_outs[f], d_outs[f] + results[f]).  On any error -- a
 * host-side refusal, an invalid pair, a refused index, a decode error in a touched superblock of any frame, a new frame that
 * does not fit its out_sizes[f] (STENOS_ERROR_DST_OVERFLOW) -- no byte of any d_outs[f] is written and results[] is left alone:
 * every byte of the outputs is written by the last kernel (update_batch_splice), which is launched only after the status and
 * all new sizes have come back.
 * REPEATED PAIRS follow the single call's rule: each piece of such a row ends up holding the bytes of one of its sources,
 * whole; which one is unspecified.
 * ONE GEOMETRY: the touched superblocks of all frames are encoded in one pass, and that pass has one geometry, so all frames of
 * non-empty arrays must have one superblock size, else STENOS_ERROR_INVALID_PARAMETER.  A store whose frames were made under
 * one block-size setting (stenos_set_block_size, or none at all: level 1 never shifts) is not affected.
 * Refused on the host, before any launch that writes, with nothing written: everything stenos_hip_update_rows refuses (the
 * shape checks on row_bytes, src_stride and n; bytesoftype outside 1..64; an unfinished _async job; ctx's level >= 2,
 * bytesoftype 1 at level 1, a time limit); m == 0; a NULL in d_frames or d_outs; m, the superblocks of all frames together plus
 * m, n times the pieces per pair, or any grid above 2^31 - 1; a frame header stenos_hip_decompress refuses (that header's
 * error code, for the first such frame); frames of different superblock sizes.
 * PAIRS ARE CHECKED ON THE DEVICE as in stenos_hip_gather_rows_batch (valid: d_frame_ids[i] < m and d_rows[i] < floor(array size
 * of that frame / row_bytes)); an invalid one gives STENOS_ERROR_INVALID_PARAMETER, in front of any decode error.
 * d_index has the layout of stenos_hip_frames_index (S + m entries, frame f's slice at entry first[f] + f); NULL has the chains
 * walked first.  An index that is given is checked per frame as the single call checks it, before anything is written: offsets
 * must not decrease, every superblock takes at least its 4 header bytes and at most 4 + 2^24 - 1, the last entry of a frame is
 * at most sizes[f] -- else STENOS_ERROR_INVALID_INPUT / STENOS_ERROR_SRC_OVERFLOW.  It may be the context's own: it is copied
 * before the context's buffer is written.  No kernel reads outside [d_frames[f], d_frames[f] + sizes[f]), whatever an index
 * entry or a size field says.
 * After a successful call the context's index is that of the NEW frames, in the same layout: stenos_hip_last_frames_index
 * returns it with its length (NULL and 0 when the last call on ctx left no many-frame index: it is valid after
 * stenos_hip_frames_index and after this call, until the next call that uses the context's index workspace), so the next
 * stenos_hip_gather_rows_batch or stenos_hip_update_rows_batch on the outputs needs no walk.  stenos_hip_last_index keeps
 * returning NULL after a batch.
 * HOW: the heads, the numbering and the walks are those of every call over many frames; the pairs are cut and grouped by
 * superblock over all frames by the batched gather's kernels; update_batch_plan lists the K touched superblocks of all frames
 * (a frame's are one run of the list) and tells the host how many each frame has; update_batch_decode decodes them whole, one
 * wavefront each, into K slots; update_batch_apply copies the pieces' source bytes in; the slots are encoded by the kernels of
 * stenos_hip_compress_batch, one item without a frame header per touched frame; update_batch_splice_plan makes the new indices
 * and sizes; update_batch_splice copies every superblock of every frame to its place, one workgroup each.  Host round trips
 * are three -- the heads, the counts with the status, the new sizes with the status -- and the wait for completion; launches
 * and round trips depend neither on n nor on the number of superblocks, and on m only through the parallel walks of chains
 * longer than 256 superblocks and the host paths below; host work and uploaded tables are O(m).
 * DEVICE MEMORY kept by ctx (S superblocks in all frames, K of them touched): about 0.8 KB per frame (tables), 48 bytes per
 * superblock + 16 per piece (tables, both indices, the sums); K * superblock size (the slots); K * (superblock size + 4) + one
 * superblock's worst case per touched frame (the encodings); and the batch encoder's workspace for K superblocks (one padded
 * slot per block, 16 bytes of tables per block, 21 per superblock): together about 3.2 * K * superblock size, as in the single
 * call.  The buffers never shrink: they stay at the largest size a call needed until the context is destroyed.
 * A slot and an encoding take a whole superblock even where the frame is shorter, and the worst-case pad is per touched frame:
 * 4 096 touched frames of 64 KiB hold 1.75 GiB.
 * WHO IS SERVED BY WHAT -- MEASURED on MI355X (profiles/update_batch_rate.txt: int32, level 1, index passed in, unique uniform
 * random pairs, medians of 20; against the only way without this call: the pairs to the host, grouped by frame, one
 * stenos_hip_update_rows per touched frame, one device copy per untouched frame), batch / baseline in microseconds:
 *   4 096 frames of 64 KiB, rows of 256 B       256 pairs      801 /  79 026   x98.6
 *                                            65 536 pairs    1 154 / 799 111   x693     (the condition the call was built under: met)
 *                                            every row       1 894 / 900 617   x476
 *   16 frames of 128 MiB, rows of 4 KiB       4 096 pairs    1 453 /   5 469   x3.76
 *    8 frames of 128 MiB, rows of 4 KiB       4 096 pairs    1 121 /   2 985   x2.66
 *    1 frame of 1 GiB, rows of 4 KiB          4 096 pairs    1 092 /   1 013   x0.93    (against stenos_hip_update_rows itself)
 * A store of many frames is served by this call whatever the number of pairs: the baseline pays the single call's fixed cost per
 * frame touched.  A store that is one large frame stays with stenos_hip_update_rows, which is 7 % faster there.
 * WHAT IS CHECKED: as in the single call -- touched superblocks are decoded completely, untouched ones are copied, not parsed:
 * damage in them is NOT detected and arrives in the output.  Touched superblocks with zstd-based codes (the last superblock
 * under 128 bytes of a level-1 frame; every superblock of a level >= 2 frame) are fetched and inflated on the host, one whole
 * superblock at a time, which is slow; a touched last superblock under 128 bytes is encoded on the host as well, as the batch
 * encoder does for its tiny items. */
STENOS_EXPORT size_t stenos_hip_update_rows_batch(stenos_context* ctx, size_t m, size_t bytesoftype, const void* const* d_frames, const size_t* sizes,
						  size_t row_bytes, size_t n, const uint64_t* d_frame_ids, const uint64_t* d_rows, const void* d_src,
						  size_t src_stride, void* const* d_outs, const size_t* out_sizes, size_t* results, const uint64_t* d_index,
						  void* stream);
STENOS_EXPORT const uint64_t* stenos_hip_last_frames_index(stenos_context* ctx, size_t* entries);

/* Append, IN PLACE: the array of a frame in device memory grows by bytes that live in device memory.  d_frame[0 .. bytes) is a
 * frame of an array A; it lies in a buffer of `capacity` >= bytes bytes; d_src[0 .. src_bytes) are the bytes B.  Afterwards
 * d_frame holds a frame of A||B and the call returns its size, or an error code.  B may have been written by earlier work on
 * `stream` (a kernel, a torch op): every enqueued step is ordered on it and the caller need not synchronise.  d_src must not
 * overlap [d_frame, d_frame + capacity); d_frame and d_src may have any alignment; src_bytes may be any value (not a multiple
 * of bytesoftype; the array's size need not be one either).  Waits for completion (there is no _async form).  Size the buffer
 * with stenos_bound(final array size).
 * THE RESULTING FRAME keeps the frame's own geometry (the shift or custom superblock size of its header, not ctx's block-size
 * setting).  With sb the superblock size, keep = floor(|A| / sb) and r = |A| mod sb: superblocks 0 .. keep of the frame stay
 * exactly where and what they are -- the frame of A||B starts with the frame of A up to A's last whole superblock, byte for
 * byte, because superblocks are encoded independently.  The stream from the header of superblock `keep` on (offset p =
 * index[keep]: the end of the chain when r == 0) is replaced by the encoding of (last r bytes of A)||B at ctx's level, as
 * independent superblocks, and the 7-byte size field of the header becomes |A| + src_bytes.  So if the input frame was made by
 * stenos_hip_compress or stenos_hip_compress_batch at ctx's level into a destination of stenos_bound's size, the result is,
 * byte for byte and in size, the frame stenos_hip_compress makes of A||B.  For frames of other origin: superblocks 0 .. keep
 * are unchanged and the new frame decodes to A||B.
 * WRITES TO d_frame: on success nothing outside the 7 size bytes of the header and [d_frame + p, d_frame + returned size);
 * nothing at or behind the returned size.  On any failure -- a host-side refusal, a refused index, damage in the last
 * superblock, a new frame larger than capacity (STENOS_ERROR_DST_OVERFLOW) -- no byte of [d_frame, d_frame + capacity) is
 * written: every byte goes through the last kernel (append_commit), which is launched only after the status and the new size
 * have come back.
 * Refused on the host, before any launch, with nothing written:
 *   STENOS_ERROR_INVALID_INSTRUCTION_SET  no usable device;
 *   STENOS_ERROR_INVALID_PARAMETER        capacity < bytes, bytesoftype outside 1..64, |A| + src_bytes not representable in 56
 *                                         bits, more than 2^31 - 1 superblocks in the new frame, while an _async job on ctx is
 *                                         unfinished, and whatever stenos_hip_compress_batch refuses to compress: ctx's level
 *                                         >= 2, bytesoftype 1 at level 1, a time limit on ctx;
 *   a frame header stenos_hip_decompress refuses: its error code.
 * SPECIAL SIZES: src_bytes == 0 returns the end of the chain after the header and index checks and writes nothing.  The frame
 * of an EMPTY array (|A| == 0) carries no geometry: there the call is stenos_hip_compress of B into [d_frame, d_frame +
 * capacity) under ctx's level and block-size settings, with THAT call's guarantees (bytes behind the returned size and inside
 * capacity are scratch, and an overflow may leave the buffer partly written).
 * d_index: NULL has the chain walked first (stenos_hip_frame_index's walk, whose cost grows with `bytes`).  An index that is
 * given may be the context's own; the two entries the call uses are checked before anything is written: header size <=
 * index[keep]; with r > 0, index[keep] + 4 <= index[keep + 1] <= bytes; with r == 0, index[keep] <= bytes -- else
 * STENOS_ERROR_INVALID_INPUT / STENOS_ERROR_SRC_OVERFLOW.  No kernel reads outside [d_frame, d_frame + bytes) or outside B,
 * whatever an index entry or a size field says.  After a successful call stenos_hip_last_index returns the index of the NEW
 * frame (the old entries 0 .. keep followed by the new ones): the next append, gather or update needs no walk.  A pointer
 * obtained earlier is invalid after the call (after an unsuccessful one too); an index passed in that is the context's own is
 * copied before the encoder overwrites that buffer.
 * WHAT IS CHECKED: only the last superblock of A, and only when it is partial (r > 0): it is decoded whole, and damage in it
 * gives STENOS_ERROR_SRC_OVERFLOW / STENOS_ERROR_INVALID_INPUT as in stenos_hip_decompress.  Everything in front of it is
 * neither read nor parsed: damage there is NOT detected by this call (with d_index == NULL the walk still sees every superblock
 * header) and stays in the frame.  A last superblock of A with a zstd-based code (one under 128 bytes of a level-1 frame; any
 * superblock of a level >= 2 frame, which a level-0/1 context may append to) is fetched and inflated on the host, which is
 * slow; a NEW last superblock under 128 bytes is coded on the host as the batch encoder does for its tiny items, which costs
 * one more small round trip.
 * HOW: append_plan checks the index entries and tells the host p; with r > 0 append_decode decodes superblock keep into a
 * stitch buffer and one device copy puts the first min(src_bytes, sb - r) bytes of B behind it -- B itself is not staged: the
 * rest is encoded straight from d_src + (sb - r), and with r == 0 nothing is staged at all; the stitched superblock and the
 * rest are encoded in ONE pass of the kernels of stenos_hip_compress_batch as two items without a frame header;
 * append_commit_plan, one thread per new superblock, makes the new index entries and the new size; append_commit copies the
 * streams behind p, 16 KiB per wavefront, and stores the size field.  Host round trips: the header, p with the status, the new
 * size with the status, and the wait for completion; launches and round trips depend neither on bytes, src_bytes nor the number
 * of superblocks.  The fused encoder of stenos_hip_compress does not take streams without a frame header, so large appends run
 * at the unfused encoder's rate.
 * DEVICE MEMORY kept by ctx, proportional to the re-encoded bytes r + src_bytes, never to the stored array: one superblock (the
 * stitch buffer); k * (sb + 4) + one superblock's worst case per stream (the encodings, k new superblocks); the batch
 * encoder's workspace for k superblocks (one padded slot per block of 256 * bytesoftype bytes, 16 bytes of tables per block, 21
 * per superblock: together about 3.2 * k * sb); and 8 bytes per superblock of the new frame for the index, twice.  The buffers
 * never shrink.
 * WHO IS SERVED BY WHAT -- MEASURED on MI355X (profiles/append_rate.txt, tools/append_rate.py: 1 GiB int32 rand12 frame of 8 192
 * superblocks, level 1, index passed in, medians of 20; against the only way without this call: stenos_hip_decompress into a scratch
 * tensor, the new bytes copied behind it, stenos_hip_compress of the concatenation back into the buffer, which leaves the same frame),
 * append / baseline in microseconds on a superblock boundary (r == 0) and behind half a superblock, device memory held:
 *     4 KiB      104 /    766  x7.38        186 /    797  x4.28     12 MiB against 1028 MiB
 *     1 MiB      157 /    747  x4.76        214 /    797  x3.73     16 MiB against 1028 MiB
 *    64 MiB      222 /    799  x3.61        280 /    844  x3.01     154 MiB against 1090 MiB
 *     1 GiB    1 517 /  1 527  x1.01      1 574 /  1 578  x1.00     2234 MiB against 2066 MiB
 * A store that grows by a batch at a time is served by this call: up to 64 MiB it is 3 to 7 times faster and holds a small share
 * of the memory.  Appending as much as is stored is a tie: the new bytes go through the unfused encoder, the baseline's through the
 * fused one, which pays for its decode of the old array.  Not measured: the walk (d_index == NULL), other element sizes, level 0. */
STENOS_EXPORT size_t stenos_hip_append(stenos_context* ctx, void* d_frame, size_t bytesoftype, size_t bytes, size_t capacity, const void* d_src,
				       size_t src_bytes, const uint64_t* d_index, void* stream);

/* stenos_hip_append over many frames in one call, IN PLACE: all arrays are host arrays of m.  Frame f is d_frames[f][0 ..
 * sizes[f]), the frame of an array A_f, in a buffer of capacities[f] >= sizes[f] bytes; d_srcs[f][0 .. src_sizes[f]) are the bytes
 * B_f, in device memory; they may have been written by earlier work on `stream`.  Afterwards d_frames[f] holds a frame of
 * A_f||B_f, for every f.  Returns 0 when the call ran, with results[f] the new frame sizes, or one error code for the whole
 * call.  Waits for completion (there is no _async form).  The contract is stenos_hip_append's, frame by frame: every frame ends
 * up holding, byte for byte and in size, what stenos_hip_append alone would leave for it -- for frames made by
 * stenos_hip_compress or stenos_hip_compress_batch at ctx's level into destinations of stenos_bound's size, the frame
 * stenos_hip_compress makes of A_f||B_f.  Each frame keeps its own header geometry; superblocks 0 .. keep_f of a frame are
 * never read or written.  Only what follows is new.
 * WRITES TO d_frames: all or nothing.  On success nothing outside each frame's 7 size bytes and [d_frames[f] + p_f, d_frames[f] +
 * results[f]).  On any error -- a host-side refusal, a refused index entry of any frame, damage in any partial last superblock,
 * any new frame larger than its capacity (STENOS_ERROR_DST_OVERFLOW) -- no byte of any buffer is written and results[] is left
 * alone: every byte of every frame goes through the last kernel (append_batch_commit), which is launched only after the status
 * and all new sizes have come back.  There is no per-frame partial success.
 * src_sizes[f] == 0: the frame is checked (its header, its two index entries) and not written; results[f] is the end of its
 * chain.  If all sources are empty, nothing is written anywhere.
 * The frame of an EMPTY array (|A_f| == 0) is how a page starts.  It carries no geometry: with src_sizes[f] > 0 its bytes are
 * encoded with a frame header under ctx's level and block-size setting, and the result is byte for byte what
 * stenos_hip_compress makes of B_f.  It goes through the same staging and the same last kernel, so all-or-nothing holds for
 * it too -- which is more than stenos_hip_append gives, which hands such a frame to stenos_hip_compress.
 * ONE GEOMETRY: the new superblocks of all frames are encoded in one pass, and that pass has one geometry, so all frames of
 * non-empty arrays must have one superblock size, and the size ctx would give the empty ones must equal it, else
 * STENOS_ERROR_INVALID_PARAMETER.  A store whose frames were made under one block-size setting (stenos_set_block_size, or none at
 * all: level 1 never shifts) is not affected.
 * Refused on the host, before any launch that writes, with nothing written: everything stenos_hip_append refuses, of any frame
 * (capacities[f] < sizes[f]; a size the 56-bit field cannot hold; bytesoftype outside 1..64; an unfinished _async job; ctx's
 * level >= 2, bytesoftype 1 at level 1, a time limit); m == 0 or above 2^31 - 1; a NULL in d_frames; a NULL source with a
 * non-zero size; a frame header stenos_hip_decompress refuses (that header's error code, for the first such frame); the old or
 * the new superblocks of all frames together plus m, or any grid, above 2^31 - 1; frames of different superblock sizes; two
 * frame buffers [d_frames[f], + capacities[f]) that overlap, or a source that overlaps a frame buffer (the host sorts the 2 m
 * intervals; the in-place commit would race with itself) -- STENOS_ERROR_INVALID_PARAMETER.  Sources may overlap each other.
 * d_index has the layout of stenos_hip_frames_index (S + m entries, frame f's slice at entry first[f] + f); NULL has the chains
 * walked first.  It may be the context's own (stenos_hip_last_frames_index): it is copied before the encoder overwrites that
 * buffer.  Per frame only the two entries stenos_hip_append uses are checked, by the same comparisons without sums, before
 * anything is written.  No kernel reads outside [d_frames[f], d_frames[f] + sizes[f]) or outside B_f, whatever an entry says.
 * After a successful call the context's index is that of the NEW frames, in the same layout: stenos_hip_last_frames_index
 * returns it, so a following stenos_hip_gather_rows_batch, stenos_hip_update_rows_batch or stenos_hip_append_batch walks
 * nothing.  After a failure stenos_hip_last_frames_index returns NULL and 0.  stenos_hip_last_index returns NULL, as after any
 * batch.
 * WHAT IS CHECKED: as in the single call -- of every frame only the last superblock of A_f, and only when it is partial: it is
 * decoded whole.  Everything in front of it is neither read nor parsed: damage there is NOT detected by this call and stays in
 * the frame.  A partial last superblock with a zstd-based code (one under 128 bytes of a level-1 frame; any superblock of a
 * level >= 2 frame) is fetched and inflated on the host, one frame at a time, which is slow; NEW last superblocks under 128
 * bytes are coded on the host as the batch encoder does for its tiny items, with one more round trip for all of them together.
 * HOW: the heads, the numbering and the walks are those of every call over many frames; append_batch_plan, one thread per
 * frame, runs the single call's entry checks and publishes p_f; append_batch_decode, one wavefront per frame with a partial last
 * superblock, decodes it into the frame's stitch slot of r_f + n0_f bytes (n0_f = min(src_sizes[f], sb - r_f): not a whole
 * superblock per frame); append_batch_stitch copies the first n0_f bytes of every B_f behind them; one pass of the kernels of
 * stenos_hip_compress_batch encodes up to 2 m items -- the stitched superblock of a frame, then the rest of B_f read where the
 * caller has it, both without a frame header; append_batch_commit_plan, one thread per new superblock, writes the new index
 * entries and checks every encoder length; append_batch_index moves the old entries 0 .. keep_f to the new layout;
 * append_batch_commit cuts the streams of all items into 16 KiB chunks, one per wavefront, and stores the size fields.  Host
 * round trips are three -- the heads, the status with the flags, the new sizes with the status -- and the wait for completion;
 * launches and round trips depend neither on the bytes nor on the superblocks, and on m only through the parallel walks of
 * chains longer than 256 superblocks and the host zstd paths: there is no copy and no launch per frame.
 * DEVICE MEMORY kept by ctx (S old, S' new superblocks in all frames; k_i new superblocks in item i of up to 2 m): about 1.3 KB
 * per frame (tables); 8 (S + m) + 8 (S' + m) (both indices); r_f + n0_f per frame, rounded up to 64 (the stitch slots); k_i *
 * (sb + 4) + one superblock's worst case PER ITEM (the encodings: every item is kept roomy, because the encoder's capacity
 * rules would change output bytes); and the batch encoder's workspace for all new superblocks (about 3.2 * sb each).  The
 * buffers never shrink.  Measured: 4 096 int32 frames of 64 KiB with 256 bytes appended to each hold 1 624 MiB, 0.40 MiB per frame,
 * of which the roomy room is 0.26 MiB per item; shrinking it is left for later.
 * WHO IS SERVED BY WHAT -- MEASURED on MI355X (profiles/append_batch_rate.txt, tools/append_batch_rate.py: int32 rand12, level 1,
 * index passed in, medians of 20; against the only way without this call: a loop of stenos_hip_append, one call per frame, each
 * given its frame's slice of a caller-held frames index -- which leaves the context with the index of the last frame only),
 * batch / baseline in microseconds, device memory held:
 *   4 096 frames of 64 KiB   256 B to every frame     1 370 / 736 730   x538     1 624 MiB against 2 MiB
 *                            4 KiB to every frame     1 340 / 739 773   x552     30 MiB more
 *                            256 B to every 16th        653 /  45 779   x70.1
 *   8 frames of 128 MiB      1 MiB each                 177 /   1 206   x6.81    20 MiB against 2 MiB
 *   1 frame of 1 GiB         4 KiB                      127 /     101   x0.79    (against stenos_hip_append itself)
 *                            64 MiB                     240 /     224   x0.93    140 MiB against 66 MiB
 * A store of many frames is served by this call: the loop pays the single call's fixed cost per frame, and leaves the context with
 * the index of the last frame only.  A store that is one frame stays with stenos_hip_append: there this call LOSES, by 21 % for
 * 4 KiB and by 7 % for 64 MiB.  Not measured: the walks (d_index == NULL), other element sizes, level 0. */
STENOS_EXPORT size_t stenos_hip_append_batch(stenos_context* ctx, size_t m, size_t bytesoftype, void* const* d_frames, const size_t* sizes,
					     const size_t* capacities, const void* const* d_srcs, const size_t* src_sizes, size_t* results,
					     const uint64_t* d_index, void* stream);

/* Whole-buffer byte kernels of the path on device memory (reference stenos/internal/shuffle.h:33,45 and
 * delta.h:34,39): byte transpose of `bytes / bytesoftype` elements and its inverse (leftover bytes copied),
 * byte delta in four quarter streams above 2048 bytes and its inverse.  src and dst must not overlap.
 * Return 0 or an error code. */
STENOS_EXPORT size_t stenos_hip_shuffle(const void* d_src, size_t bytesoftype, size_t bytes, void* d_dst, void* stream);
STENOS_EXPORT size_t stenos_hip_unshuffle(const void* d_src, size_t bytesoftype, size_t bytes, void* d_dst, void* stream);
STENOS_EXPORT size_t stenos_hip_delta(const void* d_src, void* d_dst, size_t bytes, void* stream);
STENOS_EXPORT size_t stenos_hip_delta_inv(const void* d_src, void* d_dst, size_t bytes, void* stream);

/* Host-pointer calls on several devices (the counterpart of the reference's thread dispatcher, stenos.cpp:909-1010,
 * 1151-1202: a host-pointer call is bound by the PCIe link of its device, the codec is an order of magnitude faster).
 * OPT-IN: by default a call stays on the calling thread's current device whatever stenos_set_threads() says -- that knob
 * means CPU threads to an unmodified caller (stenos.h:140), and the other devices of a process are usually some other
 * rank's.  After stenos_hip_set_devices(ctx, n >= 2) (or with STENOS_HIP_DEVICES >= 2 in the environment, read once, for
 * callers that cannot be changed) a stenos_compress_generic / stenos_decompress_generic call of 64 MiB or more at level
 * 0/1 with bytesoftype > 1 spreads over min(n, threads of stenos_set_threads, visible devices) devices, starting with the
 * calling thread's current one: every device takes a contiguous range of superblocks through a context and a host thread
 * of its own; frames are byte-identical to single-device frames.  n <= 1 turns it off again.
 * stenos_hip_last_devices returns how many devices the last host-pointer call on ctx used (1: the single-device path). */
STENOS_EXPORT void stenos_hip_set_devices(stenos_context* ctx, int devices);
STENOS_EXPORT int stenos_hip_last_devices(stenos_context* ctx);

/* Levels >= 2 (and bytesoftype 1) run a strategy layer on the host around the GPU passes (LZ4-dry estimates, zstd).  Wall
 * time per stage in milliseconds, summed over the calls on ctx since the last reset: out[0] GPU block pass + verdicts and
 * samples to the host, [1] estimates, [2] waiting for block streams from the device, [3] zstd, [4] frame layout, [5] waiting
 * for the frame's upload (device destinations), [6] zstd inflate (decompression), [7] device decode of the inflated
 * superblocks.  Transfers that are hidden behind zstd do not show.  Returns the number of stages; reset != 0 clears the sums. */
STENOS_EXPORT int stenos_hip_stage_ms(stenos_context* ctx, double* out, int n, int reset);

/* The fused encoder's waits for frame offsets are bounded; a launch that gives up (never observed) is redone without that
 * kernel instead of failing the call.  Returns how often that has happened on ctx. */
STENOS_EXPORT int stenos_hip_fused_fallbacks(stenos_context* ctx);

#ifdef STENOS_TEST_HOOKS
/* Switches for the test suite.  They exist only in the build the tests make for themselves (tests/hooks/Makefile,
 * -DSTENOS_TEST_HOOKS: tests/hooks/libstenos_hooks.so); libstenos.so neither declares nor exports them.
 * stenos_hip_test_lanes: share_current_device != 0 lets the "devices" of a multi-device call all stand for the current device
 * (one-GPU boxes); fail_lane >= 0 keeps that lane from running, as if its device could not be made current (-1: none).
 * stenos_hip_test_walk: serial != 0 makes frames that come without an index be walked by one lane (the serial walk that the
 * parallel one of walk.h is proven against, and falls back to); returns whether the last parallel walk on ctx fell back to
 * the serial one (1), did not (0), or there was none (-1).
 * stenos_hip_test_fused_timeouts: n > 0: the next n fused launches are treated as if they had given up waiting.  n = -1 - v,
 * v in 0..2: which fused encoder the calls on ctx launch from now on -- v = 0 the library's own rule (the default), 1 the plain
 * kernel, 2 the non-temporal one where the bytesoftype has it (4; the plain one elsewhere). */
STENOS_EXPORT void stenos_hip_test_lanes(stenos_context* ctx, int share_current_device, int fail_lane);
STENOS_EXPORT int stenos_hip_test_walk(stenos_context* ctx, int serial);
STENOS_EXPORT void stenos_hip_test_fused_timeouts(stenos_context* ctx, int n);
#endif

/* Kernel timing for benchmarks: when enabled, HIP events are recorded on the job's stream around the
 * dominant kernel of each direction: which = 0, the encoder (encode_superblocks, the fused kernel; encode_blocks
 * where that one does not apply), which = 1, decode_superblocks.  stenos_hip_kernel_ms returns the elapsed
 * milliseconds of the last such launch, or a negative value when none was recorded; it waits for the end event. */
STENOS_EXPORT void stenos_hip_set_profiling(stenos_context* ctx, int enabled);
STENOS_EXPORT double stenos_hip_kernel_ms(stenos_context* ctx, int which);

#ifdef __cplusplus
}
#endif
#endif
