// gather_batch.h -- host-visible interface of gather_batch_kernels.hip: rows of many frames by (frame number, row number) pairs
// that live on the device (stenos_hip_gather_rows_batch).
//
// The sequence of gather.h over the superblocks of all frames, numbered through (gather_codec.h, GatherFrame: first_f + s):
//   gather_batch_count   one thread per (pair i, piece j of the call's P): the checks of the pair, count[first_f + s] += 1
//   gather_scan          gather.h's, over the S superblocks of the batch
//   gather_batch_fill    the same threads: the piece goes to pieces[ppre[g] + count[g]++]
//   gather_batch_decode  wavefront w finds its superblock g by wpre[g] <= w < wpre[g + 1], the frame by first[f] <= g < first[f + 1]
//                        and takes up to 64 pieces of it, by the rule gather_decode follows (gather_codec.h, decode_gather_chunk);
//                        wavefronts from wpre[S] on leave at once
// The numbering and the index are those of every call over many frames (frame_batch.h): frame f's nsb_f + 1 offsets start at entry
// f + first_f, so the header of superblock g of frame f is entry g + f.
#pragma once
#include "gather.h"

struct GatherBatchArgs {
	const codec::GatherFrame* frames; // m entries
	const uint64_t* first;            // m + 1: first[f] = frames[f].first, first[m] = S
	const uint64_t* sb_off;           // S + m offsets
	const uint64_t* frame_ids;        // n (device)
	const uint64_t* rows;             // n (device)
	uint8_t* dst;
	uint64_t row_bytes, dst_stride;
	uint64_t npieces;                 // n * P <= 2^31 - 1
	uint32_t m;
	uint32_t P;                       // pieces per pair: the largest of the frames'
	uint32_t S;                       // superblocks of all frames
	uint32_t T;
	uint32_t waves;                   // grid of gather_batch_decode: stenos_g_decode_waves(S, npieces)
	uint32_t* status;                 // DECODE_STATUS_* of the call (zero on entry)
	uint32_t* count;                  // S words, zero on entry
	uint32_t* sb_flags;               // S words, zero on entry: nonzero where a superblock with pieces has a zstd-based code
	uint32_t* ppre;                   // S + 1
	uint32_t* wpre;                   // S + 1
	codec::GatherPiece* pieces;       // npieces entries
};

hipError_t stenos_gb_launch_count(const GatherBatchArgs& a, hipStream_t stream);
hipError_t stenos_gb_launch_fill(const GatherBatchArgs& a, hipStream_t stream);
hipError_t stenos_gb_launch_decode(const GatherBatchArgs& a, hipStream_t stream);
