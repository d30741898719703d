// gather.h -- host-visible interface of gather_kernels.hip: rows of one frame by row numbers that live on the device.
//
// Nothing about the rows is known on the host.  The kernels cut every row at the superblock boundaries of the frame
// (gather_codec.h, gather_cut), count the pieces per superblock, order them by superblock and decode every superblock that
// holds pieces once per 64 of them:
//   gather_count   one thread per (row i, piece j): the bounds check of the row number, count[superblock] += 1
//   gather_scan    ppre = exclusive sums of count, wpre = exclusive sums of ceil(count / 64) (nsb + 1 entries each); count := 0
//   gather_fill    the same threads: the piece goes to pieces[ppre[superblock] + count[superblock]++]
//   gather_decode  wavefront w finds its superblock by wpre[s] <= w < wpre[s + 1] and takes pieces
//                  ppre[s] + 64 (w - wpre[s]) ... of it, at most 64; wavefronts from wpre[nsb] on leave at once
#pragma once
#include "kernels.h"

#define GATHER_CUT_ONLY
#include "gather_codec.h"
#undef GATHER_CUT_ONLY

struct GatherArgs {
	const uint8_t* frame;
	uint64_t size;          // frame bytes
	const uint64_t* sb_off; // header offsets of the frame's superblocks
	const uint64_t* rows;   // n row numbers (device)
	uint8_t* dst;
	uint64_t n;
	uint64_t valid_rows;    // gather_valid_rows(): row numbers from here on make no piece and set DECODE_STATUS_BAD_ROW
	uint64_t npieces;       // n * P <= 2^31 - 1
	codec::GatherShape shape;
	uint32_t P;             // pieces per row
	uint32_t nsb;
	uint32_t T;
	uint32_t waves;         // grid of gather_decode: stenos_g_decode_waves()
	uint32_t* status;       // DECODE_STATUS_* of the call (zero on entry)
	uint32_t* count;        // nsb words, zero on entry
	uint32_t* sb_flags;     // nsb words, zero on entry: nonzero where a superblock with pieces has a zstd-based code
	uint32_t* ppre;         // nsb + 1
	uint32_t* wpre;         // nsb + 1
	codec::GatherPiece* pieces; // npieces entries
};

// Wavefronts gather_decode is launched with, known without asking the device: a superblock with c pieces takes ceil(c / 64),
// so all of them take at most (superblocks with pieces) + (pieces / 64) <= min(nsb, npieces) + npieces / 64.
inline uint64_t stenos_g_decode_waves(uint64_t nsb, uint64_t npieces) { return (nsb < npieces ? nsb : npieces) + npieces / 64; }

hipError_t stenos_g_launch_count(const GatherArgs& a, hipStream_t stream);
hipError_t stenos_g_launch_scan(const GatherArgs& a, hipStream_t stream);
hipError_t stenos_g_launch_fill(const GatherArgs& a, hipStream_t stream);
hipError_t stenos_g_launch_decode(const GatherArgs& a, hipStream_t stream);
