// append.h -- host-visible interface of append_kernels.hip: bytes appended in place to one frame in device memory
// (stenos_hip_append).
//
// The array A of the frame has `keep` whole superblocks and r more bytes; B are the caller's bytes.
//   append_plan         checks the two index entries the call uses, reads the code byte of superblock `keep` inside the frame
//                       (a zstd-based code is flagged for the host), publishes p = idx[keep] and the status
//   append_decode       with r > 0: superblock `keep`, whole, -> the stitch buffer (one wavefront, the register path of
//                       decode_superblocks); a zstd-based code is left to the host
//   (the host copies the first min(|B|, sb - r) bytes of B behind the r decoded ones and has the stitched superblock and the
//   rest of B, straight from the caller's memory, encoded in one pass of the batch encoder as two items without a frame
//   header -> enc, enc_off)
//   append_commit_plan  one thread per new superblock: entry keep + j of the new index = p + the encoder's offset, every
//                       length checked, the streams' bytes and the new total for the host
//   append_commit       the streams -> frame + p, 16 KiB per wavefront; the 7 size bytes of the frame header.  The only
//                       kernel that writes to the frame.
#pragma once
#include "kernels.h"

#define APPEND_ARGS_ONLY
#include "append_codec.h" // AppendArgs, APPEND_W_*
#undef APPEND_ARGS_ONLY

hipError_t stenos_a_launch_plan(const AppendArgs& a, hipStream_t stream);
// raw: where the r decoded bytes go; total: bytes of A, sb: superblock bytes, T: bytesoftype
hipError_t stenos_a_launch_decode(const AppendArgs& a, uint8_t* raw, uint64_t total, uint32_t sb, uint32_t T, hipStream_t stream);
hipError_t stenos_a_launch_commit_plan(const AppendArgs& a, hipStream_t stream);
// len0, len1: the streams' bytes as append_commit_plan told the host (they size the grid; the kernel reads its own copy)
hipError_t stenos_a_launch_commit(const AppendArgs& a, uint64_t len0, uint64_t len1, hipStream_t stream);
