// append_batch.h -- host-visible interface of append_batch_kernels.hip: bytes appended in place to many frames in device memory
// in one call (stenos_hip_append_batch).
//
// The sequence of append.h over all frames (AppendBatchFrame: frame f's array A_f has keep_f whole superblocks and r_f more
// bytes, B_f are the caller's bytes; the old and the new index have the layout of every call over many frames, frame_batch.h):
//   append_batch_plan         one thread per frame: the single call's checks of the two index entries the frame uses, the code
//                             byte of superblock keep_f inside the frame (a zstd-based code is flagged for the frame), p_f
//                             published; the end of the chain of a frame nothing is appended to
//   append_batch_decode       one wavefront per frame with r_f > 0: superblock keep_f, whole, -> the frame's stitch slot
//                             (decode_superblock_entry, decode_body.h); a zstd-based code is left to the host
//   append_batch_stitch       the first n0_f = min(|B_f|, sb - r_f) bytes of every B_f behind the decoded bytes, 16 KiB per wavefront
//   (the host has the stitched superblocks and the rests of the B_f, read where the caller has them, encoded in one pass of the
//   batch encoder's kernels (batch.h) as up to 2 m items without a frame header; the one item of the frame of an empty array
//   carries a header)
//   append_batch_commit_plan  one thread per new superblock of all frames: the new index entries in the new layout, every
//                             encoder length checked, per frame the streams' bytes and the new total for the host
//   append_batch_index        one thread per old entry that moves unchanged to the new layout
//   append_batch_commit       the streams of all frames -> behind p_f, 16 KiB per wavefront; the 7 size bytes of every frame
//                             header.  The only kernel that writes to the frames.
// What a thread or a wavefront of each does is in append_batch_codec.h.
#pragma once
#include "kernels.h"

#define APPEND_BATCH_ARGS_ONLY
#include "append_batch_codec.h" // AppendBatchArgs, AppendBatchFrame
#undef APPEND_BATCH_ARGS_ONLY

hipError_t stenos_ab_launch_plan(const AppendBatchArgs& a, hipStream_t stream);
hipError_t stenos_ab_launch_decode(const AppendBatchArgs& a, hipStream_t stream);
// chunks: spre[m], which the host knows
hipError_t stenos_ab_launch_stitch(const AppendBatchArgs& a, uint64_t chunks, hipStream_t stream);
// K: kpre[m]
hipError_t stenos_ab_launch_commit_plan(const AppendBatchArgs& a, uint64_t K, hipStream_t stream);
// moved: mpre[m]
hipError_t stenos_ab_launch_index(const AppendBatchArgs& a, uint64_t moved, hipStream_t stream);
// chunks: cpre[2 m]
hipError_t stenos_ab_launch_commit(const AppendBatchArgs& a, uint64_t chunks, hipStream_t stream);
