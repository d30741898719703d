// update_batch.h -- host-visible interface of update_batch_kernels.hip: rows of many frames replaced by (frame number, row
// number) pairs that live on the device, every updated frame written to a buffer of its own (stenos_hip_update_rows_batch).
//
// The sequence of update.h over the superblocks of all frames, numbered through (gather_codec.h, GatherFrame: g = first_f + s).
// The pairs are cut and grouped by superblock with the batched gather's own kernels (gather_batch.h: gather_batch_count,
// gather_scan, gather_batch_fill; a piece's 64-bit offset counts from the source rows).  Then:
//   update_batch_plan         the touched superblocks of all frames, ascending in g, in one compact list: slot[g], touched[c];
//                             a frame's touched superblocks are one run of it, its short last superblock at the end of the
//                             run.  Flags of zstd-based codes; K, and per frame (k_f, largest touched superblock) for the host
//   update_batch_decode       touched[c], whole, -> raw + c * sb: one wavefront each finds its frame in first[] and runs
//                             decode_superblock_entry (decode_body.h); zstd-based codes are left to the host
//   update_batch_apply        bytes [lo, hi) of slot slot[g] := the piece's bytes of its source row
//   (the host has the k_f slots of every touched frame encoded as one stream without a frame header, by the batch encoder's
//   kernels (batch.h), one FrameJob per frame: -> enc + enc_base[f], enc_off[c_f + f ...])
//   update_batch_splice_plan  checks every frame's old index, new length of every superblock, the new indices (the sums start
//                             again at every frame's header), the m new sizes for the host
//   update_batch_splice       superblock g -> outs[f] + new_idx[g + f], from enc or from the old frame; the frame headers.
//                             The only kernel that writes to the outputs.
// What a thread or a wavefront of each does is in update_codec.h.
#pragma once
#include "gather_batch.h"

#define UPDATE_ARGS_ONLY
#include "update_codec.h" // UpdateBatchArgs, UPDATE_W_*
#undef UPDATE_ARGS_ONLY

hipError_t stenos_ub_launch_plan(const UpdateBatchArgs& a, hipStream_t stream);
hipError_t stenos_ub_launch_decode(const UpdateBatchArgs& a, hipStream_t stream);
hipError_t stenos_ub_launch_apply(const UpdateBatchArgs& a, hipStream_t stream);
hipError_t stenos_ub_launch_splice_plan(const UpdateBatchArgs& a, hipStream_t stream);
hipError_t stenos_ub_launch_splice(const UpdateBatchArgs& a, hipStream_t stream);
