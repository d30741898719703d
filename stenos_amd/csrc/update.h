// update.h -- host-visible interface of update_kernels.hip: rows of one frame replaced by row numbers that live on the device,
// the updated frame written to a second buffer (stenos_hip_update_rows).
//
// The rows are cut and grouped by superblock with the gather call's own kernels (gather.h: gather_count, gather_scan,
// gather_fill over a GatherArgs whose tables live in the update's buffer; a piece's 64-bit offset counts from the source rows).
// Then:
//   update_plan         the superblocks that hold pieces ("touched"), ascending, in a compact list: slot[s] = place of
//                       superblock s in it (UPDATE_NO_SLOT: untouched), touched[c] = the superblock in place c; a flag per touched
//                       superblock with a zstd-based code; k and the largest touched superblock number for the host
//   update_decode       touched superblock touched[c], whole, -> raw + c * sb (one wavefront each, the register path of
//                       decode_superblocks); zstd-based codes are left to the host
//   update_apply        bytes [lo, hi) of slot slot[s] := the piece's bytes of its source row
//   (the host has raw[0, (k - 1) * sb + bytes of the last touched superblock) encoded as k independent superblocks:
//   enqueue_compress without a frame header -> enc, enc_off[0 .. k])
//   update_splice_plan  checks the old index, new length of every superblock (touched: enc_off[c + 1] - enc_off[c], else
//                       idx[s + 1] - idx[s]), new_idx = header + exclusive sums, the new total for the host
//   update_splice       superblock s -> out + new_idx[s], from enc or from the old frame; the frame header.  The only kernel
//                       that writes to `out`.
#pragma once
#include "gather.h"


#define UPDATE_ARGS_ONLY
#include "update_codec.h" // UpdateArgs, UPDATE_W_*
#undef UPDATE_ARGS_ONLY

hipError_t stenos_u_launch_plan(const UpdateArgs& a, hipStream_t stream);
hipError_t stenos_u_launch_decode(const UpdateArgs& a, hipStream_t stream);
hipError_t stenos_u_launch_apply(const UpdateArgs& a, hipStream_t stream);
hipError_t stenos_u_launch_splice_plan(const UpdateArgs& a, hipStream_t stream);
hipError_t stenos_u_launch_splice(const UpdateArgs& a, hipStream_t stream);
