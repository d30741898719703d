// gather_ranges.h -- host-visible interface of gather_ranges_kernels.hip: variable-length ranges of one frame by offsets and
// lengths that live on the device (stenos_hip_gather_ranges).
//
// Nothing about the ranges is known on the host but their number n and the capacity of the packed output, which bound the pieces
// (gather_ranges_codec.h, ranges_piece_bound).  The kernels form the piece table gather_scan and gather_decode consume (gather.h):
//   ranges_sums    one thread per range: the validity test, (bytes, pieces) of the range; one sum of each per block of ranges
//   ranges_scan    ONE block: exclusive prefixes of the blocks' sums in place; D[n], the piece total, the overflow bit
//   ranges_apply   one thread per range: D[i] and pstart[i], the first piece slot of range i
//   ranges_count   one thread per piece slot t < pmax: its range by binary search in pstart, its piece cut, count[superblock] += 1
//   (gather_scan)
//   ranges_fill    the same threads: the piece goes to pieces[ppre[superblock] + count[superblock]++]
// Each launch is ordered behind the one in front of it by the stream and by nothing else: no workgroup waits for another.
// With DECODE_STATUS_BAD_ROW (an invalid range) or DECODE_STATUS_DST_OVERFLOW set, count and fill make no piece.
#pragma once
#include "gather.h"
#include "gather_ranges_codec.h"

constexpr uint32_t STENOS_GR_BLOCK = 256; // ranges per block of ranges_sums and ranges_apply

inline uint64_t stenos_gr_blocks(uint64_t n) { return (n + STENOS_GR_BLOCK - 1) / STENOS_GR_BLOCK; }

// ranges_sums, ranges_scan, ranges_apply: D, pstart, the words' total and piece count, the two gating bits
hipError_t stenos_gr_launch_offsets(const codec::RangesArgs& a, hipStream_t stream);
hipError_t stenos_gr_launch_count(const codec::RangesArgs& a, hipStream_t stream);
hipError_t stenos_gr_launch_fill(const codec::RangesArgs& a, hipStream_t stream);
