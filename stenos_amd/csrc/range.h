// range.h -- host-visible interface of range_decode_kernels.hip: byte ranges of one frame, one wavefront per unit.
//
// The host cuts every range at the superblock boundaries of the frame (range_host.cpp).  A unit is the part of one range
// inside one superblock; units that share a superblock are decoded each on its own.
#pragma once
#include "kernels.h"

struct RangeUnit {
	uint8_t* dst; // where byte lo of the superblock goes (device memory, any alignment)
	uint32_t sb;  // superblock number
	uint32_t lo;  // 0 <= lo < hi <= bytes of that superblock
	uint32_t hi;
	uint32_t unused;
};

struct RangeArgs {
	const uint8_t* frame;
	uint64_t size;           // frame bytes
	const uint64_t* sb_off;  // header offsets of the frame's superblocks; NULL: every unit's header stands at direct_off
	uint64_t direct_off;
	const RangeUnit* units;
	uint32_t* unit_status;   // nunits words, every one written: DECODE_STATUS_* of the unit
	uint32_t* status;        // the OR of them (zero on entry)
	uint64_t total_bytes;
	uint32_t sb_bytes;
	uint32_t T;
	uint32_t nunits;
};

hipError_t stenos_r_launch_decode(const RangeArgs& a, hipStream_t stream);
