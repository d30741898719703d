// decode_body.h -- the work of one wavefront on one superblock of a frame, for decode_frames_batch
// (batch_decode_kernels.hip, many frames per launch).
//
// These are the steps of decode_superblocks (decode_kernels.hip), which keeps its own copy of them: called from there, this
// function changes that kernel's instruction listing (the inlined block decoder comes out with other operand orders and
// another schedule: a hundred lines of its listing and more differ, depending on how the arguments are passed), and the listing of the single-frame decoder is held fixed.  From the
// header checks on, the two copies are the same text (tests/test_batch_cpu.py keeps them so).
// The including translation unit is compiled with -structurizecfg-skip-uniform-regions (csrc/Makefile): nothing in here may
// branch on a lane-dependent value.
#pragma once
#include "kernels.h"

namespace codec {

// Superblock s of a.frame, whose header stands at a.sb_off[s].
template <uint32_t TT>
__device__ __forceinline__ void decode_superblock_entry(wv::Lds g_lds, const DecodeArgs& a, uint32_t s)
{
	using namespace wv;
	const uint32_t T = TT ? TT : a.T;
	const uint64_t p = a.sb_off[s];
	if (p > a.size || a.size - p < 4) { // (written without sums: an index entry may hold anything)
		status_or(a.status, DECODE_STATUS_TRUNCATED);
		return;
	}
	const uint32_t code = a.frame[p];
	const uint32_t csize = (uint32_t)a.frame[p + 1] | ((uint32_t)a.frame[p + 2] << 8) | ((uint32_t)a.frame[p + 3] << 16);
	const uint64_t begin = s * (uint64_t)a.sb_bytes;
	const uint32_t dsize = (uint32_t)((a.total_bytes - begin) < a.sb_bytes ? (a.total_bytes - begin) : a.sb_bytes);
	if (a.size - p - 4 < csize) { // stenos.cpp:1133-1134
		status_or(a.status, DECODE_STATUS_TRUNCATED);
		return;
	}
	const uint8_t* payload = a.frame + p + 4;
	uint8_t* out = a.dst + begin;
	if (code == 1) {
		const DecLayout L = make_dec_layout(T);
		uint32_t r = decode_superblock(g_lds, L, T, payload, csize, out, dsize, TT != 0);
		if (r == DEC_ERROR)
			status_or(a.status, DECODE_STATUS_INVALID);
	}
	else if (code == 6) { // stenos.cpp:741-746
		if (csize != dsize) {
			status_or(a.status, DECODE_STATUS_INVALID);
			return;
		}
		copy_g2g_wide<COPY_ROUNDS>(out, payload, csize); // (this kernel has registers to spare: more loads in flight per trip)
	}
	else if (code >= 2 && code <= 5) { // zstd based codes are finished by the host
		status_or(a.status, DECODE_STATUS_HOST_CODES);
	}
	else
		status_or(a.status, DECODE_STATUS_INVALID);
}

} // namespace codec
