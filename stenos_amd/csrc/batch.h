// batch.h -- host-visible interface of the batch kernels (batch_kernels.hip, batch_decode_kernels.hip): many independent
// frames per launch.
//
// The host builds one FrameJob (DecodeArgs) per item whose pointers are already offset into the shared workspace, plus
// exclusive prefix sums of the items' blocks and superblocks (n + 1 entries each, the last one the total).  A workgroup
// finds its item by binary search of its unit number in the prefix array; the search is wave-uniform.
#pragma once
#include "kernels.h"

// per-item words of a compress batch (device): what enqueue_compress keeps in DeviceWords (host.h): total, encode_status, first_flagged
struct BatchItemState {
	uint64_t total;
	uint32_t status;
	uint32_t first_flagged;
};

// one tiny last superblock (< 128 bytes, zstd on the host): what comes to the host ...
struct BatchTinyIn {
	uint64_t off_last; // frame offset of the last superblock's header
	uint32_t status;   // the item's encode status so far
	uint32_t pad;
	uint8_t raw[128];  // its input bytes
};
// ... and what goes back: the payload (the item's override_payload points here), its code, size and the frame's end
struct BatchTinyOut {
	uint8_t payload[128];
	uint64_t end;
	uint32_t csize;
	uint32_t code; // 0: the item overflows its destination (nothing more is written for it)
};

#ifdef __HIPCC__
// item of unit x: pre[i] <= x < pre[i + 1] (items without units are passed over).  Every lane searches for the same x, so the
// loads are scalar.
__device__ __forceinline__ uint32_t stenos_b_find_item(const uint64_t* __restrict__ pre, uint32_t n, uint64_t x)
{
	uint32_t lo = 0, hi = n;
	while (hi - lo > 1) {
		const uint32_t mid = (lo + hi) >> 1;
		if (pre[mid] <= x)
			lo = mid;
		else
			hi = mid;
	}
	return lo;
}
#endif

// compress: blocks of all items (level >= 1), superblocks of all items, one wavefront per item for the scan and the capacity
// replay, the tiny last superblocks (tiny[k] = item of the k-th one), PACK_WAVES wavefronts per superblock
hipError_t stenos_b_launch_encode(const codec::FrameJob* jobs, const uint64_t* bpre, uint32_t n, uint64_t nblocks, uint32_t T, hipStream_t stream);
hipError_t stenos_b_launch_plan(const codec::FrameJob* jobs, const uint64_t* spre, uint32_t n, uint64_t nsb, hipStream_t stream);
hipError_t stenos_b_launch_scan(const codec::FrameJob* jobs, uint32_t n, hipStream_t stream);
hipError_t stenos_b_launch_resolve(const codec::FrameJob* jobs, uint32_t n, uint32_t T, hipStream_t stream);
hipError_t stenos_b_launch_tiny_gather(const codec::FrameJob* jobs, const uint32_t* tiny, uint32_t ntiny, BatchTinyIn* out, hipStream_t stream);
hipError_t stenos_b_launch_tiny_apply(const codec::FrameJob* jobs, const uint32_t* tiny, uint32_t ntiny, const BatchTinyOut* in, hipStream_t stream);
hipError_t stenos_b_launch_pack(const codec::FrameJob* jobs, const uint64_t* spre, uint32_t n, uint64_t nsb, uint32_t bps, hipStream_t stream);

// decompress: the first min(12, size) bytes of every frame to heads[12 i ..]; the serial chain walk of the items with
// walk[i] != 0 (one lane each); one wavefront per superblock of all items
hipError_t stenos_b_launch_heads(const uint8_t* const* frames, const uint64_t* sizes, uint32_t n, uint8_t* heads, hipStream_t stream);
hipError_t stenos_b_launch_walk(const DecodeArgs* args, const uint64_t* first, const uint8_t* walk, uint32_t n, hipStream_t stream);
hipError_t stenos_b_launch_decode(const DecodeArgs* args, const uint64_t* spre, uint32_t n, uint64_t nsb, uint32_t T, hipStream_t stream);
