// host.h -- internal to the host side of libstenos.so (never installed): the types the units share, the framing helpers
// and the prototypes they call across.  One unit per concern: host_support.cpp (zstd loader, worker threads),
// encode_host.cpp (levels 0/1), strategy_host.cpp (levels >= 2), decode_host.cpp, batch_host.cpp, range_host.cpp, gather_host.cpp, gather_ranges_host.cpp, gather_batch_host.cpp, update_host.cpp, update_batch_host.cpp, append_host.cpp, append_batch_host.cpp, host_pointer.cpp and
// capi.cpp (the exported functions); frame_access.h is the front end of those that read a frame in device memory.  Everything here
// is hidden from the library's users (libstenos.map).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <functional>
#include <vector>

#include "../../include/stenos_hip.h"
#include "batch.h"
#include "kernels.h"
#include "strategy.h"

namespace stenos_host {

constexpr size_t kMaxT = STENOS_MAX_BYTESOFTYPE - 1; // stenos.h:65; above STENOS_K_LDS_MAX_T the kernels of kernels_wide.hip take over

inline bool is_err(size_t r) { return r >= STENOS_LAST_ERROR_CODE; }

// ---- zstd through dlopen: only for superblocks < 128 bytes (stenos.cpp:435-437) and for decoding code 2 ----
typedef size_t (*zstd_compress_fn)(void*, size_t, const void*, size_t, int);
typedef size_t (*zstd_decompress_fn)(void*, size_t, const void*, size_t);
typedef unsigned (*zstd_iserror_fn)(size_t);
typedef int (*zstd_maxclevel_fn)(void);
typedef void* (*zstd_createcctx_fn)(void);
typedef size_t (*zstd_freecctx_fn)(void*);
typedef size_t (*zstd_compresscctx_fn)(void*, void*, size_t, const void*, size_t, int);
struct Zstd {
	zstd_maxclevel_fn max_level = nullptr;
	zstd_compress_fn compress_once = nullptr;
	zstd_createcctx_fn create_cctx = nullptr;
	zstd_freecctx_fn free_cctx = nullptr;
	zstd_compresscctx_fn compress_cctx = nullptr;
	// ZSTD_compress allocates and frees a context of several hundred KB per call, which serialises dozens of worker
	// threads in the allocator; each thread keeps one context instead (ZSTD_compressCCtx, what the reference calls,
	// zstd_wrapper.h:81-83: same bytes)
	size_t compress(void* dst, size_t cap, const void* src, size_t n, int level) const
	{
		struct Holder {
			void* c = nullptr;
			zstd_freecctx_fn fr = nullptr;
			~Holder()
			{
				if (c && fr)
					fr(c);
			}
		};
		static thread_local Holder h;
		if (!h.c && create_cctx) {
			h.c = create_cctx();
			h.fr = free_cctx;
		}
		return h.c ? compress_cctx(h.c, dst, cap, src, n, level) : compress_once(dst, cap, src, n, level);
	}
	zstd_decompress_fn decompress = nullptr;
	zstd_iserror_fn is_error = nullptr;
	bool ok = false;
	Zstd(); // looks the library up (host_support.cpp)
};

struct DevBuf {
	void* p = nullptr;
	size_t cap = 0;
	bool ensure(size_t n)
	{
		if (n <= cap)
			return true;
		release();
		size_t want = (n + 4095) & ~(size_t)4095;
		if (hipMalloc(&p, want) != hipSuccess) {
			p = nullptr;
			return false;
		}
		cap = want;
		return true;
	}
	void release()
	{
		if (p)
			(void)hipFree(p);
		p = nullptr;
		cap = 0;
	}
	template <class T>
	T* as() const
	{
		return (T*)p;
	}
};

// Host staging of the strategy layer (levels >= 2): page-locked so the transfers run at link speed; plain malloc
// when the pinned allocation fails.  Kept by the context between calls.
struct HostBuf {
	uint8_t* p = nullptr;
	size_t cap = 0;
	bool pinned = false;
	bool ensure(size_t n)
	{
		if (n <= cap)
			return true;
		release();
		const size_t want = (n + (n >> 3) + 4095) & ~(size_t)4095;
		void* q = nullptr;
		if (hipHostMalloc(&q, want, hipHostMallocDefault) == hipSuccess)
			pinned = true;
		else {
			(void)hipGetLastError();
			q = malloc(want);
			pinned = false;
		}
		if (!q)
			return false;
		p = (uint8_t*)q;
		cap = want;
		return true;
	}
	void release()
	{
		if (p) {
			if (pinned)
				(void)hipHostFree(p);
			else
				free(p);
		}
		p = nullptr;
		cap = 0;
	}
	uint8_t* data() const { return p; }
};

// builds with -DSTENOS_HOST_TRACE: wall-clock of the host phases of the strategy layer on stderr (diagnostics)
// Wall time of the stages of a levels >= 2 call (the host's strategy layer around the GPU passes), summed per stage name
// into the context: stenos_hip_stage_ms() reads them (bench.py reports them); -DSTENOS_HOST_TRACE also prints every mark.
enum StageId { STAGE_GPU_PASS = 0, STAGE_ESTIMATES, STAGE_BLOCKS_TO_HOST, STAGE_ZSTD, STAGE_LAYOUT, STAGE_UPLOAD, STAGE_INFLATE, STAGE_DEVICE_FINISH, STAGE_COUNT };
struct PhaseTrace {
	double* acc; // STAGE_COUNT sums in milliseconds (nullptr: none)
	std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
	explicit PhaseTrace(double* sums = nullptr) : acc(sums) {}
	void mark(const char* what, int stage)
	{
		const auto n = std::chrono::steady_clock::now();
		const double ms = std::chrono::duration<double, std::milli>(n - t).count();
		if (acc)
			acc[stage] += ms;
#ifdef STENOS_HOST_TRACE
		fprintf(stderr, "[stenos] %-28s %8.2f ms\n", what, ms);
#else
		(void)what;
#endif
		t = n;
	}
};

inline void put_le(uint8_t* p, uint64_t v, int n)
{
	for (int i = 0; i < n; ++i)
		p[i] = (uint8_t)(v >> (8 * i));
}
inline uint64_t get_le(const uint8_t* p, int n)
{
	uint64_t v = 0;
	for (int i = 0; i < n; ++i)
		v |= (uint64_t)p[i] << (8 * i);
	return v;
}

// frame header: [shift][bytes:7] and, with a custom superblock size (shift 255), [sb:4]; returns its size
inline size_t write_frame_header(uint8_t* p, uint32_t shift, uint64_t bytes, size_t sb)
{
	p[0] = (uint8_t)shift;
	put_le(p + 1, bytes, 7);
	if (shift != 255)
		return 8;
	put_le(p + 8, sb, 4);
	return 12;
}
// superblock header: [code][size:3]
inline void write_superblock_header(uint8_t* p, uint32_t code, size_t size)
{
	p[0] = (uint8_t)code;
	put_le(p + 1, size, 3);
}
// compress_memcpy (stenos.cpp:363-374): a superblock stored as it is; returns its bytes in the frame
inline size_t copy_superblock(uint8_t* dst, const void* src, size_t bytes)
{
	write_superblock_header(dst, 6, bytes);
	memcpy(dst + 4, src, bytes);
	return bytes + 4;
}
// bytes of superblock s of a frame of `total` bytes
inline size_t superblock_bytes(uint64_t total, size_t sb, uint64_t s) { return (size_t)(total - s * sb < sb ? total - s * sb : sb); }

// stenos.cpp:71-76
inline size_t base_superblock(size_t block_size)
{
	if (block_size > STENOS_BLOCK_SIZE)
		return block_size;
	return (STENOS_BLOCK_SIZE / block_size) * block_size;
}

// The words at the start of ctx->misc (device memory) that the kernels of a job and the host share.  The kernels reach
// most of them through the pointers a FrameJob or DecodeArgs hands them; init_job (kernels.hip) writes total,
// encode_status, first_flagged, fused_copies and scan_carry by their byte offsets, which the asserts pin.
struct DeviceWords {
	uint64_t total;         // bytes of the frame so far
	uint32_t decode_status; // DECODE_STATUS_*
	uint32_t encode_status; // codec::ENCODE_STATUS_*
	uint32_t first_flagged; // FrameJob::first_flagged
	uint32_t fused_copies;  // superblocks the fused kernel stored as copies
	uint64_t scan_carry;
	uint8_t unused0[32];
	uint8_t override_payload[256]; // the tiny last superblock, coded by the host
	uint8_t unused1[8];
	uint32_t set_status[4]; // finish_host_codes: decode status of each set of buffers
};
// ctx->h_total (page-locked): a compress job's words up to scan_carry as the device left them (one copy), and the
// status words of the decode paths
struct PinnedWords {
	uint64_t total;
	uint32_t unused0;
	uint32_t encode_status;
	uint32_t first_flagged;
	uint32_t fused_copies;
	uint64_t unused1;
	uint32_t decode_status;
	uint32_t unused2;
	uint32_t set_status[4];
};
static_assert(offsetof(DeviceWords, total) == 0 && offsetof(PinnedWords, total) == 0, "init_job");
static_assert(offsetof(DeviceWords, decode_status) == 8, "misc layout");
static_assert(offsetof(DeviceWords, encode_status) == 12 && offsetof(PinnedWords, encode_status) == 12, "init_job");
static_assert(offsetof(DeviceWords, first_flagged) == 16 && offsetof(PinnedWords, first_flagged) == 16, "init_job");
static_assert(offsetof(DeviceWords, fused_copies) == 20 && offsetof(PinnedWords, fused_copies) == 20, "init_job");
static_assert(offsetof(DeviceWords, scan_carry) == 24, "init_job");
static_assert(offsetof(DeviceWords, override_payload) == 64 && offsetof(DeviceWords, set_status) == 328, "misc layout");
static_assert(offsetof(PinnedWords, decode_status) == 32 && offsetof(PinnedWords, set_status) == 40 && sizeof(PinnedWords) <= 64, "h_total layout");

} // namespace stenos_host

using stenos_host::DevBuf;
using stenos_host::DeviceWords;
using stenos_host::HostBuf;
using stenos_host::PinnedWords;

struct stenos_context_s {
	// parameters (stenos.cpp:94-106)
	int level = 1;
	int threads = 1;
	uint64_t max_nanoseconds = 0;
	size_t custom_shift = STENOS_NO_BLOCK_SHIFT;

	// device state
	bool probed = false, usable = false;
	DevBuf in, out;                                  // staging for the host-pointer ABI
	DevBuf slots, bsize, binfo, bneed, boff, sbcsize, sbneed, sbcode, sboff; // workspace of the encode pipeline / decode index
	DevBuf chain;                                    // fused path: ticket counter + one chained-scan word per superblock
	DevBuf tmp1, tmp2;                               // device scratch for superblocks that pass through zstd on the host (codes 3-5)
	DevBuf qprod, shuf, mid0, mid1;                  // levels >= 2: ratio checkpoints, shuffled input, plane middles (raw / delta'd)
	DevBuf walk;                                     // segments of the parallel header walk (walk.h)
	DevBuf dslots, dtab;                             // levels >= 2, device destinations: zstd output slots of two batches and their offset / size tables
	bool test_serial_walk = false;                   // (only the test build can set it) stenos_hip_test_walk: frames without an index are walked by one lane
	DevBuf wide;                                     // bytesoftype above 64: scratch of the HBM-resident kernels (kernels_wide.hip)
	DevBuf btab;                                     // batch calls: item tables and per-item words (stenos_hip_compress_batch / decompress_batch)
	DevBuf rtab, rsb;                                // range calls: status word, unit table and per-unit words (stenos_hip_decompress_ranges); one decoded superblock (codes 3, 4)
	DevBuf gtab;                                     // gather calls: status word, per-superblock counts, flags and prefixes, the piece table (stenos_hip_gather_rows)
	DevBuf grtab;                                    // gather of ranges: words, per-superblock counts, flags and prefixes, the piece table, per-range starts and the blocks' sums (stenos_hip_gather_ranges)
	DevBuf gbtab;                                    // batched gather calls: frame tables, walk arguments and the piece tables (stenos_hip_gather_rows_batch, stenos_hip_frames_index)
	DevBuf utab, uraw, uenc;                         // update calls: words, tables and both indices; the touched superblocks decoded; encoded again (stenos_hip_update_rows)
	DevBuf ubtab;                                    // batched update calls: frame tables, the piece tables, slots' lists, both indices, the encoder's item tables (stenos_hip_update_rows_batch)
	DevBuf atab, araw, aenc;                         // append calls: words, the encoder's item tables and the index; the stitched superblock; the new streams (stenos_hip_append)
	DevBuf abtab, abraw, abenc;                      // batched append calls: frame tables, the encoder's item tables, words and both indices; the stitch slots; the new streams (stenos_hip_append_batch)
	DevBuf misc;                                     // the words a job's kernels share with the host: DeviceWords, through words()
	HostBuf h_in, h_out, h_blocks, h_shuf, h_mid0, h_mid1, h_stage, h_tab; // host staging of the strategy layer
	HostBuf h_btab;                                  // batch calls: page-locked mirror of btab (tables up, per-item results down)
	HostBuf h_rtab;                                  // range calls: page-locked mirror of rtab
	HostBuf h_gtab;                                  // gather calls, zstd-based codes only: the row numbers and the superblock flags on the host
	HostBuf h_grtab;                                 // gather of ranges: the call's words as they come back (page-locked); zstd-based codes only: offsets, lengths and the superblock flags
	HostBuf h_gbtab;                                 // batched gather calls: page-locked mirror of gbtab's frame tables
	HostBuf h_utab;                                  // update calls, zstd-based codes only: the list of touched superblocks and the superblock flags on the host
	HostBuf h_ubtab;                                 // batched update calls: page-locked mirror of ubtab's tables of O(frames)
	HostBuf h_atab;                                  // append calls: page-locked mirror of atab's words and item tables
	HostBuf h_abtab;                                 // batched append calls: page-locked mirror of abtab's tables of O(frames)
	PinnedWords* h_total = nullptr;                  // what comes back of them (64 page-locked bytes)
	// last asynchronous job
	hipStream_t job_stream = nullptr;
	int job_kind = 0; // 0 none, 1 compress, 2 decompress
	size_t job_dst_size = 0, job_expected = 0;
	bool job_host_codes = false; // the last decode met zstd-based superblocks (finished on the host)
	size_t last_nsb = 0;
	bool last_batch = false; // the last call that touched the index workspace was a batch: stenos_hip_last_index has no index to give
	size_t last_frames = 0;  // entries of the many-frame index the context's index workspace holds (stenos_hip_last_frames_index); 0: none
	bool job_async = false;  // job_kind was set by an _async call (a batch call leaves such a job alone)
	// optional kernel timing (stenos_hip_set_profiling)
	bool profiling = false;
	hipEvent_t ev[4] = { nullptr, nullptr, nullptr, nullptr }; // encode start/stop, decode start/stop
	bool ev_valid[2] = { false, false };
	hipStream_t up_stream = nullptr, main_stream = nullptr; // chunked host-pointer calls: uploads / coding + downloads
	hipStream_t copy_stream = nullptr, upload_stream = nullptr; // levels >= 2: block streams to the host / the frame to the device, beside the host's zstd
	std::vector<hipEvent_t> batch_ev;   // ... one event per batch of superblocks
	std::vector<hipEvent_t> set_ev;     // ... and one per set of zstd output slots on their way to the device
	std::vector<hipStream_t> set_streams; // decode of zstd-based superblocks: one stream per set of inflated batches
	double stage_ms[16] = { 0 }; // levels >= 2: wall time per stage of the strategy layer, summed over the calls (stenos_hip_stage_ms)
	bool warm = false;    // a device call has gone through on this context (buffers, code objects and streams are up)
	int last_devices = 1; // devices the last host-pointer call used
	int hip_devices = 0;  // stenos_hip_set_devices: devices a host-pointer call may spread over (0: STENOS_HIP_DEVICES, else one)
	bool test_lanes_share_device = false; // stenos_hip_test_lanes: the lanes all use the current device (one-GPU test boxes)
	int test_fail_lane = -1;              // stenos_hip_test_lanes: this lane never runs (error-path test)
	// what the last compression was asked to do: a fused launch that gave up waiting is done again without the fused kernel
	const void* job_src = nullptr;
	void* job_dst = nullptr;
	size_t job_T = 0, job_bytes = 0;
	bool no_fused = false;
	int fused_fallbacks = 0;      // times that happened (stenos_hip_fused_fallbacks)
	int inject_chain_timeout = 0; // (only the test build can set it, stenos_hip_test_fused_timeouts) the next n fused launches are treated as if they had given up
	int test_fused_variant = 0;   // (only the test build can set it, stenos_hip_test_fused_timeouts(ctx, -1 - v)) v = 0: the rule of enqueue_compress, 1: plain, 2: nt
	bool fused_copy_heavy = false; // the last fused call on this context stored more than half its superblocks as copies
	uint64_t job_fused_nsb = 0;    // superblocks of the pending job's fused launch (0: none); its copy count comes back in fused_copies
	int device = -1; // the device the buffers above live on (the one that was current when they were first needed)
	// host-pointer calls with stenos_set_threads(ctx, n > 1): one child context per further device (or per stand-in lane),
	// used from a host thread of its own (multi_device below)
	std::vector<stenos_context_s*> lanes;


	DeviceWords* words() const { return misc.as<DeviceWords>(); }
	// the pending job; size: the destination's capacity (compress, kind 1) / the bytes expected (decompress, kind 2)
	void set_job(int kind, hipStream_t stream, bool async, size_t size)
	{
		job_kind = kind;
		job_async = async;
		job_stream = stream;
		(kind == 1 ? job_dst_size : job_expected) = size;
	}
	bool ensure_stream(hipStream_t* s) { return *s || hipStreamCreateWithFlags(s, hipStreamNonBlocking) == hipSuccess; }
	bool ensure_events(std::vector<hipEvent_t>& v, size_t n)
	{
		while (v.size() < n) {
			hipEvent_t e;
			if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess)
				return false;
			v.push_back(e);
		}
		return true;
	}
	// everything the context owns on a device: buffers, events and streams
	void release_device_state()
	{
		DevBuf* all[] = { &in, &out, &slots, &bsize, &binfo, &bneed, &boff, &sbcsize, &sbneed, &sbcode, &sboff, &misc, &tmp1, &tmp2, &qprod, &shuf, &mid0, &mid1, &chain, &wide, &walk, &dslots, &dtab, &btab, &rtab, &rsb, &gtab, &grtab, &gbtab, &utab, &uraw, &uenc, &ubtab, &atab, &araw, &aenc, &abtab, &abraw, &abenc };
		for (DevBuf* b : all)
			b->release();
		if (h_total)
			(void)hipHostFree(h_total);
		h_total = nullptr;
		for (hipEvent_t& e : ev)
			if (e) {
				(void)hipEventDestroy(e);
				e = nullptr;
			}
		ev_valid[0] = ev_valid[1] = false;
		for (hipStream_t* s : { &up_stream, &main_stream, &copy_stream, &upload_stream })
			if (*s) {
				(void)hipStreamDestroy(*s);
				*s = nullptr;
			}
		for (std::vector<hipEvent_t>* v : { &batch_ev, &set_ev }) {
			for (hipEvent_t e : *v)
				(void)hipEventDestroy(e);
			v->clear();
		}
		for (hipStream_t st : set_streams)
			(void)hipStreamDestroy(st);
		set_streams.clear();
		last_nsb = 0;
		last_batch = false;
		last_frames = 0;
		job_kind = 0;
	}
	bool device_ready()
	{
		int cur = -1;
		if (probed && usable && hipGetDevice(&cur) == hipSuccess && cur != device) {
			// the caller switched devices between calls: buffers of the old device are of no use on this one.  An asynchronous
			// job that is still pending there is waited for first (its stream outlives the switch); its result is lost to
			// stenos_hip_finish, which then reports that there is no job -- not a silent success.
			if (job_kind && job_stream)
				(void)hipStreamSynchronize(job_stream);
			release_device_state();
			probed = false;
			warm = false;
		}
		if (!probed) {
			probed = true;
			int n = 0;
			usable = hipGetDeviceCount(&n) == hipSuccess && n > 0 && hipGetDevice(&device) == hipSuccess;
			if (usable && hipHostMalloc((void**)&h_total, 64, hipHostMallocDefault) != hipSuccess)
				usable = false;
		}
		return usable;
	}
	~stenos_context_s()
	{
		for (stenos_context_s* l : lanes)
			if (l) {
				l->~stenos_context_s();
				free(l);
			}
		release_device_state();
		HostBuf* host[] = { &h_in, &h_out, &h_blocks, &h_shuf, &h_mid0, &h_mid1, &h_stage, &h_tab, &h_btab, &h_rtab, &h_gtab, &h_grtab, &h_gbtab, &h_utab, &h_ubtab, &h_atab, &h_abtab };
		for (HostBuf* b : host)
			b->release();
	}
	void mark(int idx, hipStream_t stream)
	{
		if (!profiling)
			return;
		if (!ev[idx] && hipEventCreate(&ev[idx]) != hipSuccess)
			return;
		if (hipEventRecord(ev[idx], stream) == hipSuccess && (idx & 1))
			ev_valid[idx >> 1] = true;
	}
};

namespace stenos_host {

struct FramePlan {
	size_t sb = 0;          // superblock bytes
	uint32_t shift = 0;     // frame byte 0 (255 = custom size follows)
	size_t header = 8;      // frame header bytes
	uint64_t nsb = 0, nfull = 0;
	uint32_t tail = 0, bps = 0;
};
struct FrameInfo {
	uint64_t total = 0;
	size_t sb = 0, header = 0;
	uint64_t nsb = 0;
};
// levels >= 2 and bytesoftype 1 go through the strategy layer (block codec on the GPU + zstd on the host)
inline bool needs_strategy(size_t T, int level) { return level >= 2 || (level == 1 && T == 1); }
// staging of the fused encoder, whichever of its kernels a call launches
inline size_t fused_stage_bytes_any(uint32_t T, uint32_t bps, uint64_t nsb)
{
	const size_t plain = stenos_k_fused_stage_bytes(T, bps, nsb, false), nt = stenos_k_fused_nt_supported(T) ? stenos_k_fused_stage_bytes(T, bps, nsb, true) : 0;
	return plain > nt ? plain : nt;
}

// host_support.cpp
Zstd& zstd();
void parallel_for(uint64_t cnt, const std::function<void(uint64_t)>& fn); // the worker threads of the zstd stages; the caller works too

// encode_host.cpp
size_t plan_frame(const stenos_context_s* ctx, size_t T, size_t bytes, int level, FramePlan& f);
size_t check_supported(const stenos_context_s* ctx, size_t T, int level);
uint64_t wide_scratch_bytes(size_t T, uint64_t units);
bool wide_scratch(stenos_context_s* ctx, size_t T, uint64_t units, uint8_t** p, uint64_t* bytes);
bool ensure_workspace(stenos_context_s* ctx, uint64_t blocks, uint64_t sbs, uint64_t frames);
bool frame_job(stenos_context_s* ctx, const FramePlan& f, size_t T, size_t bytes, uint64_t b0, uint64_t s0, uint64_t frame, codec::FrameJob& j);
constexpr size_t kTinyCapacity = 256;
inline size_t tiny_capacity(size_t room) { return room > kTinyCapacity ? kTinyCapacity : room; } // above ZSTD_compressBound(127) the capacity no longer matters
uint32_t tiny_superblock(const uint8_t* raw, size_t n, size_t room, uint8_t* out, size_t capacity, uint32_t* csize);
size_t enqueue_compress(stenos_context_s* ctx, const uint8_t* d_src, size_t T, size_t bytes, uint8_t* d_dst, size_t dst_size, int level, const FramePlan& f,
			bool frame_header, hipStream_t stream);
size_t compress_device(stenos_context_s* ctx, const void* d_src, size_t T, size_t bytes, void* d_dst, size_t dst_size, hipStream_t stream, bool wait);
size_t finish_job(stenos_context_s* ctx);

// strategy_host.cpp
size_t compress_strategy(stenos_context_s* ctx, const uint8_t* h_src, const uint8_t* d_src, size_t T, size_t bytes, uint8_t* h_dst, size_t dst_size, int level,
			 const FramePlan& f, hipStream_t stream, uint8_t* d_dst = nullptr);

// decode_host.cpp
size_t parse_frame(const uint8_t* h, size_t have, size_t T, size_t dst_size, FrameInfo& fi);
bool decode_args(stenos_context_s* ctx, const void* frame, size_t size, const uint64_t* sb_off, void* dst, uint64_t total, uint64_t nsb, size_t sb, size_t T,
		 uint32_t* status, DecodeArgs& a);
size_t finish_host_codes(stenos_context_s* ctx, const uint8_t* d_frame, const uint8_t* h_frame, size_t size, size_t T, const uint64_t* h_index, const FrameInfo& fi,
			 uint8_t* d_dst, hipStream_t stream);
size_t decompress_device(stenos_context_s* ctx, const void* d_src, size_t T, size_t size, void* d_dst, size_t dst_size, const uint64_t* d_index, const uint64_t* h_index,
			 const uint8_t* h_frame, hipStream_t stream, bool wait);
const uint64_t* frame_index(stenos_context_s* ctx, const void* d_src, size_t T, size_t bytes, size_t* nsb, hipStream_t stream);

// batch_host.cpp
size_t compress_batch(stenos_context_s* ctx, size_t n, size_t T, const void* const* d_srcs, const size_t* bytes, void* const* d_dsts, const size_t* dst_sizes,
		      size_t* results, hipStream_t stream);
size_t decompress_batch(stenos_context_s* ctx, size_t n, size_t T, const void* const* d_srcs, const size_t* src_sizes, void* const* d_dsts, const size_t* dst_sizes,
			size_t* results, hipStream_t stream);

// range_host.cpp
size_t decompress_ranges(stenos_context_s* ctx, const void* d_src, size_t T, size_t size, size_t n, const uint64_t* offsets, const uint64_t* lengths,
			 void* const* d_dsts, const uint64_t* d_index, hipStream_t stream);

// gather_host.cpp
size_t gather_rows(stenos_context_s* ctx, const void* d_src, size_t T, size_t size, size_t row_bytes, size_t n, const uint64_t* d_rows, void* d_dst,
		   size_t dst_stride, const uint64_t* d_index, hipStream_t stream);

// gather_ranges_host.cpp
size_t gather_ranges(stenos_context_s* ctx, const void* d_src, size_t T, size_t size, size_t n, const uint64_t* d_offsets, const uint64_t* d_lengths, void* d_dst,
		     size_t dst_size, uint64_t* d_dst_offsets, const uint64_t* d_index, hipStream_t stream);

// gather_batch_host.cpp
size_t gather_rows_batch(stenos_context_s* ctx, size_t m, size_t T, const void* const* d_frames, const size_t* sizes, size_t row_bytes, size_t n,
			 const uint64_t* d_frame_ids, const uint64_t* d_rows, void* d_dst, size_t dst_stride, const uint64_t* d_index, hipStream_t stream);
const uint64_t* frames_index(stenos_context_s* ctx, size_t m, size_t T, const void* const* d_frames, const size_t* sizes, size_t* entries, hipStream_t stream);

// update_batch_host.cpp
size_t update_rows_batch(stenos_context_s* ctx, size_t m, size_t T, const void* const* d_frames, const size_t* sizes, size_t row_bytes, size_t n,
			 const uint64_t* d_frame_ids, const uint64_t* d_rows, const void* d_src, size_t src_stride, void* const* d_outs, const size_t* out_sizes,
			 size_t* results, const uint64_t* d_index, hipStream_t stream);

// update_host.cpp
size_t update_rows(stenos_context_s* ctx, const void* d_frame, size_t T, size_t size, size_t row_bytes, size_t n, const uint64_t* d_rows, const void* d_src,
		   size_t src_stride, void* d_out, size_t out_size, const uint64_t* d_index, hipStream_t stream);

// append_host.cpp
size_t append(stenos_context_s* ctx, void* d_frame, size_t T, size_t size, size_t capacity, const void* d_src, size_t src_bytes, const uint64_t* d_index,
	      hipStream_t stream);

// append_batch_host.cpp
bool append_batch_overlap(size_t m, void* const* d_frames, const size_t* capacities, const void* const* d_srcs, const size_t* src_sizes);
size_t append_batch(stenos_context_s* ctx, size_t m, size_t T, void* const* d_frames, const size_t* sizes, const size_t* capacities, const void* const* d_srcs,
		    const size_t* src_sizes, size_t* results, const uint64_t* d_index, hipStream_t stream);

// host_pointer.cpp
size_t compress_host(stenos_context_s* ctx, const void* src, size_t T, size_t bytes, void* dst, size_t dst_size);
size_t decompress_host(stenos_context_s* ctx, const void* src, size_t T, size_t size, void* dst, size_t dst_size);

} // namespace stenos_host
