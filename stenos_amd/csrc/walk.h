// walk.h -- the superblock chain of a frame, found in parallel.
//
// A frame is [header] then per superblock [code][csize:3][payload of csize bytes] (stenos.cpp:862-907); the decoder finds
// superblock s by walking the chain of headers from the first one (stenos.cpp:1126-1134, 1166-1182).  One lane doing that
// on a device-resident frame pays a dependent HBM read per superblock (0.35 us each: 23 ms for the 65 536 superblocks of
// 8 GiB of int32, ten times the decode kernel).  Here the chain is cut into segments of the frame that are walked
// concurrently, and the result is EXACTLY the serial walk's:
//
//   A  speculate  segment k (one wavefront) looks at every byte position of the window [B_k, B_k + W), W = superblock
//                 size + 4 = the longest hop, for headers that look like one (code 1..6, csize <= superblock size) and hop
//                 out of the window: the "roots".  The last header of the true chain inside the window is one of them.
//                 All roots are followed in lock step, one per lane, while the headers they land on look like headers.
//                 Chains that start inside payload bytes die within a hop or two (a random position looks like a header
//                 with probability 2e-4); the survivor's root r_k, exit x_k (first position at or behind B_k+1) and number
//                 of hops are recorded (several survivors that have merged into one chain, up to four, are all kept).  Segment 0 starts at the first header and needs no window.
//   B  verify     segment k hops from x_k-1 -- plain hops, nothing is assumed about the bytes -- until it reaches r_k or
//                 passes it.  Reaching it proves by induction that x_k-1 -> ... -> r_k -> ... -> x_k is the serial chain.
//                 The hops are counted.  The last segment is walked to the end of the frame (no speculation).
//   C  write      segment k sums the counts in front of it and hops once more from x_k-1, writing the offsets.
//
// Anything else -- no survivor, survivors that disagree, a walk that passes its root, a chain that ends early -- raises a flag and the
// serial walk runs after all (frames that are malformed, or that hold whole Stenos frames inside stored superblocks
// aligned just so; never a wrong index).
//
// Written as per-lane functions for host and device: tests/emul runs them lane by lane against the serial walk.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define WALK_HD __host__ __device__ inline
#else
#define WALK_HD inline
#endif

namespace walk {

#ifndef STENOS_WALK_MAX_SEGMENTS
#define STENOS_WALK_MAX_SEGMENTS 2048
#endif
#ifndef STENOS_WALK_SEG_WINDOWS
#define STENOS_WALK_SEG_WINDOWS 4
#endif
constexpr uint32_t MAX_SEGMENTS = STENOS_WALK_MAX_SEGMENTS;
constexpr uint32_t LANES = 64;
constexpr uint32_t MIN_SEGMENTS = 4;       // below, the serial walk
constexpr uint32_t SEG_WINDOWS = STENOS_WALK_SEG_WINDOWS; // a segment is at most this many windows long, unless the frame needs more than MAX_SEGMENTS of them
constexpr uint32_t PROOF_HOPS = 2;         // plausible headers a speculated chain must meet behind its segment
enum : uint32_t { SEG_UNRESOLVED = 0, SEG_OK = 1 };
enum : uint32_t { WALK_FAILED = 1 };

struct Plan {
	uint64_t first, size, nsb; // offset of the first superblock header, frame bytes, superblocks the frame header announces
	uint64_t seg_len;          // bytes per segment
	uint32_t nseg;             // 0: serial walk
	uint32_t window;           // W
	uint32_t sb_bytes;
};
constexpr uint32_t MAX_ROOTS = 4; // speculated chains of a segment that survive (they have merged: one exit)
struct Segment {
	uint64_t exit;
	uint64_t count; // phase B: chain positions inside the segment
	uint32_t state, nroots;
	uint64_t root[MAX_ROOTS];
	uint32_t hops[MAX_ROOTS];
};

WALK_HD uint64_t seg_begin(const Plan& P, uint32_t k) { return P.first + (uint64_t)k * P.seg_len; }
WALK_HD uint64_t seg_end(const Plan& P, uint32_t k) { return k + 1 >= P.nseg ? ~0ull : P.first + (uint64_t)(k + 1) * P.seg_len; }

// seg_len_override: tests force short segments
inline Plan make_plan(uint64_t first, uint64_t size, uint64_t nsb, uint32_t sb_bytes, uint64_t seg_len_override = 0)
{
	Plan P;
	P.first = first;
	P.size = size;
	P.nsb = nsb;
	P.sb_bytes = sb_bytes;
	P.window = sb_bytes + 4;
	P.nseg = 0;
	P.seg_len = 0;
	if (size <= first || nsb < 2 * MIN_SEGMENTS)
		return P;
	const uint64_t span = size - first;
	// Segment length: a few windows.  (One window per segment would suit frames of small payloads -- sorted keys: 2 KB per
	// 128 KiB superblock, 230 serial hops per segment in phases B and C -- but then a false chain only has to survive a hop or
	// two, and structured payloads hold enough header look-alikes for several to survive with different exits: measured, the
	// 8 GiB sorted frame then falls back to the serial walk.)
	uint64_t len = seg_len_override ? seg_len_override : (uint64_t)P.window * SEG_WINDOWS;
	if (len < P.window)
		len = P.window;
	if ((span + len - 1) / len > MAX_SEGMENTS)
		len = (span + MAX_SEGMENTS - 1) / MAX_SEGMENTS;
	len = (len + 15) & ~15ull;
	const uint64_t n = (span + len - 1) / len;
	if (n < MIN_SEGMENTS)
		return P;
	P.seg_len = len;
	P.nseg = (uint32_t)n;
	return P;
}

WALK_HD bool readable(const Plan& P, uint64_t p) { return p <= P.size && P.size - p >= 4; }
typedef uint32_t __attribute__((aligned(1))) u32_unaligned;
WALK_HD uint32_t header_word(const uint8_t* frame, uint64_t p) { return *(const u32_unaligned*)(frame + p); } // little endian: code | csize << 8
WALK_HD bool plausible(const Plan& P, uint32_t w) { return (w & 0xFFu) - 1u < 6u && (w >> 8) <= P.sb_bytes; }
WALK_HD uint64_t hop(uint64_t p, uint32_t w) { return p + 4 + (uint64_t)(w >> 8); }

// ---- phase A ----------------------------------------------------------------------------------------------
// Positions [base, base + 16) of segment k's window: appends the roots among them to roots[0..64) (count in *nroots, which
// may run past 64: the caller then gives the segment up).  add(counter) must return the old value and add one atomically.
template <class Add>
WALK_HD void scan_window16(const Plan& P, const uint8_t* frame, uint32_t k, uint64_t base, uint64_t* roots, uint32_t* nroots, Add add)
{
	const uint64_t wend = seg_begin(P, k) + P.window;
	uint32_t w[5];
	if (base + 20 <= P.size) {
		for (int i = 0; i < 5; ++i)
			w[i] = header_word(frame, base + 4 * (uint64_t)i);
	}
	else {
		for (int i = 0; i < 5; ++i) {
			w[i] = 0;
			for (int b = 0; b < 4; ++b) {
				const uint64_t q = base + 4 * (uint64_t)i + (uint64_t)b;
				if (q < P.size)
					w[i] |= (uint32_t)frame[q] << (8 * b);
			}
		}
	}
	// First a filter on the sixteen code bytes at once: a byte b is a candidate when b - 1 < 8 (codes 1..6 and two more:
	// the price of doing it on four bytes per instruction); 3 % of the bytes of a payload pass and get the full test.
	uint32_t cand = 0;
	for (int i = 0; i < 4; ++i) {
		const uint32_t y = (w[i] | 0x80808080u) - 0x01010101u;                   // per byte (b - 1) mod 128, no borrow between bytes
		const uint32_t z = (y & 0x78787878u) | (w[i] & 0x80808080u);             // zero byte: b in 1..8
		const uint32_t nz = ((z & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | z;               // bit 7 of every byte: the byte is not zero
		const uint32_t f = ~nz & 0x80808080u;
		cand |= (((f >> 7) & 1u) | ((f >> 14) & 2u) | ((f >> 21) & 4u) | ((f >> 28) & 8u)) << (4 * i);
	}
	while (cand) {
		const uint32_t j = (uint32_t)__builtin_ctz(cand);
		cand &= cand - 1u;
		const uint64_t p = base + j;
		if (p >= wend || !readable(P, p))
			break;
		const uint32_t sh = (j & 3u) * 8u;
		const uint32_t h = sh ? (w[j >> 2] >> sh) | (w[(j >> 2) + 1] << (32u - sh)) : w[j >> 2];
		if (plausible(P, h) && hop(p, h) >= wend) {
			// (payload bytes look like a header two hundred times per window of 128 KiB: where they point must look like one too)
			const uint64_t q = hop(p, h);
			if (readable(P, q) ? !plausible(P, header_word(frame, q)) : q != P.size)
				continue;
			const uint32_t idx = add(nroots);
			if (idx < LANES)
				roots[idx] = p;
		}
	}
}
// ---- phase A as walk_speculate runs it: scan_window16 cut into its parts --------------------------------------------
// The same roots as scan_window16 (the same set, the same count; tests/emul_walk_scan replays both on the same windows), but
//   * the bytes of a step are loaded apart from their test (scan_load16), so that a lane can have several steps' loads in flight;
//   * the filter looks at two bytes of a position, the code and the top byte of the size (scan_candidates16);
//   * what passes the filter is not looked at on the spot, a lane at a time with the others of its wavefront waiting, twice, for
//     memory: it goes to a list (scan_list16) that is gone through afterwards, one entry per lane, with all loads in flight
//     (scan_deferred).  A full list sends a candidate to its exact test at once: the result does not depend on the list's size.
#ifndef STENOS_WALK_SCAN_STEPS
#define STENOS_WALK_SCAN_STEPS 4 // (8: 70 vector registers, seven waves per SIMD, and the 2 048 workgroups of a long frame need a second round)
#endif
constexpr uint32_t SCAN_STEPS = STENOS_WALK_SCAN_STEPS; // steps of 16 positions whose bytes a lane requests before it looks at the first
constexpr uint32_t DEFER_CAP = 2048;                    // candidates that wait in the list for their exact test
struct ScanFilter {
	uint32_t add; // per byte: 0x7F - (the largest top size byte & 0x7F)
	uint32_t hi;  // the largest top size byte is 128 or more
};
WALK_HD ScanFilter scan_filter(const Plan& P)
{
	const uint32_t top = (P.sb_bytes >> 16) > 255u ? 255u : (P.sb_bytes >> 16);
	ScanFilter F;
	F.add = (0x7Fu - (top & 0x7Fu)) * 0x01010101u;
	F.hi = top >> 7;
	return F;
}
// the 20 bytes at base, all of them inside the frame (base + 20 <= size)
WALK_HD void scan_load16(const uint8_t* frame, uint64_t base, uint32_t* w)
{
	for (int i = 0; i < 5; ++i)
		w[i] = header_word(frame, base + 4 * (uint64_t)i);
}
// ... and the last steps of a frame, byte by byte: zeros behind the frame's end
WALK_HD void scan_load16_bytes(const Plan& P, const uint8_t* frame, uint64_t base, uint32_t* w)
{
	for (int i = 0; i < 5; ++i) {
		w[i] = 0;
		for (int b = 0; b < 4; ++b) {
			const uint64_t q = base + 4 * (uint64_t)i + (uint64_t)b;
			if (q < P.size)
				w[i] |= (uint32_t)frame[q] << (8 * b);
		}
	}
}
// Bit j: position base + j may hold a plausible header -- its code byte is in 1..8 and the top byte of its size is at most
// that of the superblock size.  A superset of plausible(); about one payload byte in 2 000 passes where 3 % pass the code alone.
WALK_HD uint32_t scan_candidates16(ScanFilter F, const uint32_t* w)
{
	uint32_t f[4], any = 0;
	for (int i = 0; i < 4; ++i) {
		const uint32_t y = (w[i] | 0x80808080u) - 0x01010101u; // per byte (b - 1) mod 128, no borrow between bytes
		const uint32_t c = (y & 0x78787878u) + 0x78787878u;    // bit 7: (b - 1) mod 128 is 8 or more; with bit 7 of b itself: b is not in 1..8
		const uint32_t t = (w[i] >> 24) | (w[i + 1] << 8);     // the bytes three positions on
		const uint32_t s = (t & 0x7F7F7F7Fu) + F.add;          // bit 7: the low seven bits are above the bound's
		const uint32_t gt = F.hi ? t & s : t | s;              // bit 7: the byte is above the bound
		f[i] = ~(c | w[i] | gt) & 0x80808080u;
		any |= f[i];
	}
	if (!any) // (nearly always: the bits are put together for the few)
		return 0;
	uint32_t cand = 0;
	for (int i = 0; i < 4; ++i)
		cand |= (((f[i] >> 7) & 1u) | ((f[i] >> 14) & 2u) | ((f[i] >> 21) & 4u) | ((f[i] >> 28) & 8u)) << (4 * i);
	return cand;
}
// The exact test of position p, as scan_window16 makes it: a root when it is inside the window and holds a plausible header that
// hops out of the window onto another plausible header, or onto the frame's end.
template <class Add>
WALK_HD void scan_test(const Plan& P, const uint8_t* frame, uint32_t k, uint64_t p, uint64_t* roots, uint32_t* nroots, Add add)
{
	const uint64_t wend = seg_begin(P, k) + P.window;
	if (p >= wend || !readable(P, p))
		return;
	const uint32_t h = header_word(frame, p);
	const uint64_t q = hop(p, h);
	if (!plausible(P, h) || q < wend)
		return;
	if (readable(P, q) ? !plausible(P, header_word(frame, q)) : q != P.size)
		return;
	const uint32_t idx = add(nroots);
	if (idx < LANES)
		roots[idx] = p;
}
// The candidates among positions [base, base + 16) go to list[0..DEFER_CAP) as offsets from the segment's begin; *nlist may run
// past DEFER_CAP: those candidates have had their exact test here.  add as for scan_window16.
template <class Add>
WALK_HD void scan_list16(const Plan& P, const uint8_t* frame, uint32_t k, uint64_t base, uint32_t cand, uint64_t* roots, uint32_t* nroots, uint32_t* list,
			 uint32_t* nlist, Add add)
{
	const uint32_t at = (uint32_t)(base - seg_begin(P, k));
	while (cand) {
		const uint32_t j = (uint32_t)__builtin_ctz(cand);
		cand &= cand - 1u;
		const uint32_t d = add(nlist);
		if (d < DEFER_CAP)
			list[d] = at + j;
		else
			scan_test(P, frame, k, base + j, roots, nroots, add);
	}
}
// One lane's share of segment k's window, for a workgroup of SCAN_THREADS lanes.  A step is 16 positions per lane, STEP_BYTES
// for the workgroup.  The steps are taken SCAN_STEPS at a time while every lane of every one of them has the first of its 16
// positions inside the window and its 20 bytes inside the frame: all loads of such a group are requested before the first is
// looked at.  What is left -- the window's last positions, the last steps of a frame -- goes step by step, byte by byte where the
// frame ends; lanes behind the window's end request nothing.
constexpr uint32_t SCAN_THREADS = 256;
constexpr uint32_t STEP_BYTES = SCAN_THREADS * 16u, GROUP_BYTES = SCAN_STEPS * STEP_BYTES;
WALK_HD uint32_t scan_groups(const Plan& P, uint32_t k)
{
	const uint64_t begin = seg_begin(P, k);
	const uint64_t in_frame = P.size >= begin + 4 ? P.size - begin - 4 : 0; // a group ends here at the latest: its last lane reads 4 bytes more
	const uint64_t in_window = (uint64_t)P.window + 15u;                  // ... and here: its last lane's first position is inside the window
	return (uint32_t)((in_frame < in_window ? in_frame : in_window) / GROUP_BYTES);
}
template <class Add>
WALK_HD void scan_lane(const Plan& P, const uint8_t* frame, uint32_t k, uint32_t lane, uint64_t* roots, uint32_t* nroots, uint32_t* list, uint32_t* nlist,
		       Add add)
{
	const uint64_t begin = seg_begin(P, k), wend = begin + P.window;
	const ScanFilter F = scan_filter(P);
	const uint32_t groups = scan_groups(P, k);
	for (uint32_t g = 0; g < groups; ++g) {
		const uint64_t from = begin + (uint64_t)g * GROUP_BYTES;
		uint32_t w[SCAN_STEPS][5];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
		for (uint32_t u = 0; u < SCAN_STEPS; ++u)
			scan_load16(frame + from, u * STEP_BYTES + lane * 16u, w[u]);
#if defined(__HIP_DEVICE_COMPILE__)
		__builtin_amdgcn_sched_barrier(0); // (left alone, the scheduler puts the first step's filter, and a wait, in front of the later steps' loads)
#pragma unroll
#endif
		for (uint32_t u = 0; u < SCAN_STEPS; ++u) {
			const uint32_t cand = scan_candidates16(F, w[u]);
			if (cand)
				scan_list16(P, frame, k, from + u * STEP_BYTES + lane * 16u, cand, roots, nroots, list, nlist, add);
		}
	}
	for (uint64_t base = begin + (uint64_t)groups * GROUP_BYTES + lane * 16u; base < wend; base += STEP_BYTES) {
		uint32_t w[5];
		if (base + 20 <= P.size)
			scan_load16(frame, base, w);
		else
			scan_load16_bytes(P, frame, base, w);
		const uint32_t cand = scan_candidates16(F, w);
		if (cand)
			scan_list16(P, frame, k, base, cand, roots, nroots, list, nlist, add);
	}
}
// entry i of the list (i < min(*nlist, DEFER_CAP))
template <class Add>
WALK_HD void scan_deferred(const Plan& P, const uint8_t* frame, uint32_t k, const uint32_t* list, uint32_t i, uint64_t* roots, uint32_t* nroots, Add add)
{
	scan_test(P, frame, k, seg_begin(P, k) + list[i], roots, nroots, add);
}

// one lane follows one root while the headers look like headers; false: the chain broke
WALK_HD bool follow_root(const Plan& P, const uint8_t* frame, uint32_t k, uint64_t root, uint64_t* exit, uint32_t* hops)
{
	const uint64_t end = seg_end(P, k);
	uint64_t p = root;
	uint32_t n = 0;
	while (p < end && readable(P, p)) {
		const uint32_t w = header_word(frame, p);
		if (!plausible(P, w))
			return false;
		p = hop(p, w);
		++n;
	}
	*exit = p;
	*hops = n;
	// a chain that leaves the segment after a hop or two has proven little: the next headers must look like headers too
	for (uint32_t extra = 0; extra < PROOF_HOPS && readable(P, p); ++extra) {
		const uint32_t w = header_word(frame, p);
		if (!plausible(P, w))
			return false;
		p = hop(p, w);
	}
	// ... and a chain that ends, ends with the frame (a hop out of a truncated frame proves nothing: the serial walk sorts that out)
	return readable(P, p) || p == P.size;
}
// segment 0: plain hops from the first header
WALK_HD void follow_first(const Plan& P, const uint8_t* frame, Segment* s)
{
	const uint64_t end = seg_end(P, 0);
	uint64_t p = P.first;
	uint32_t n = 0;
	while (p < end && readable(P, p) && n <= P.nsb) {
		p = hop(p, header_word(frame, p));
		++n;
	}
	s->nroots = 1;
	s->root[0] = P.first;
	s->exit = p;
	s->hops[0] = n;
	s->state = p >= end || !readable(P, p) ? SEG_OK : SEG_UNRESOLVED;
	s->count = n;
}

// ---- phase B ----------------------------------------------------------------------------------------------
// false: the speculation does not hold, the serial walk has to run
WALK_HD bool verify_segment(const Plan& P, const uint8_t* frame, uint32_t k, Segment* seg)
{
	if (k == 0)
		return seg[0].state == SEG_OK;
	if (seg[k - 1].state != SEG_OK)
		return false;
	uint64_t p = seg[k - 1].exit;
	uint64_t n = 0;
	if (k + 1 < P.nseg) {
		if (seg[k].state != SEG_OK || p < seg_begin(P, k))
			return false;
		// the roots that survived have merged into one chain: the true chain meets exactly one of them
		uint64_t last = 0;
		for (uint32_t i = 0; i < seg[k].nroots; ++i)
			last = seg[k].root[i] > last ? seg[k].root[i] : last;
		for (;;) {
			for (uint32_t i = 0; i < seg[k].nroots; ++i)
				if (p == seg[k].root[i]) {
					seg[k].count = n + seg[k].hops[i];
					return true;
				}
			if (p > last || !readable(P, p))
				return false;
			p = hop(p, header_word(frame, p));
			++n;
		}
	}
	// the last segment: to the end of the frame, or until the index is full
	if (p < seg_begin(P, k))
		return false;
	while (readable(P, p) && n <= P.nsb) {
		p = hop(p, header_word(frame, p));
		++n;
	}
	seg[k].nroots = 1;
	seg[k].root[0] = seg[k - 1].exit;
	seg[k].exit = p;
	seg[k].hops[0] = (uint32_t)n;
	seg[k].state = SEG_OK;
	seg[k].count = n;
	return true;
}

// ---- phase C ----------------------------------------------------------------------------------------------
// one lane: the positions of segment k go to off[base ...]; the last segment adds what the serial walk leaves behind the
// chain (stenos.cpp:1126-1127: a chain that ends early is a truncated frame).  Returns the status bits to raise.
WALK_HD uint32_t write_segment(const Plan& P, const uint8_t* frame, uint32_t k, const Segment* seg, uint64_t base, uint64_t* off, uint32_t truncated_bit)
{
	uint64_t p = k ? seg[k - 1].exit : P.first;
	const uint64_t n = seg[k].count;
	for (uint64_t i = 0; i < n && base + i <= P.nsb; ++i) {
		off[base + i] = p;
		p = hop(p, header_word(frame, p));
	}
	if (k + 1 < P.nseg)
		return 0;
	const uint64_t total = base + n; // readable positions of the whole chain (counted up to nsb + 1)
	if (total < P.nsb) {
		for (uint64_t s = total; s <= P.nsb; ++s)
			off[s] = P.size;
		return truncated_bit;
	}
	if (total == P.nsb) {
		off[P.nsb] = p;
		return p > P.size ? truncated_bit : 0;
	}
	return 0;
}

} // namespace walk
