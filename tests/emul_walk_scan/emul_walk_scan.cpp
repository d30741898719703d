// Phase A of the parallel header walk as walk_speculate runs it (csrc/walk.h: scan_lane, scan_deferred -- loads of several steps
// at once, a filter on two bytes, the candidates' exact test put off to a list) replayed lane by lane against scan_window16 on the same
// window: the same set of roots and the same count (so the same "more than 64: the segment is given up").
//
// A stand-alone program: every frame lives in a buffer of exactly `size` bytes from malloc, so the build with
// -fsanitize=address,undefined sees any read outside [0, size).  usage: emul_walk_scan [frame_file first sb_bytes]...
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../stenos_amd/csrc/walk.h"

using namespace walk;

namespace {

struct Rng { // xorshift64*
	uint64_t s;
	uint64_t next()
	{
		s ^= s >> 12;
		s ^= s << 25;
		s ^= s >> 27;
		return s * 0x2545F4914F6CDD1Dull;
	}
	uint64_t below(uint64_t n) { return n ? next() % n : 0; }
};

struct Add {
	uint32_t operator()(uint32_t* c) const { return (*c)++; }
};

struct Counts {
	uint64_t windows = 0, roots = 0, gave_up = 0, list_full = 0, with_groups = 0, bytewise = 0, target_is_size = 0, at_size_minus_4 = 0, hop_is_window = 0;
} seen;

Plan plan_of(uint64_t first, uint64_t size, uint32_t sb_bytes, uint64_t seg_len)
{
	Plan P;
	P.first = first;
	P.size = size;
	P.nsb = 1u << 20;
	P.sb_bytes = sb_bytes;
	P.window = sb_bytes + 4;
	P.seg_len = seg_len; // a multiple of 16, as make_plan leaves it
	P.nseg = 1u << 20;
	return P;
}

// scan_window16 over the window, as walk_speculate called it before (and tests/emul still does)
uint32_t scan_old(const Plan& P, const uint8_t* frame, uint32_t k, uint64_t* roots)
{
	uint32_t n = 0;
	const uint64_t begin = seg_begin(P, k), wend = begin + P.window;
	for (uint64_t base = begin; base < wend; base += 16)
		scan_window16(P, frame, k, base, roots, &n, Add());
	return n;
}
// the workgroup of walk_speculate: SCAN_THREADS lanes in turn (the order of the lanes decides who finds the list full, nothing else)
uint32_t scan_new(const Plan& P, const uint8_t* frame, uint32_t k, uint64_t* roots, bool backwards, uint32_t* ndef_out)
{
	static uint32_t list[DEFER_CAP];
	uint32_t n = 0, ndef = 0;
	for (uint32_t i = 0; i < SCAN_THREADS; ++i)
		scan_lane(P, frame, k, backwards ? SCAN_THREADS - 1 - i : i, roots, &n, list, &ndef, Add());
	const uint32_t listed = ndef < DEFER_CAP ? ndef : DEFER_CAP;
	for (uint32_t i = 0; i < listed; ++i)
		scan_deferred(P, frame, k, list, backwards ? listed - 1 - i : i, roots, &n, Add());
	*ndef_out = ndef;
	return n;
}

int failures = 0;
void compare(const Plan& P, const uint8_t* frame, uint32_t k, const char* what)
{
	uint64_t a[LANES], b[LANES];
	uint32_t ndef = 0;
	const uint32_t na = scan_old(P, frame, k, a);
	const uint32_t nb = scan_new(P, frame, k, b, (seen.windows & 1) != 0, &ndef);
	const uint64_t begin = seg_begin(P, k);
	++seen.windows;
	seen.gave_up += na > LANES;
	seen.list_full += ndef > DEFER_CAP;
	seen.with_groups += scan_groups(P, k) > 0;
	seen.bytewise += begin + P.window + 16 > P.size;
	bool same = na == nb;
	if (same && na <= LANES) {
		std::sort(a, a + na);
		std::sort(b, b + nb);
		same = std::equal(a, a + na, b);
		seen.roots += na;
		for (uint32_t i = 0; i < na; ++i) {
			const uint64_t q = hop(a[i], header_word(frame, a[i]));
			seen.target_is_size += q == P.size;
			seen.at_size_minus_4 += a[i] + 4 == P.size;
			seen.hop_is_window += q == begin + P.window;
		}
	}
	if (!same && failures++ < 10)
		fprintf(stderr, "MISMATCH %s: first %llu size %llu sb %u seg_len %llu k %u: scan_window16 %u roots, scan_lane %u\n", what, (unsigned long long)P.first,
			(unsigned long long)P.size, P.sb_bytes, (unsigned long long)P.seg_len, k, na, nb);
}

void put_header(uint8_t* frame, uint64_t size, uint64_t p, uint32_t code, uint64_t csize)
{
	if (p + 4 > size || csize > 0xFFFFFFu)
		return;
	frame[p] = (uint8_t)code;
	frame[p + 1] = (uint8_t)csize;
	frame[p + 2] = (uint8_t)(csize >> 8);
	frame[p + 3] = (uint8_t)(csize >> 16);
}

enum Fill { UNIFORM, DENSE, SPARSE };
void fill(Rng& r, uint8_t* p, uint64_t n, Fill f)
{
	for (uint64_t i = 0; i < n; ++i) {
		const uint64_t x = r.next();
		if (f == UNIFORM)
			p[i] = (uint8_t)(x >> 32);
		else if (f == DENSE) // mostly 0..8: look-alikes everywhere, whose sizes have small top bytes
			p[i] = (x & 15) == 0 ? (uint8_t)(x >> 32) : (uint8_t)((x >> 8) % 3 == 0 ? 0 : (x >> 16) % 9);
		else // mostly zeros with some look-alike bytes
			p[i] = (x & 7) ? 0 : (uint8_t)((x >> 16) % 9);
	}
}
// headers that point at, just in front of and just behind the window's end and the frame's end, with and without a header there
void plant(Rng& r, uint8_t* frame, const Plan& P, uint32_t k)
{
	const uint64_t begin = seg_begin(P, k), wend = begin + P.window;
	const int n = (int)r.below(12);
	for (int i = 0; i < n; ++i) {
		const uint64_t p = begin + r.below(P.window);
		const uint64_t targets[] = {wend, wend - 1, wend + 1, P.size, P.size - 1, P.size + 1, P.size >= 4 ? P.size - 4 : 0, wend + r.below(P.sb_bytes), p + 4 + P.sb_bytes, p + 4};
		const uint64_t q = targets[r.below(sizeof targets / sizeof *targets)];
		if (q < p + 4)
			continue;
		put_header(frame, P.size, p, 1 + (uint32_t)r.below(8), q - p - 4);
		if (r.below(4)) // where it points: mostly something plausible
			put_header(frame, P.size, q, 1 + (uint32_t)r.below(7), r.below(3) ? r.below((uint64_t)P.sb_bytes + 1) : P.sb_bytes + r.below(3));
	}
}

struct Shape {
	uint32_t sb_bytes;
	uint64_t first;
};
// top size byte 2 (the superblock of 32-bit elements), top byte 0, an odd size from a 12-byte frame header, top byte 1
const Shape SHAPES[] = {{131072, 8}, {20480, 8}, {24573, 12}, {69632, 12}};

void synthetic(Rng& r, Fill f, const Shape& s, int windows, const char* what)
{
	for (int i = 0; i < windows; ++i) {
		const uint64_t seg_len = 16 * (1 + r.below(8));
		const uint32_t k = 1 + (uint32_t)r.below(3);
		const uint64_t begin = s.first + k * seg_len, window = (uint64_t)s.sb_bytes + 4;
		// the frame ends: far behind the window (the targets are readable), around its end, inside it
		uint64_t size;
		const uint64_t ending = r.below(5);
		switch (ending) {
		case 0: size = begin + window + s.sb_bytes + 8 + r.below(64); break;
		case 4: size = begin + window + r.below(4); break; // the frame's last header is the window's last position or next to it
		case 1: size = begin + window + r.below(4200); break;
		case 2: size = begin + window - r.below(window < 30 ? window : 30); break;
		default: size = begin + 1 + r.below(window); break;
		}
		uint8_t* frame = (uint8_t*)malloc(size);
		fill(r, frame, size, f);
		const Plan P = plan_of(s.first, size, s.sb_bytes, seg_len);
		if (r.below(4))
			plant(r, frame, P, k);
		if (ending == 4)
			put_header(frame, size, size - 4, 1 + (uint32_t)r.below(6), 0);
		compare(P, frame, k, what);
		free(frame);
	}
}
// windows that begin in the last 0..40 bytes of a frame: the byte-wise loads, a header at size - 4, targets equal to size
void tails(Rng& r, const Shape& s, int rounds)
{
	for (int i = 0; i < rounds; ++i)
		for (uint64_t d = 0; d <= 40; ++d) {
			const uint64_t seg_len = 16 * (1 + r.below(8));
			const uint32_t k = 1 + (uint32_t)r.below(2);
			const uint64_t size = s.first + k * seg_len + d;
			uint8_t* frame = (uint8_t*)malloc(size);
			fill(r, frame, size, (Fill)(i % 3));
			const Plan P = plan_of(s.first, size, s.sb_bytes, seg_len);
			const uint64_t begin = seg_begin(P, k);
			if (i % 4 != 3)
				for (int j = 0; j < 3; ++j) {
					const uint64_t p = begin + r.below(d + 1);
					put_header(frame, size, p, 1 + (uint32_t)r.below(7), p + 4 <= size ? size - p - 4 + (r.below(4) ? 0 : r.below(3)) : 0);
				}
			if (i % 2)
				put_header(frame, size, size - 4, 1 + (uint32_t)r.below(6), r.below(3) ? 0 : r.below(5));
			compare(P, frame, k, "tail");
			free(frame);
		}
}
// windows cut from a real frame, with its own superblock size and with a small one (so that whole groups of steps fit)
void golden(Rng& r, const char* path, uint64_t first, uint32_t sb_bytes, int windows)
{
	FILE* f = fopen(path, "rb");
	if (!f) {
		fprintf(stderr, "cannot read %s\n", path);
		++failures;
		return;
	}
	std::vector<uint8_t> bytes;
	uint8_t buf[65536];
	for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;)
		bytes.insert(bytes.end(), buf, buf + n);
	fclose(f);
	const uint64_t size = bytes.size();
	if (size < first + 64)
		return;
	uint8_t* frame = (uint8_t*)malloc(size);
	memcpy(frame, bytes.data(), size);
	const uint32_t sbs[] = {sb_bytes, 20480, 16 * 1024 + 256};
	for (int i = 0; i < windows; ++i) {
		const uint32_t sb = sbs[r.below(3)];
		const uint64_t seg_len = 16 * (1 + r.below(64));
		const uint64_t kmax = (size - first) / seg_len;
		const uint32_t k = 1 + (uint32_t)r.below(kmax ? kmax : 1);
		// the whole frame, or the frame cut somewhere behind the window's begin
		const uint64_t begin = first + k * seg_len;
		const uint64_t cut = r.below(3) || begin >= size ? size : begin + 1 + r.below(size - begin);
		uint8_t* exact = frame;
		if (cut != size) {
			exact = (uint8_t*)malloc(cut);
			memcpy(exact, frame, cut);
		}
		compare(plan_of(first, cut, sb, seg_len), exact, k, path);
		if (exact != frame)
			free(exact);
	}
	free(frame);
}

// for every code byte, every top size byte and these superblock sizes: what plausible() accepts passes the filter
uint64_t filter_is_a_superset()
{
	const uint32_t sizes[] = {131072, 20480, 24573, 69632, 0xFFFFFFu, 0xFF0000u, 0x7F0000u, 0x7FFFFFu, 0x800000u, 0x80FFFFu, 0x1000000u, 256, 0};
	uint64_t passed = 0;
	for (uint32_t sb : sizes) {
		Plan P = plan_of(8, 1 << 20, sb, 16);
		const ScanFilter F = scan_filter(P);
		const uint32_t top = sb >> 16;
		for (uint32_t code = 0; code < 256; ++code)
			for (uint32_t t = 0; t < 256; ++t)
				for (uint32_t j = 0; j < 16; ++j) { // the position inside the 16; its neighbours hold what would pass alone
					uint8_t b[20];
					memset(b, (code + t + j) & 1 ? 0x01 : 0xFF, sizeof b);
					b[j] = (uint8_t)code;
					b[j + 3] = (uint8_t)t;
					uint32_t w[5];
					memcpy(w, b, sizeof b);
					const bool pass = (scan_candidates16(F, w) >> j) & 1u;
					const bool want = code >= 1 && code <= 8 && t <= (top > 255 ? 255 : top); // what the filter promises
					// the largest and the smallest size with this top byte
					const bool plaus = plausible(P, code | 0xFFFF00u | (t << 24)) || plausible(P, code | (t << 24));
					if (pass != want || (plaus && !pass)) {
						if (failures++ < 10)
							fprintf(stderr, "FILTER sb %#x code %u top %u position %u: passes %d, promised %d, plausible %d\n", sb, code, t, j, pass, want, plaus);
					}
					passed += pass;
				}
	}
	return passed;
}

} // namespace

int main(int argc, char** argv)
{
	Rng r{0x9E3779B97F4A7C15ull};
	const uint64_t passed = filter_is_a_superset();
	for (const Shape& s : SHAPES) {
		const int n = s.sb_bytes > 65536 ? 400 : 1500;
		synthetic(r, UNIFORM, s, n, "uniform");
		synthetic(r, DENSE, s, n, "dense");
		synthetic(r, SPARSE, s, n / 2, "sparse");
		tails(r, s, 24);
	}
	for (int i = 1; i + 2 < argc; i += 3)
		golden(r, argv[i], strtoull(argv[i + 1], nullptr, 10), (uint32_t)strtoul(argv[i + 2], nullptr, 10), 60);
	printf("windows %llu roots %llu gave_up %llu list_full %llu with_groups %llu bytewise %llu target_is_size %llu at_size_minus_4 %llu hop_is_window %llu filter_passed %llu "
	       "scan_steps %u failures %d\n",
	       (unsigned long long)seen.windows, (unsigned long long)seen.roots, (unsigned long long)seen.gave_up, (unsigned long long)seen.list_full,
	       (unsigned long long)seen.with_groups, (unsigned long long)seen.bytewise, (unsigned long long)seen.target_is_size, (unsigned long long)seen.at_size_minus_4,
	       (unsigned long long)seen.hop_is_window, (unsigned long long)passed, SCAN_STEPS, failures);
	return failures ? 1 : 0;
}
