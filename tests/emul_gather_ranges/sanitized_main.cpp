// tests/emul_gather_ranges/sanitized_main.cpp -- TEST INFRASTRUCTURE.  A stand-alone program around emul_gather_ranges.cpp for
// a build with -fsanitize=address,undefined (make sanitized): the scan passes at width 4 and 64 against a serial sum, and the
// whole call on a frame of stored superblocks (code 6: built here without an encoder) against memcpy, with valid sets, an
// invalid range and a dst_size one byte short.  Exit status 0: everything agreed and the sanitizers saw nothing.
#include "emul_gather_ranges.cpp"

#include <stdio.h>

static int failures = 0;
#define CHECK(cond)                                                        \
	do {                                                               \
		if (!(cond)) {                                             \
			fprintf(stderr, "line %d: %s\n", __LINE__, #cond); \
			++failures;                                        \
		}                                                          \
	} while (0)

static uint64_t rnd(uint64_t& s)
{
	s = s * 6364136223846793005ull + 1442695040888963407ull;
	return s >> 33;
}

int main()
{
	uint64_t seed = 7;
	// ---- the scan passes ----
	for (uint32_t width : { 4u, 64u })
		for (uint64_t n : { 0ull, 1ull, 4ull, 5ull, 16ull, 17ull, 64ull, 65ull, 1000ull }) {
			const uint64_t total = (1ull << 40) + 12345, sb = 131072;
			std::vector<uint64_t> off(n + 1), len(n + 1), D(n + 1);
			std::vector<uint32_t> P(n + 1);
			uint64_t sum = 0;
			for (uint64_t i = 0; i < n; ++i) {
				off[i] = rnd(seed) % (total - (1ull << 31));
				len[i] = i % 7 ? rnd(seed) % (1ull << 31) : 0;
			}
			uint64_t words[3];
			CHECK(emul_ranges_offsets(total, sb, ~0ull, n, off.data(), len.data(), width, D.data(), P.data(), words) == 0);
			for (uint64_t i = 0; i < n; ++i) {
				CHECK(D[i] == sum);
				sum += len[i];
			}
			CHECK(D[n] == sum && words[2] == sum && words[0] == 0);
			if (sum) {
				CHECK(emul_ranges_offsets(total, sb, sum - 1, n, off.data(), len.data(), width, D.data(), P.data(), words) == 0);
				CHECK(words[0] == RANGES_ST_DST_OVERFLOW);
			}
		}
	// ---- the call, on three stored superblocks and a partial one ----
	const uint64_t T = 4, sb = 1024, total = 3 * sb + 300, nsb = 4;
	std::vector<uint8_t> array(total), frame;
	for (uint8_t& b : array)
		b = (uint8_t)rnd(seed);
	frame.push_back(255);
	for (int i = 0; i < 7; ++i)
		frame.push_back((uint8_t)(total >> (8 * i)));
	for (int i = 0; i < 4; ++i)
		frame.push_back((uint8_t)(sb >> (8 * i)));
	uint64_t index[5];
	for (uint64_t s = 0; s < nsb; ++s) {
		const uint64_t d = total - s * sb < sb ? total - s * sb : sb;
		index[s] = frame.size();
		frame.push_back(6);
		for (int i = 0; i < 3; ++i)
			frame.push_back((uint8_t)(d >> (8 * i)));
		frame.insert(frame.end(), array.begin() + s * sb, array.begin() + s * sb + d);
	}
	index[nsb] = frame.size();
	const size_t size = frame.size();
	frame.resize(size + 64); // (the 16-byte hull of the last payload)
	for (int round = 0; round < 20; ++round) {
		const uint64_t n = round < 3 ? 65 + round : 1 + rnd(seed) % 40;
		std::vector<uint64_t> off(n), len(n), D(n + 1);
		std::vector<uint8_t> want;
		for (uint64_t i = 0; i < n; ++i) {
			len[i] = round < 3 ? 7 : rnd(seed) % (round % 2 ? 40 : 2500);
			off[i] = round < 3 ? sb + rnd(seed) % (sb - 7) : rnd(seed) % (total - len[i] + 1);
		}
		if (round == 5) {
			off[0] = 0;
			len[0] = total; // the whole array
		}
		for (uint64_t i = 0; i < n; ++i)
			want.insert(want.end(), array.begin() + off[i], array.begin() + off[i] + len[i]);
		std::vector<uint8_t> out(want.size() + 16);
		uint32_t flags[4];
		uint64_t words[3];
		size_t r = emul_gather_ranges(frame.data(), size, T, total, sb, nsb, index, n, off.data(), len.data(), want.size(), want.size(), round % 2 ? 4 : 64, out.data(), D.data(),
					      flags, words, round % 16, (round * 5) % 16);
		CHECK(r == 0 && words[2] == want.size());
		CHECK(memcmp(out.data(), want.data(), want.size()) == 0);
		if (want.size()) { // one byte short: the bit, and nothing written
			r = emul_gather_ranges(frame.data(), size, T, total, sb, nsb, index, n, off.data(), len.data(), want.size() - 1, want.size(), 4, out.data(), D.data(), flags, words, 0, 3);
			CHECK(r == RANGES_ST_DST_OVERFLOW);
			for (size_t i = 0; i < want.size(); ++i)
				if (out[i] != GUARD_BYTE) {
					CHECK(!"written after an overflow");
					break;
				}
		}
		// an invalid range in the middle
		const uint64_t keep_off = off[n / 2], keep_len = len[n / 2];
		off[n / 2] = ~0ull;
		len[n / 2] = 2;
		r = emul_gather_ranges(frame.data(), size, T, total, sb, nsb, index, n, off.data(), len.data(), want.size(), want.size(), 4, out.data(), D.data(), flags, words, 1, 0);
		CHECK(r == RANGES_ST_BAD_RANGE);
		for (size_t i = 0; i < want.size(); ++i)
			if (out[i] != GUARD_BYTE) {
				CHECK(!"written after an invalid range");
				break;
			}
		off[n / 2] = keep_off;
		len[n / 2] = keep_len;
	}
	printf("%s\n", failures ? "FAILED" : "ok");
	return failures ? 1 : 0;
}
