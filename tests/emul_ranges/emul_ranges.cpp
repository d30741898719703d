// tests/emul_ranges/emul_ranges.cpp -- TEST INFRASTRUCTURE.  decode_superblock_window (stenos_amd/csrc/range_codec.h) compiled
// for the host with WV_HOST_EMULATION, as tests/emul/emul.cpp compiles decode_superblock: 64 lanes in lockstep, LDS as a plain
// buffer.  The shipped library never contains or calls this.
#define WV_HOST_EMULATION 1
#include "../../stenos_amd/csrc/range_codec.h"

#include <stdlib.h>
#include <string.h>

using namespace codec;

static int g_lds_fill = 0xCD; // what a wave finds in its LDS (results must not depend on it)
enum { GUARD = 64, GUARD_BYTE = 0xA5 };

namespace {
struct Buffers {
	uint8_t *lds = nullptr, *in = nullptr, *out = nullptr;
	uint8_t *from = nullptr, *to = nullptr;
	DecLayout L;
	bool make(const uint8_t* src, size_t csize, size_t T, size_t n, int misalign, int dst_misalign)
	{
		L = make_dec_layout((uint32_t)T);
		// (larger than the regions by a margin nothing relies on)
		if (posix_memalign((void**)&lds, 64, L.total + 256) || posix_memalign((void**)&in, 64, csize + 128) || posix_memalign((void**)&out, 64, n + 2 * GUARD + 128))
			return false;
		memset(lds, g_lds_fill, L.total + 256); // LDS is not zero-initialised on the device either
		memset(in, 0xEE, csize + 128);
		memset(out, GUARD_BYTE, n + 2 * GUARD + 128);
		from = in + 16 + misalign;
		memcpy(from, src, csize);
		to = out + GUARD + dst_misalign;
		return true;
	}
	bool guards_intact(size_t n) const
	{
		for (uint8_t* p = out; p < out + n + 2 * GUARD + 128; ++p)
			if ((p < to || p >= to + n) && *p != GUARD_BYTE)
				return false;
		return true;
	}
	~Buffers()
	{
		free(lds);
		free(in);
		free(out);
	}
};
} // namespace

extern "C" {

void emul_set_lds_fill(int byte) { g_lds_fill = byte & 255; }

// Bytes [lo, hi) of the superblock with payload src[0, csize) and dsize decoded bytes -> dst[0, hi - lo).  misalign shifts the
// source off its 16-byte boundary, dst_misalign the destination the decoder writes to; that one has 64 guard bytes on both sides.
// Returns hi - lo, (size_t)-4 for a stream the decoder refuses, (size_t)-7 if a guard byte changed.
size_t emul_window_decompress(const uint8_t* src, size_t csize, size_t T, size_t dsize, size_t lo, size_t hi, uint8_t* dst, int misalign, int dst_misalign)
{
	Buffers b;
	if (!b.make(src, csize, T, hi - lo, misalign, dst_misalign))
		return (size_t)-3;
	const uint32_t r = decode_superblock_window(b.lds, b.L, (uint32_t)T, b.from, (uint32_t)csize, (uint32_t)dsize, (uint32_t)lo, (uint32_t)hi, b.to);
	if (!b.guards_intact(hi - lo))
		return (size_t)-7;
	if (r == DEC_ERROR)
		return (size_t)-4;
	memcpy(dst, b.to, hi - lo);
	return r;
}

#ifdef WV_AUDIT
// The same with every memory access of the kernel source checked (wavevec_host.h, "the access audit"):
//   LDS           the wave's make_dec_layout(T).total bytes, nothing behind them;
//   global reads  the 16-byte aligned hull of [src, src + csize);
//   global writes [dst, dst + hi - lo) exactly.
// report: as emul_audit_block_decompress (tests/emul/emul.cpp).
static const char* g_audit_first_name = "";
const char* emul_audit_first_name(void) { return g_audit_first_name; }
size_t emul_audit_window_decompress(const uint8_t* src, size_t csize, size_t T, size_t dsize, size_t lo, size_t hi, uint8_t* dst, int misalign, int dst_misalign,
				    uint64_t* report)
{
	Buffers b;
	if (!b.make(src, csize, T, hi - lo, misalign, dst_misalign))
		return (size_t)-3;
	wv::AuditState& A = wv::audit_state();
	memset(&A, 0, sizeof A);
	A.lo[wv::WV_AUDIT_LDS] = b.lds;
	A.hi[wv::WV_AUDIT_LDS] = b.lds + b.L.total;
	A.lo[wv::WV_AUDIT_GREAD] = (const uint8_t*)((uintptr_t)b.from & ~(uintptr_t)15);
	A.hi[wv::WV_AUDIT_GREAD] = (const uint8_t*)(((uintptr_t)b.from + csize + 15) & ~(uintptr_t)15);
	A.lo[wv::WV_AUDIT_GWRITE] = b.to;
	A.hi[wv::WV_AUDIT_GWRITE] = b.to + (hi - lo);
	A.on = true;
	const uint32_t r = decode_superblock_window(b.lds, b.L, (uint32_t)T, b.from, (uint32_t)csize, (uint32_t)dsize, (uint32_t)lo, (uint32_t)hi, b.to);
	A.on = false;
	report[0] = A.violations;
	report[1] = A.checked;
	report[2] = (uint64_t)A.first_kind;
	report[3] = (uint64_t)A.first_off;
	report[4] = A.first_width;
	g_audit_first_name = A.first_name ? A.first_name : "";
	if (!b.guards_intact(hi - lo))
		return (size_t)-7;
	if (r == DEC_ERROR)
		return (size_t)-4;
	memcpy(dst, b.to, hi - lo);
	return r;
}
#endif

} // extern "C"
