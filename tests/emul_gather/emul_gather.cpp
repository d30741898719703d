// tests/emul_gather/emul_gather.cpp -- TEST INFRASTRUCTURE.  The cutting function and decode_superblock_pieces
// (stenos_amd/csrc/gather_codec.h) compiled for the host with WV_HOST_EMULATION, as tests/emul_ranges compiles
// decode_superblock_window: 64 lanes in lockstep, LDS as a plain buffer.  The shipped library never contains or calls this.
#define WV_HOST_EMULATION 1
#include "../../stenos_amd/csrc/gather_codec.h"

#include <stdlib.h>
#include <string.h>

using namespace codec;

static int g_lds_fill = 0xCD; // what a wave finds in its LDS (results must not depend on it)
enum { GUARD = 64, GUARD_BYTE = 0xA5 };

namespace {
// One read arena: the piece table (16-byte entries), then the payload, shifted off its 16-byte boundary by `misalign`.
// One write arena: a guard, then per piece its slot and a guard; the arena itself is shifted by dst_misalign.
struct Arenas {
	uint8_t *lds = nullptr, *rd = nullptr, *wr = nullptr;
	uint8_t *tab = nullptr, *from = nullptr, *to = nullptr;
	size_t rd_bytes = 0, wr_bytes = 0;
	DecLayout L;
	bool make(const uint8_t* src, size_t csize, size_t T, const uint32_t* lo, const uint32_t* hi, size_t count, int misalign, int dst_misalign)
	{
		L = make_dec_layout((uint32_t)T);
		const size_t tab_bytes = count * sizeof(GatherPiece);
		rd_bytes = tab_bytes + 16 + misalign + csize;
		wr_bytes = GUARD;
		for (size_t k = 0; k < count; ++k)
			wr_bytes += (hi[k] > lo[k] ? hi[k] - lo[k] : 0) + GUARD;
		// (larger than the regions by a margin nothing relies on)
		if (posix_memalign((void**)&lds, 64, L.total + 256) || posix_memalign((void**)&rd, 64, rd_bytes + 128) || posix_memalign((void**)&wr, 64, wr_bytes + 128))
			return false;
		memset(lds, g_lds_fill, L.total + 256); // LDS is not zero-initialised on the device either
		memset(rd, 0xEE, rd_bytes + 128);
		memset(wr, GUARD_BYTE, wr_bytes + 128);
		tab = rd;
		from = rd + tab_bytes + 16 + misalign;
		memcpy(from, src, csize);
		to = wr + dst_misalign;
		uint64_t at = GUARD;
		for (size_t k = 0; k < count; ++k) {
			GatherPiece p;
			p.lo = lo[k];
			p.hi = hi[k];
			p.dst = at;
			memcpy(tab + k * sizeof p, &p, sizeof p);
			at += (hi[k] > lo[k] ? hi[k] - lo[k] : 0) + GUARD;
		}
		return true;
	}
	// the slots' bytes, back to back, to out; false: a byte outside the slots changed
	bool collect(const uint32_t* lo, const uint32_t* hi, size_t count, uint8_t* out) const
	{
		const uint8_t* p = wr;
		for (; p < to + GUARD; ++p)
			if (*p != GUARD_BYTE)
				return false;
		for (size_t k = 0; k < count; ++k) {
			const size_t len = hi[k] > lo[k] ? hi[k] - lo[k] : 0;
			memcpy(out, p, len);
			out += len;
			p += len;
			for (const uint8_t* e = p + GUARD; p < e; ++p)
				if (*p != GUARD_BYTE)
					return false;
		}
		for (; p < wr + wr_bytes + 128; ++p)
			if (*p != GUARD_BYTE)
				return false;
		return true;
	}
	uint32_t run(size_t csize, size_t T, size_t dsize, size_t count)
	{
		const LanePieces q = load_pieces(tab, (uint32_t)count);
		return decode_superblock_pieces(lds, L, (uint32_t)T, from, (uint32_t)csize, (uint32_t)dsize, q, to);
	}
	~Arenas()
	{
		free(lds);
		free(rd);
		free(wr);
	}
};
} // namespace

extern "C" {

void emul_set_lds_fill(int byte) { g_lds_fill = byte & 255; }

// ---- the cutting function ----
uint64_t emul_gather_pieces_per_row(uint64_t row_bytes, uint64_t sb) { return gather_pieces_per_row(row_bytes, sb); }
uint64_t emul_gather_valid_rows(uint64_t total, uint64_t row_bytes) { return gather_valid_rows(total, row_bytes); }
// out: superblock, lo, hi, destination offset; returns 0 for an empty piece (out untouched)
int emul_gather_cut(uint64_t row_bytes, uint64_t dst_stride, uint64_t total, uint64_t sb, uint64_t row, uint64_t i, uint64_t j, uint64_t* out)
{
	GatherShape g = { row_bytes, dst_stride, total, sb };
	GatherPiece p;
	uint64_t s;
	if (!gather_cut(g, row, i, j, &s, &p))
		return 0;
	out[0] = s;
	out[1] = p.lo;
	out[2] = p.hi;
	out[3] = p.dst;
	return 1;
}

// ---- the decoder ----
// `count` (1..64) pieces [lo[k], hi[k]) of the superblock with payload src[0, csize) and dsize decoded bytes -> out, back to
// back.  Returns 0, (size_t)-4 for a stream the decoder refuses, (size_t)-7 if a byte outside the slots changed.
size_t emul_gather_pieces(const uint8_t* src, size_t csize, size_t T, size_t dsize, const uint32_t* lo, const uint32_t* hi, size_t count, uint8_t* out, int misalign,
			  int dst_misalign)
{
	Arenas b;
	if (count == 0 || count > 64 || !b.make(src, csize, T, lo, hi, count, misalign, dst_misalign))
		return (size_t)-3;
	const uint32_t r = b.run(csize, T, dsize, count);
	if (!b.collect(lo, hi, count, out))
		return (size_t)-7;
	return r == DEC_ERROR ? (size_t)-4 : 0;
}

#ifdef WV_AUDIT
// The same with every memory access of the kernel source checked (wavevec_host.h, "the access audit"):
//   LDS           the wave's make_dec_layout(T).total bytes, nothing behind them;
//   global reads  the read arena: from the piece table to the end of the 16-byte hull of the payload;
//   global writes the write arena (the guards inside it are checked byte by byte afterwards).
// report: as emul_audit_window_decompress (tests/emul_ranges).
static const char* g_audit_first_name = "";
const char* emul_audit_first_name(void) { return g_audit_first_name; }
size_t emul_audit_gather_pieces(const uint8_t* src, size_t csize, size_t T, size_t dsize, const uint32_t* lo, const uint32_t* hi, size_t count, uint8_t* out,
				int misalign, int dst_misalign, uint64_t* report)
{
	Arenas b;
	if (count == 0 || count > 64 || !b.make(src, csize, T, lo, hi, count, misalign, dst_misalign))
		return (size_t)-3;
	wv::AuditState& A = wv::audit_state();
	memset(&A, 0, sizeof A);
	A.lo[wv::WV_AUDIT_LDS] = b.lds;
	A.hi[wv::WV_AUDIT_LDS] = b.lds + b.L.total;
	A.lo[wv::WV_AUDIT_GREAD] = b.rd;
	A.hi[wv::WV_AUDIT_GREAD] = (const uint8_t*)(((uintptr_t)b.from + csize + 15) & ~(uintptr_t)15);
	A.lo[wv::WV_AUDIT_GWRITE] = b.to;
	A.hi[wv::WV_AUDIT_GWRITE] = b.to + b.wr_bytes;
	A.on = true;
	const uint32_t r = b.run(csize, T, dsize, count);
	A.on = false;
	report[0] = A.violations;
	report[1] = A.checked;
	report[2] = (uint64_t)A.first_kind;
	report[3] = (uint64_t)A.first_off;
	report[4] = A.first_width;
	g_audit_first_name = A.first_name ? A.first_name : "";
	if (!b.collect(lo, hi, count, out))
		return (size_t)-7;
	return r == DEC_ERROR ? (size_t)-4 : 0;
}
#endif

} // extern "C"
