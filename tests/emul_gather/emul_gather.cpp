// tests/emul_gather/emul_gather.cpp -- TEST INFRASTRUCTURE.  The cutting function, decode_superblock_pieces and the chunk rule
// of the gather kernels, decode_gather_chunk (stenos_amd/csrc/gather_codec.h), compiled for the host with WV_HOST_EMULATION,
// as tests/emul_ranges compiles decode_superblock_window: 64 lanes in lockstep, LDS as a plain buffer.  The shipped library
// never contains or calls this.
#define WV_HOST_EMULATION 1
#include "../../stenos_amd/csrc/gather_codec.h"

#include <stdlib.h>
#include <string.h>

using namespace codec;

static int g_lds_fill = 0xCD; // what a wave finds in its LDS (results must not depend on it)
enum { GUARD = 64, GUARD_BYTE = 0xA5 };

namespace {
// One read arena: the piece table (16-byte entries), then the payload, shifted off its 16-byte boundary by `misalign`.
// One write arena: a guard, then per piece its slot and a guard, then (flag_word) the superblock's flag word and a guard; the
// arena itself is shifted by dst_misalign.
struct Arenas {
	uint8_t *lds = nullptr, *rd = nullptr, *wr = nullptr;
	uint8_t *tab = nullptr, *from = nullptr, *to = nullptr, *flag = nullptr;
	size_t rd_bytes = 0, wr_bytes = 0;
	DecLayout L;
	bool make(const uint8_t* src, size_t csize, size_t T, const uint32_t* lo, const uint32_t* hi, size_t count, int misalign, int dst_misalign, bool flag_word = false)
	{
		L = make_dec_layout((uint32_t)T);
		const size_t tab_bytes = count * sizeof(GatherPiece);
		rd_bytes = tab_bytes + 16 + misalign + csize;
		wr_bytes = GUARD;
		for (size_t k = 0; k < count; ++k)
			wr_bytes += (hi[k] > lo[k] ? hi[k] - lo[k] : 0) + GUARD;
		wr_bytes += flag_word ? 4 + GUARD : 0;
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
		flag = flag_word ? to + at : nullptr;
		return true;
	}
	// the slots' bytes, back to back, to out, and the flag word (four guard bytes where nothing wrote it) to *flag_out; false: a
	// byte outside the slots and the flag word changed
	bool collect(const uint32_t* lo, const uint32_t* hi, size_t count, uint8_t* out, uint32_t* flag_out = nullptr) const
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
		if (flag) {
			memcpy(flag_out, p, 4);
			for (const uint8_t* e = (p += 4) + GUARD; p < e; ++p)
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
	// the chunk rule on the frame at `from`: superblock s, whose header the index puts at p
	uint32_t run_chunk(size_t size, size_t T, uint64_t total, uint64_t sb, uint64_t s, uint64_t p, size_t count)
	{
		return decode_gather_chunk<0>(lds, (uint32_t)T, from, size, total, sb, s, p, tab, (uint32_t)count, to, (uint32_t*)flag);
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

// ---- the chunk rule ----
// Superblock s of the frame src[0, size) (an array of `total` bytes in superblocks of sb) with the index entry p and `count`
// (1..64) pieces -> out, back to back; *flag: the superblock's flag word, 0xA5A5A5A5 where it was not written.  Returns the
// DECODE_STATUS_* bits of the chunk, (size_t)-7 if a byte outside the slots and the flag word changed.
size_t emul_gather_chunk(const uint8_t* src, size_t size, size_t T, uint64_t total, uint64_t sb, uint64_t s, uint64_t p, const uint32_t* lo, const uint32_t* hi,
			 size_t count, uint8_t* out, uint32_t* flag, int misalign, int dst_misalign)
{
	Arenas b;
	if (count == 0 || count > 64 || !b.make(src, size, T, lo, hi, count, misalign, dst_misalign, true))
		return (size_t)-3;
	const uint32_t r = b.run_chunk(size, T, total, sb, s, p, count);
	return b.collect(lo, hi, count, out, flag) ? r : (size_t)-7;
}

#ifdef WV_AUDIT
// The same with every memory access of the kernel source checked (wavevec_host.h, "the access audit"):
//   LDS           the wave's make_dec_layout(T).total bytes, nothing behind them;
//   global reads  the read arena: from the piece table to the end of the 16-byte hull of the payload;
//   global writes the write arena (the guards inside it are checked byte by byte afterwards).
// report: as emul_audit_window_decompress (tests/emul_ranges).
static const char* g_audit_first_name = "";
const char* emul_audit_first_name(void) { return g_audit_first_name; }
static void audit_on(const Arenas& b, size_t read_bytes)
{
	wv::AuditState& A = wv::audit_state();
	memset(&A, 0, sizeof A);
	A.lo[wv::WV_AUDIT_LDS] = b.lds;
	A.hi[wv::WV_AUDIT_LDS] = b.lds + b.L.total;
	A.lo[wv::WV_AUDIT_GREAD] = b.rd;
	A.hi[wv::WV_AUDIT_GREAD] = (const uint8_t*)(((uintptr_t)b.from + read_bytes + 15) & ~(uintptr_t)15);
	A.lo[wv::WV_AUDIT_GWRITE] = b.to;
	A.hi[wv::WV_AUDIT_GWRITE] = b.to + b.wr_bytes;
	A.on = true;
}
static void audit_off(uint64_t* report)
{
	wv::AuditState& A = wv::audit_state();
	A.on = false;
	report[0] = A.violations;
	report[1] = A.checked;
	report[2] = (uint64_t)A.first_kind;
	report[3] = (uint64_t)A.first_off;
	report[4] = A.first_width;
	g_audit_first_name = A.first_name ? A.first_name : "";
}
size_t emul_audit_gather_pieces(const uint8_t* src, size_t csize, size_t T, size_t dsize, const uint32_t* lo, const uint32_t* hi, size_t count, uint8_t* out,
				int misalign, int dst_misalign, uint64_t* report)
{
	Arenas b;
	if (count == 0 || count > 64 || !b.make(src, csize, T, lo, hi, count, misalign, dst_misalign))
		return (size_t)-3;
	audit_on(b, csize);
	const uint32_t r = b.run(csize, T, dsize, count);
	audit_off(report);
	if (!b.collect(lo, hi, count, out))
		return (size_t)-7;
	return r == DEC_ERROR ? (size_t)-4 : 0;
}
// ... and the chunk rule: the global reads end with the 16-byte hull of the frame, the flag word lies in the write arena
size_t emul_audit_gather_chunk(const uint8_t* src, size_t size, size_t T, uint64_t total, uint64_t sb, uint64_t s, uint64_t p, const uint32_t* lo, const uint32_t* hi,
			       size_t count, uint8_t* out, uint32_t* flag, int misalign, int dst_misalign, uint64_t* report)
{
	Arenas b;
	if (count == 0 || count > 64 || !b.make(src, size, T, lo, hi, count, misalign, dst_misalign, true))
		return (size_t)-3;
	audit_on(b, size);
	const uint32_t r = b.run_chunk(size, T, total, sb, s, p, count);
	audit_off(report);
	return b.collect(lo, hi, count, out, flag) ? r : (size_t)-7;
}
#endif

} // extern "C"
