// tests/emul_gather_ranges/emul_gather_ranges.cpp -- TEST INFRASTRUCTURE.  The rules of stenos_hip_gather_ranges
// (stenos_amd/csrc/gather_ranges_codec.h: measuring, cutting, the three scan passes as block steps, the piece slots) compiled for
// the host, the block steps at a width the caller chooses (4: every level boundary is crossed by a handful of ranges), and the
// whole call in the emulation: measure -> scan -> count -> gather_scan's rule -> fill -> decode_gather_chunk (gather_codec.h,
// WV_HOST_EMULATION: 64 lanes in lockstep, LDS as a plain buffer).  The shipped library never contains or calls this.
#define WV_HOST_EMULATION 1
#define RANGES_HOST_STEPS 1
#include "../../stenos_amd/csrc/gather_codec.h"
#include "../../stenos_amd/csrc/gather_ranges_codec.h"

#include <stdlib.h>
#include <string.h>

#include <vector>

using namespace codec;

static int g_lds_fill = 0xCD; // what a wave finds in its LDS (results must not depend on it)
enum { GUARD = 64, GUARD_BYTE = 0xA5 };

namespace {

// a step of a block of W threads: every thread runs it; the end of the loop is the barrier
struct LoopEach {
	uint32_t W;
	template <class F>
	void operator()(F f) const
	{
		for (uint32_t k = 0; k < W; ++k)
			f(k);
	}
};

// the three passes of gather_ranges_kernels.hip (ranges_sums, ranges_scan, ranges_apply) at block width W
template <uint32_t W>
void offsets_passes(const RangesArgs& a)
{
	RangesTile<W> t;
	LoopEach each = { W };
	for (uint32_t b = 0; b < a.nblocks; ++b) {
		memset(&t, 0xEE, sizeof t); // (shared memory is not zero on the device either)
		ranges_block_sums<W>(a, b, t, each);
	}
	memset(&t, 0xEE, sizeof t);
	ranges_scan_sums<W>(a, t, each);
	for (uint32_t b = 0; b < a.nblocks; ++b) {
		memset(&t, 0xEE, sizeof t);
		ranges_block_apply<W>(a, b, t, each);
	}
}

// the tables of one call but the piece table, which the read arena holds; width: 4 or 64
struct Tables {
	RangesWords words = { 0, 0, 0 };
	std::vector<uint64_t> D, block_bytes;
	std::vector<uint32_t> pstart, block_pieces, count, ppre, wpre;
	RangesArgs a;
	bool make(uint64_t total, uint64_t sb, uint64_t dst_size, uint64_t n, const uint64_t* offsets, const uint64_t* lengths, uint32_t width, uint64_t nsb)
	{
		if (width != 4 && width != 64)
			return false;
		a = RangesArgs();
		a.offsets = offsets;
		a.lengths = lengths;
		a.n = n;
		a.total = total;
		a.sb = sb;
		a.dst_size = dst_size;
		a.pmax = ranges_piece_bound(n, dst_size, sb);
		a.nblocks = (uint32_t)((n + width - 1) / width);
		D.assign(n + 1, 0xEEEEEEEEEEEEEEEEull);
		pstart.assign(n + 1, 0xEEEEEEEEu);
		block_bytes.assign(a.nblocks + 1, 0xEEEEEEEEEEEEEEEEull);
		block_pieces.assign(a.nblocks + 1, 0xEEEEEEEEu);
		count.assign(nsb + 1, 0);
		ppre.assign(nsb + 1, 0xEEEEEEEEu);
		wpre.assign(nsb + 1, 0xEEEEEEEEu);
		a.words = &words;
		a.D = D.data();
		a.pstart = pstart.data();
		a.block_bytes = block_bytes.data();
		a.block_pieces = block_pieces.data();
		a.count = count.data();
		a.ppre = ppre.data();
		a.pieces = nullptr;
		return true;
	}
	void offsets_of(uint32_t width) { width == 4 ? offsets_passes<4>(a) : offsets_passes<64>(a); }
	// gather_scan's rule (gather_kernels.hip): exclusive sums of count and of ceil(count / 64), count := 0
	void scan_counts(uint64_t nsb)
	{
		uint32_t p = 0, w = 0;
		for (uint64_t s = 0; s < nsb; ++s) {
			const uint32_t c = count[s];
			ppre[s] = p;
			wpre[s] = w;
			count[s] = 0;
			p += c;
			w += (c + 63u) >> 6;
		}
		ppre[nsb] = p;
		wpre[nsb] = w;
	}
};

// One read arena: the piece table (pmax entries of 16 bytes), then the frame, shifted off its 16-byte boundary by `misalign`.
// One write arena, shifted by dst_misalign: a guard, the packed output (out_bytes), a guard, the nsb flag words, a guard.
struct Arenas {
	uint8_t *lds = nullptr, *rd = nullptr, *wr = nullptr;
	uint8_t *tab = nullptr, *from = nullptr, *to = nullptr;
	size_t rd_bytes = 0, wr_bytes = 0, out_bytes = 0, nsb = 0;
	DecLayout L;
	bool make(const uint8_t* frame, size_t size, size_t T, uint64_t pmax, size_t out, size_t superblocks, int misalign, int dst_misalign)
	{
		L = make_dec_layout((uint32_t)T);
		out_bytes = out;
		nsb = superblocks;
		const size_t tab_bytes = pmax * sizeof(GatherPiece);
		rd_bytes = tab_bytes + 16 + misalign + size;
		wr_bytes = GUARD + out_bytes + GUARD + 4 * nsb + GUARD;
		if (posix_memalign((void**)&lds, 64, L.total + 256) || posix_memalign((void**)&rd, 64, rd_bytes + 128) || posix_memalign((void**)&wr, 64, wr_bytes + 128))
			return false;
		memset(lds, g_lds_fill, L.total + 256);
		memset(rd, 0xEE, rd_bytes + 128);
		memset(wr, GUARD_BYTE, wr_bytes + 128);
		tab = rd;
		from = rd + tab_bytes + 16 + misalign;
		memcpy(from, frame, size);
		to = wr + dst_misalign;
		memset(flags(), 0, 4 * nsb); // (the call's memset)
		return true;
	}
	uint8_t* dst() const { return to + GUARD; }
	uint8_t* flags() const { return to + GUARD + out_bytes + GUARD; }
	// the packed output to out, the flag words to flags_out; false: a byte outside them changed
	bool collect(uint8_t* out, uint32_t* flags_out) const
	{
		auto guard = [](const uint8_t* p, const uint8_t* e) {
			for (; p < e; ++p)
				if (*p != GUARD_BYTE)
					return false;
			return true;
		};
		memcpy(out, dst(), out_bytes);
		memcpy(flags_out, flags(), 4 * nsb);
		return guard(wr, dst()) && guard(dst() + out_bytes, flags()) && guard(flags() + 4 * nsb, wr + wr_bytes + 128);
	}
	~Arenas()
	{
		free(lds);
		free(rd);
		free(wr);
	}
};

// The call: D and pstart, the pieces counted, ordered by superblock and decoded chunk by chunk as gather_decode's wavefronts do.
// Returns the status word.
uint32_t run_call(Tables& t, Arenas& b, size_t size, size_t T, uint64_t total, uint64_t sb, uint64_t nsb, const uint64_t* index, uint32_t width)
{
	t.a.pieces = (GatherPiece*)b.tab;
	t.offsets_of(width);
	for (uint64_t s = 0; s < t.a.pmax; ++s)
		ranges_count_slot(t.a, s);
	t.scan_counts(nsb);
	for (uint64_t s = 0; s < t.a.pmax; ++s)
		ranges_fill_slot(t.a, s);
	for (uint32_t w = 0; w < t.wpre[nsb]; ++w) { // (gather_decode: wavefronts from wpre[nsb] on leave at once)
		const uint32_t s = gather_find32(t.wpre.data(), (uint32_t)nsb, w);
		const uint32_t first = t.ppre[s] + 64u * (w - t.wpre[s]), left = t.ppre[s + 1] - first;
		t.words.status |= decode_gather_chunk<0>(b.lds, (uint32_t)T, b.from, size, total, sb, s, index[s], b.tab + (size_t)first * sizeof(GatherPiece), left < 64u ? left : 64u,
							 b.dst(), (uint32_t*)b.flags() + s);
	}
	return t.words.status;
}

} // namespace

extern "C" {

void emul_set_lds_fill(int byte) { g_lds_fill = byte & 255; }

// ---- one range ----
// out: bytes, pieces; returns 1 for a valid range
int emul_ranges_measure(uint64_t total, uint64_t sb, uint64_t off, uint64_t len, uint64_t* out)
{
	uint64_t bytes;
	uint32_t pieces;
	const bool ok = ranges_measure(total, sb, off, len, &bytes, &pieces);
	out[0] = bytes;
	out[1] = pieces;
	return ok ? 1 : 0;
}
uint64_t emul_ranges_piece_bound(uint64_t n, uint64_t dst_size, uint64_t sb) { return ranges_piece_bound(n, dst_size, sb); }
// out: superblock, lo, hi, destination offset
void emul_ranges_cut(uint64_t sb, uint64_t off, uint64_t len, uint64_t d, uint64_t j, uint64_t* out)
{
	GatherPiece p;
	uint64_t s;
	ranges_cut(sb, off, len, d, j, &s, &p);
	out[0] = s;
	out[1] = p.lo;
	out[2] = p.hi;
	out[3] = p.dst;
}

// ---- the scan passes at block width `width` (4 or 64) ----
// D, pstart: n + 1 entries out; words: status, piece total, D[n].  Returns 0, (size_t)-3 for a width or bound it cannot run.
size_t emul_ranges_offsets(uint64_t total, uint64_t sb, uint64_t dst_size, uint64_t n, const uint64_t* offsets, const uint64_t* lengths, uint32_t width, uint64_t* D,
			   uint32_t* pstart, uint64_t* words)
{
	Tables t;
	if (!t.make(total, sb, dst_size, n, offsets, lengths, width, 0))
		return (size_t)-3;
	t.offsets_of(width);
	memcpy(D, t.D.data(), (n + 1) * 8);
	memcpy(pstart, t.pstart.data(), (n + 1) * 4);
	words[0] = t.words.status;
	words[1] = t.words.npieces;
	words[2] = t.words.total;
	return 0;
}

// ---- the call ----
// The frame src[0, size) of an array of `total` bytes in nsb superblocks of sb, whose headers stand at index[0 .. nsb); n ranges;
// the packed output has out_bytes between its guards and the call is told dst_size.  out: out_bytes; D: n + 1; flags: nsb words;
// words: status, piece total, D[n].  Returns the status word, (size_t)-7 if a byte outside the output and the flag words changed,
// (size_t)-3 for a call it cannot run.
size_t emul_gather_ranges(const uint8_t* src, size_t size, size_t T, uint64_t total, uint64_t sb, uint64_t nsb, const uint64_t* index, uint64_t n,
			  const uint64_t* offsets, const uint64_t* lengths, uint64_t dst_size, size_t out_bytes, uint32_t width, uint8_t* out, uint64_t* D, uint32_t* flags,
			  uint64_t* words, int misalign, int dst_misalign)
{
	Tables t;
	Arenas b;
	if (!t.make(total, sb, dst_size, n, offsets, lengths, width, nsb) || t.a.pmax == 0 || !b.make(src, size, T, t.a.pmax, out_bytes, nsb, misalign, dst_misalign))
		return (size_t)-3;
	const uint32_t r = run_call(t, b, size, T, total, sb, nsb, index, width);
	memcpy(D, t.D.data(), (n + 1) * 8);
	words[0] = t.words.status;
	words[1] = t.words.npieces;
	words[2] = t.words.total;
	return b.collect(out, flags) ? r : (size_t)-7;
}

#ifdef WV_AUDIT
// The same with every memory access of the decoder's source checked (wavevec_host.h, "the access audit"):
//   LDS           the wave's make_dec_layout(T).total bytes, nothing behind them;
//   global reads  the read arena: from the piece table to the end of the 16-byte hull of the frame;
//   global writes the write arena (its guards are checked byte by byte afterwards) -- or, with no_write, NOTHING: every write
//                 the decoder attempts is then counted as a violation and does not take place.
// report: violations, accesses checked, kind, offset and width of the first violation.
static const char* g_audit_first_name = "";
const char* emul_audit_first_name(void) { return g_audit_first_name; }
size_t emul_audit_gather_ranges(const uint8_t* src, size_t size, size_t T, uint64_t total, uint64_t sb, uint64_t nsb, const uint64_t* index, uint64_t n,
				const uint64_t* offsets, const uint64_t* lengths, uint64_t dst_size, size_t out_bytes, uint32_t width, uint8_t* out, uint64_t* D, uint32_t* flags,
				uint64_t* words, int misalign, int dst_misalign, int no_write, uint64_t* report)
{
	Tables t;
	Arenas b;
	if (!t.make(total, sb, dst_size, n, offsets, lengths, width, nsb) || t.a.pmax == 0 || !b.make(src, size, T, t.a.pmax, out_bytes, nsb, misalign, dst_misalign))
		return (size_t)-3;
	wv::AuditState& A = wv::audit_state();
	memset(&A, 0, sizeof A);
	A.lo[wv::WV_AUDIT_LDS] = b.lds;
	A.hi[wv::WV_AUDIT_LDS] = b.lds + b.L.total;
	A.lo[wv::WV_AUDIT_GREAD] = b.rd;
	A.hi[wv::WV_AUDIT_GREAD] = (const uint8_t*)(((uintptr_t)b.from + size + 15) & ~(uintptr_t)15);
	A.lo[wv::WV_AUDIT_GWRITE] = b.to;
	A.hi[wv::WV_AUDIT_GWRITE] = no_write ? b.to : b.to + b.wr_bytes;
	A.on = true;
	const uint32_t r = run_call(t, b, size, T, total, sb, nsb, index, width);
	A.on = false;
	report[0] = A.violations;
	report[1] = A.checked;
	report[2] = (uint64_t)A.first_kind;
	report[3] = (uint64_t)A.first_off;
	report[4] = A.first_width;
	g_audit_first_name = A.first_name ? A.first_name : "";
	memcpy(D, t.D.data(), (n + 1) * 8);
	words[0] = t.words.status;
	words[1] = t.words.npieces;
	words[2] = t.words.total;
	return b.collect(out, flags) ? r : (size_t)-7;
}
#endif

} // extern "C"
