// Host emulation of the piece plan of stenos_hip_gather_rows_batch (test infrastructure, see tests/test_gather_batch_cpu.py): the
// pair-cutting function and the searches of csrc/gather_codec.h -- the one copy the kernels (gather_batch_kernels.hip) and the
// host unit (gather_batch_host.cpp) compile -- driven through the sequence of the kernels in plain C++: count, scan, fill, and
// the chunks the decode wavefronts would take.
#define GATHER_CUT_ONLY
#include "../../stenos_amd/csrc/gather_codec.h"

#include <vector>

using namespace codec;

// the frame table as the host unit makes it (gather_frame), the `first` array and the call's pieces per pair
struct Batch {
	std::vector<GatherFrame> frames;
	std::vector<uint64_t> first;
	uint64_t S = 0, P = 1;
	Batch(uint64_t m, const uint64_t* totals, const uint64_t* sbs, uint64_t row_bytes)
	{
		for (uint64_t f = 0; f < m; ++f) {
			const uint64_t nsb = totals[f] ? totals[f] / sbs[f] + (totals[f] % sbs[f] ? 1 : 0) : 0;
			frames.push_back(gather_frame(nullptr, 0, totals[f], sbs[f], nsb, S, row_bytes));
			first.push_back(S);
			S += nsb;
			if (frames.back().pieces > P)
				P = frames.back().pieces;
		}
		first.push_back(S);
	}
};

extern "C" {

// out: P of the call, S, then per frame: first, nsb, valid rows, pieces
void emul_gb_table(uint64_t m, const uint64_t* totals, const uint64_t* sbs, uint64_t row_bytes, uint64_t* out)
{
	const Batch b(m, totals, sbs, row_bytes);
	out[0] = b.P;
	out[1] = b.S;
	for (uint64_t f = 0; f < m; ++f) {
		out[2 + 4 * f] = b.frames[f].first;
		out[3 + 4 * f] = b.frames[f].nsb;
		out[4 + 4 * f] = b.frames[f].valid_rows;
		out[5 + 4 * f] = b.frames[f].pieces;
	}
}

// gather_cut_pair for one (pair, slot, piece): its result; out: global superblock, lo, hi, destination offset (a piece only)
int emul_gb_cut_pair(uint64_t m, const uint64_t* totals, const uint64_t* sbs, uint64_t row_bytes, uint64_t dst_stride, uint64_t fid, uint64_t row, uint64_t i, uint64_t j,
		     uint64_t* out)
{
	const Batch b(m, totals, sbs, row_bytes);
	GatherPiece p;
	uint64_t g;
	const int r = gather_cut_pair(b.frames.data(), m, row_bytes, dst_stride, fid, row, i, j, &g, &p);
	if (r == GATHER_PAIR_PIECE) {
		out[0] = g;
		out[1] = p.lo;
		out[2] = p.hi;
		out[3] = p.dst;
	}
	return r;
}

// The whole plan for n pairs.  pieces: 4 words per piece in table order (global superblock, lo, hi, dst), room for n * P;
// chunks: 4 words per decode wavefront that has work (global superblock, frame, first piece, count), room for `chunk_room`.
// info: pieces, wavefronts with work (wpre[S]), bad-pair flag, P, S.  Returns 0, or 1 when the chunks do not fit.
int emul_gb_plan(uint64_t m, const uint64_t* totals, const uint64_t* sbs, uint64_t row_bytes, uint64_t dst_stride, uint64_t n, const uint64_t* fids, const uint64_t* rows,
		 uint64_t* pieces, uint64_t* chunks, uint64_t chunk_room, uint64_t* info)
{
	const Batch b(m, totals, sbs, row_bytes);
	const uint64_t S = b.S, P = b.P, threads = n * P;
	std::vector<uint32_t> count(S, 0), ppre(S + 1, 0), wpre(S + 1, 0);
	std::vector<GatherPiece> table(threads);
	std::vector<uint64_t> table_g(threads);
	uint64_t bad = 0;
	// thread t = i * P + j, as piece_of_thread of the kernels
	auto piece = [&](uint64_t t, uint64_t* g, GatherPiece* p) {
		const uint64_t i = t / P, j = t - i * P;
		const int r = gather_cut_pair(b.frames.data(), m, row_bytes, dst_stride, fids[i], rows[i], i, j, g, p);
		if (r == GATHER_PAIR_INVALID && j == 0)
			bad = 1;
		return r == GATHER_PAIR_PIECE;
	};
	uint64_t g;
	GatherPiece p;
	for (uint64_t t = 0; t < threads; ++t) // gather_batch_count
		if (piece(t, &g, &p))
			count[g] += 1;
	uint32_t ps = 0, ws = 0;
	for (uint64_t s = 0; s < S; ++s) { // gather_scan
		ppre[s] = ps;
		wpre[s] = ws;
		ps += count[s];
		ws += (count[s] + 63u) >> 6;
		count[s] = 0;
	}
	ppre[S] = ps;
	wpre[S] = ws;
	for (uint64_t t = 0; t < threads; ++t) // gather_batch_fill
		if (piece(t, &g, &p)) {
			const uint32_t at = ppre[g] + count[g]++;
			table[at] = p;
			table_g[at] = g;
		}
	for (uint32_t k = 0; k < ps; ++k) {
		pieces[4 * k] = table_g[k];
		pieces[4 * k + 1] = table[k].lo;
		pieces[4 * k + 2] = table[k].hi;
		pieces[4 * k + 3] = table[k].dst;
	}
	info[0] = ps;
	info[1] = ws;
	info[2] = bad;
	info[3] = P;
	info[4] = S;
	if (ws > chunk_room)
		return 1;
	for (uint32_t w = 0; w < ws; ++w) { // gather_batch_decode: the wavefronts below wpre[S]
		const uint32_t gs = gather_find32(wpre.data(), (uint32_t)S, w);
		const uint32_t f = gather_find64(b.first.data(), (uint32_t)m, gs);
		const uint32_t first = ppre[gs] + 64u * (w - wpre[gs]), left = ppre[gs + 1] - first;
		chunks[4 * w] = gs;
		chunks[4 * w + 1] = f;
		chunks[4 * w + 2] = first;
		chunks[4 * w + 3] = left < 64u ? left : 64u;
	}
	return 0;
}

} // extern "C"
