// tests/emul_update_batch/emul_update_batch.cpp -- TEST INFRASTRUCTURE.  What one thread or wavefront of update_batch_plan,
// update_batch_apply, update_batch_splice_plan and update_batch_splice does (stenos_amd/csrc/update_codec.h), compiled for the
// host with WV_HOST_EMULATION as tests/emul_update compiles the single call's steps: 64 lanes in lockstep, the threads of a
// workgroup one after the other, the workgroup's prefix sums by a loop.  Grouping the pieces by superblock, decoding the touched
// superblocks and encoding them again are the caller's: the test hands in decoded bytes and whatever "encodings" it likes -- the
// splice does not parse them.  The shipped library never contains or calls this.
//
// The access audit has one read range and one write range at a time.  Everything a kernel may read lies in one arena: the
// tables in front, then the source rows, then the frames one after the other, each ending with its last byte.  While the work of
// frame f is emulated the read range ENDS with frame f's last byte (a planning thread's run is cut at the frames' boundaries for
// that: the same function over the parts), so a read behind the frame is a read outside its arena.  The write range is the
// planning tables, then the slots, then [0, new total_f) of output f.
#define WV_HOST_EMULATION 1
#include "../../stenos_amd/csrc/update_codec.h"

#include <stdlib.h>
#include <string.h>

#include <vector>

using namespace codec;

enum { GUARD = 64, GUARD_BYTE = 0xA5, PLAN_THREADS = UPDATE_PLAN_THREADS };

namespace {

size_t up64(size_t v) { return (v + 63) & ~(size_t)63; }

struct Arena {
	uint8_t* base = nullptr;
	size_t bytes = 0, w_end = 0;
	UpdateBatchArgs a;
	uint32_t words[UPDATE_WORDS];
	std::vector<const uint8_t*> frame_end;
	~Arena() { free(base); }
	bool make(uint32_t m, const uint8_t* cat, size_t cat_bytes, const uint64_t* frame_off, const uint64_t* sizes, const uint64_t* totals, const uint64_t* headers, uint32_t sb,
		  const uint64_t* idx, const uint32_t* ppre, const GatherPiece* pieces, size_t npieces, const uint8_t* src, size_t src_bytes, const uint8_t* enc, size_t enc_bytes,
		  const uint64_t* enc_base, const uint64_t* enc_off, size_t nenc, int misalign)
	{
		std::vector<uint64_t> first(m + 1, 0);
		for (uint32_t f = 0; f < m; ++f)
			first[f + 1] = first[f] + (totals[f] ? totals[f] / sb + (totals[f] % sb ? 1 : 0) : 0);
		const uint32_t S = (uint32_t)first[m];
		// written by the planning steps: slot, touched, flags, kf, new index, gpre, totals
		const size_t o_slot = 0, o_touched = o_slot + up64(S * 4), o_flags = o_touched + up64(S * 4), o_kf = o_flags + up64(S * 4), o_new = o_kf + up64(m * 8),
			     o_gpre = o_new + up64((S + m) * 8), o_totals = o_gpre + up64((S + 1) * 8);
		w_end = o_totals + up64(m * 8);
		const size_t o_frames = w_end, o_first = o_frames + up64(m * sizeof(GatherFrame)), o_header = o_first + up64((m + 1) * 8), o_outs = o_header + up64(m * 8),
			     o_ppre = o_outs + up64(m * 8), o_pieces = o_ppre + up64((S + 1) * 4), o_ebase = o_pieces + up64(npieces * sizeof(GatherPiece)),
			     o_encoff = o_ebase + up64(m * 8), o_enc = o_encoff + up64(nenc * 8), o_idx = o_enc + up64(enc_bytes) + 64, o_src = o_idx + up64((S + m) * 8),
			     o_cat = o_src + up64(src_bytes) + 64 + (size_t)misalign;
		bytes = o_cat + cat_bytes;
		if (posix_memalign((void**)&base, 64, bytes + 256))
			return false;
		memset(base, 0xEE, bytes + 256);
		memset(base + o_flags, 0, up64(S * 4) + up64(m * 8)); // (flags and kf: zero on entry, update_batch.h)
		GatherFrame* fr = (GatherFrame*)(base + o_frames);
		for (uint32_t f = 0; f < m; ++f) {
			fr[f] = gather_frame(base + o_cat + frame_off[f], sizes[f], totals[f], sb, first[f + 1] - first[f], first[f], 1);
			frame_end.push_back(base + o_cat + frame_off[f] + sizes[f]);
		}
		memcpy(base + o_first, first.data(), (m + 1) * 8);
		memcpy(base + o_header, headers, m * 8);
		memcpy(base + o_ppre, ppre, (S + 1) * 4);
		if (npieces)
			memcpy(base + o_pieces, pieces, npieces * sizeof(GatherPiece));
		if (enc_base)
			memcpy(base + o_ebase, enc_base, m * 8);
		if (nenc)
			memcpy(base + o_encoff, enc_off, nenc * 8);
		if (enc_bytes)
			memcpy(base + o_enc, enc, enc_bytes);
		memcpy(base + o_idx, idx, (S + m) * 8);
		if (src_bytes)
			memcpy(base + o_src, src, src_bytes);
		memcpy(base + o_cat, cat, cat_bytes);
		memset(words, 0, sizeof words);
		a = UpdateBatchArgs();
		a.frames = fr;
		a.first = (const uint64_t*)(base + o_first);
		a.header = (const uint64_t*)(base + o_header);
		a.outs = (uint8_t* const*)(base + o_outs);
		a.idx = (const uint64_t*)(base + o_idx);
		a.new_idx = (uint64_t*)(base + o_new);
		a.gpre = (uint64_t*)(base + o_gpre);
		a.totals = (uint64_t*)(base + o_totals);
		a.enc = base + o_enc;
		a.enc_base = (const uint64_t*)(base + o_ebase);
		a.enc_off = (const uint64_t*)(base + o_encoff);
		a.src = base + o_src;
		a.sb = sb;
		a.m = m;
		a.S = S;
		a.words = words;
		a.ppre = (const uint32_t*)(base + o_ppre);
		a.slot = (uint32_t*)(base + o_slot);
		a.touched = (uint32_t*)(base + o_touched);
		a.flags = (uint32_t*)(base + o_flags);
		a.kf = (uint32_t*)(base + o_kf);
		a.pieces = (const GatherPiece*)(base + o_pieces);
		return true;
	}
	uint32_t frame_of(uint32_t g) const { return gather_find64(a.first, a.m, g); }
};

// a write arena: a guard, the region shifted by `misalign`, a guard
struct Guarded {
	uint8_t *base = nullptr, *at = nullptr;
	size_t cap = 0;
	~Guarded() { free(base); }
	bool make(size_t n, int misalign)
	{
		cap = n;
		if (posix_memalign((void**)&base, 64, n + 2 * GUARD + 128))
			return false;
		memset(base, GUARD_BYTE, n + 2 * GUARD + 128);
		at = base + GUARD + misalign;
		return true;
	}
	// every byte outside [at, at + used) is a guard byte still
	bool intact(size_t used) const
	{
		for (const uint8_t* p = base; p < at; ++p)
			if (*p != GUARD_BYTE)
				return false;
		for (const uint8_t* p = at + used; p < base + cap + 2 * GUARD + 128; ++p)
			if (*p != GUARD_BYTE)
				return false;
		return true;
	}
};

struct Audit {
	uint64_t* report;
	Audit(uint64_t* r, const Arena& A) : report(r)
	{
#ifdef WV_AUDIT
		wv::AuditState& S = wv::audit_state();
		memset(&S, 0, sizeof S);
		S.lo[wv::WV_AUDIT_LDS] = S.hi[wv::WV_AUDIT_LDS] = A.base; // (these steps use no LDS through the accessors)
		S.lo[wv::WV_AUDIT_GREAD] = A.base;
		S.hi[wv::WV_AUDIT_GREAD] = A.base + A.bytes;
		S.lo[wv::WV_AUDIT_GWRITE] = A.base;
		S.hi[wv::WV_AUDIT_GWRITE] = A.base + A.w_end;
		S.on = true;
#else
		(void)A;
#endif
	}
	void reads_end(const uint8_t* hi)
	{
#ifdef WV_AUDIT
		wv::audit_state().hi[wv::WV_AUDIT_GREAD] = hi;
#else
		(void)hi;
#endif
	}
	void writes(const uint8_t* lo, const uint8_t* hi)
	{
#ifdef WV_AUDIT
		wv::AuditState& S = wv::audit_state();
		S.lo[wv::WV_AUDIT_GWRITE] = lo;
		S.hi[wv::WV_AUDIT_GWRITE] = hi;
#else
		(void)lo;
		(void)hi;
#endif
	}
	~Audit()
	{
#ifdef WV_AUDIT
		wv::AuditState& S = wv::audit_state();
		S.on = false;
		report[0] = S.violations;
		report[1] = S.checked;
		report[2] = (uint64_t)S.first_kind;
		report[3] = (uint64_t)S.first_off;
		report[4] = S.first_width;
		g_name = S.first_name ? S.first_name : "";
#else
		memset(report, 0, 5 * sizeof(uint64_t));
#endif
	}
	static const char* g_name;
};
const char* Audit::g_name = "";

// fn(f, begin, end) for the parts of [begin, end) that lie in one frame each
template <class F>
void by_frame(const Arena& A, uint32_t begin, uint32_t end, F fn)
{
	while (begin < end) {
		const uint32_t f = A.frame_of(begin);
		const uint32_t stop = (uint32_t)(A.a.first[f + 1] < end ? A.a.first[f + 1] : end);
		fn(f, begin, stop);
		begin = stop;
	}
}

} // namespace

extern "C" {

const char* emul_audit_first_name(void) { return Audit::g_name; }
int emul_update_batch_audited(void)
{
#ifdef WV_AUDIT
	return 1;
#else
	return 0;
#endif
}

// update_batch_plan, then update_batch_apply over slots that hold the arrays' bytes (decoded_cat + dec_off[f]: the stand-in for
// update_batch_decode).  The frames lie in `cat` at frame_off[f] (two entries may name the same bytes).  Out: slot[S], touched[S],
// flags[S], words[UPDATE_WORDS], kf[2 m], raw[K * sb] (the slots after the apply).  Returns 0, (size_t)-7 if a byte outside the
// slots' decoded bytes changed, (size_t)-3 for no memory.
size_t emul_ub_plan_apply(uint32_t m, const uint8_t* cat, size_t cat_bytes, const uint64_t* frame_off, const uint64_t* sizes, const uint64_t* totals, const uint64_t* headers,
			  uint32_t sb, const uint64_t* idx, const uint32_t* ppre, const void* pieces, size_t npieces, const uint8_t* src, size_t src_bytes,
			  const uint8_t* decoded_cat, const uint64_t* dec_off, int misalign, int raw_misalign, uint32_t* slot, uint32_t* touched, uint32_t* flags, uint32_t* words,
			  uint32_t* kf, uint8_t* raw, uint64_t* report)
{
	Arena A;
	if (!A.make(m, cat, cat_bytes, frame_off, sizes, totals, headers, sb, idx, ppre, (const GatherPiece*)pieces, npieces, src, src_bytes, nullptr, 0, nullptr, nullptr, 0, misalign))
		return (size_t)-3;
	UpdateBatchArgs& a = A.a;
	const uint32_t S = a.S;
	Guarded R;
	uint32_t K = 0;
	bool slack_intact = true;
	{
		Audit au(report, A);
		// update_batch_plan: every thread counts, the workgroup's sums, every thread writes
		std::vector<uint32_t> pre(PLAN_THREADS);
		for (uint32_t th = 0; th < PLAN_THREADS; ++th) {
			uint32_t b, e;
			update_run_of_thread(S, th, &b, &e);
			pre[th] = K;
			K += update_plan_count(a, b, e);
		}
		for (uint32_t th = 0; th < PLAN_THREADS; ++th) {
			uint32_t b, e, c = pre[th];
			update_run_of_thread(S, th, &b, &e);
			by_frame(A, b, e, [&](uint32_t f, uint32_t pb, uint32_t pe) {
				au.reads_end(A.frame_end[f]);
				a.words[UPDATE_W_STATUS] |= update_batch_plan_write(a, pb, pe, c);
				c += update_plan_count(a, pb, pe);
			});
		}
		au.reads_end(A.base + A.bytes);
		a.words[UPDATE_W_K] = K;
		a.K = K;
		if (!R.make((size_t)K * sb, raw_misalign))
			return (size_t)-3;
		a.raw = R.at;
		std::vector<uint32_t> dsize(K);
		for (uint32_t c = 0; c < K; ++c) { // (the stand-in for update_batch_decode)
			const uint32_t g = a.touched[c], f = A.frame_of(g);
			const uint64_t begin = (g - a.first[f]) * (uint64_t)sb;
			dsize[c] = (uint32_t)(totals[f] - begin < sb ? totals[f] - begin : sb);
			memcpy(a.raw + (size_t)c * sb, decoded_cat + dec_off[f] + begin, dsize[c]);
		}
		for (uint32_t c = 0; c < K; ++c) {
			au.writes(R.at + (size_t)c * sb, R.at + (size_t)c * sb + dsize[c]);
			for (uint32_t w = 0; w < UPDATE_APPLY_WAVES; ++w)
				update_batch_apply_wave(a, c, w);
		}
		for (uint32_t c = 0; c < K; ++c) // (behind a short superblock's bytes the slot is still what it was)
			for (size_t i = dsize[c]; i < sb; ++i)
				slack_intact &= R.at[(size_t)c * sb + i] == GUARD_BYTE;
	}
	memcpy(slot, a.slot, S * 4);
	memcpy(touched, a.touched, K * 4);
	memcpy(flags, a.flags, S * 4);
	memcpy(words, a.words, sizeof A.words);
	memcpy(kf, a.kf, m * 8);
	memcpy(raw, R.at, (size_t)K * sb);
	return R.intact((size_t)K * sb) && slack_intact ? 0 : (size_t)-7;
}

// update_batch_splice_plan and, if it raises no status bit and every new frame fits its out_caps[f], update_batch_splice into
// one arena per output between guards.  slot: from the call above; enc / enc_base / enc_off: the touched superblocks' new bytes
// (K + m offsets, update_codec.h).  Out: new_idx[S + m], new_totals[m], words, out (output f at the sum of the caps in front of
// it).  Returns 0, (size_t)-4 / -2 for a refused index (INVALID / TRUNCATED), (size_t)-6 if a frame does not fit, (size_t)-7 if a
// byte of an output arena outside [0, new total_f) changed -- after a refusal, any byte at all.
size_t emul_ub_splice(uint32_t m, const uint8_t* cat, size_t cat_bytes, const uint64_t* frame_off, const uint64_t* sizes, const uint64_t* totals, const uint64_t* headers,
		      uint32_t sb, const uint64_t* idx, const uint32_t* slot, const uint8_t* enc, size_t enc_bytes, const uint64_t* enc_base, const uint64_t* enc_off, uint32_t K,
		      const uint64_t* out_caps, int misalign, int out_misalign, uint64_t* new_idx, uint64_t* new_totals, uint32_t* words, uint8_t* out, uint64_t* report)
{
	Arena A;
	uint64_t S64 = 0;
	for (uint32_t f = 0; f < m; ++f)
		S64 += totals[f] ? totals[f] / sb + (totals[f] % sb ? 1 : 0) : 0;
	std::vector<uint32_t> ppre(S64 + 1, 0);
	if (!A.make(m, cat, cat_bytes, frame_off, sizes, totals, headers, sb, idx, ppre.data(), nullptr, 0, nullptr, 0, enc, enc_bytes, enc_base, enc_off, (size_t)K + m, misalign))
		return (size_t)-3;
	UpdateBatchArgs& a = A.a;
	const uint32_t S = a.S;
	memcpy(a.slot, slot, S * 4);
	a.K = K;
	std::vector<Guarded> O(m);
	for (uint32_t f = 0; f < m; ++f) {
		if (!O[f].make((size_t)out_caps[f], out_misalign))
			return (size_t)-3;
		((uint8_t**)a.outs)[f] = O[f].at;
	}
	size_t result = 0;
	bool ran = false;
	{
		Audit au(report, A);
		std::vector<uint64_t> pre(PLAN_THREADS);
		uint64_t total = 0;
		uint32_t st = 0;
		for (uint32_t th = 0; th < PLAN_THREADS; ++th) {
			uint32_t b, e;
			update_run_of_thread(S, th, &b, &e);
			pre[th] = total;
			total += update_batch_splice_sum(a, b, e, &st);
		}
		a.words[UPDATE_W_STATUS] |= st;
		for (uint32_t th = 0; th < PLAN_THREADS; ++th) {
			uint32_t b, e;
			update_run_of_thread(S, th, &b, &e);
			update_batch_splice_write(a, b, e, pre[th]);
		}
		a.gpre[S] = total;
		for (uint32_t th = 0; th < PLAN_THREADS; ++th) {
			uint32_t b, e;
			update_run_of_thread(S, th, &b, &e);
			update_batch_splice_index(a, b, e);
			for (uint32_t f = th; f < m; f += PLAN_THREADS)
				update_batch_splice_total(a, f);
		}
		// (the host's part, update_batch_host.cpp: nothing is launched after a status bit or when a frame does not fit)
		if (st & UPDATE_ST_TRUNCATED)
			result = (size_t)-2;
		else if (st & UPDATE_ST_INVALID)
			result = (size_t)-4;
		else {
			for (uint32_t f = 0; f < m; ++f)
				if (a.totals[f] > out_caps[f])
					result = (size_t)-6;
		}
		if (!result) {
			ran = true;
			for (uint32_t x = 0; x < S + m; ++x) {
				const uint32_t f = x < S ? A.frame_of(x) : x - S;
				au.reads_end(A.frame_end[f]);
				au.writes(O[f].at, O[f].at + a.totals[f]);
				for (uint32_t w = 0; w < UPDATE_SPLICE_WAVES; ++w)
					update_batch_splice_wave(a, x, w);
			}
		}
	}
	memcpy(new_idx, a.new_idx, ((size_t)S + m) * 8);
	memcpy(new_totals, a.totals, (size_t)m * 8);
	memcpy(words, a.words, sizeof A.words);
	size_t at = 0;
	for (uint32_t f = 0; f < m; ++f) {
		const size_t used = ran ? (size_t)a.totals[f] : 0;
		memcpy(out + at, O[f].at, used);
		at += (size_t)out_caps[f];
		if (!O[f].intact(used))
			return (size_t)-7;
	}
	return result;
}

} // extern "C"
