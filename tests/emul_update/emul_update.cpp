// tests/emul_update/emul_update.cpp -- TEST INFRASTRUCTURE.  What one thread or wavefront of update_plan, update_apply,
// update_splice_plan and update_splice does (stenos_amd/csrc/update_codec.h), compiled for the host with WV_HOST_EMULATION as
// tests/emul_gather compiles the piece decoder: 64 lanes in lockstep, the threads of a workgroup one after the other, the
// workgroup's prefix sums by a loop.  Grouping the pieces by superblock (gather_count / gather_scan / gather_fill on the
// device), decoding the touched superblocks and encoding them again are the caller's: the test hands in decoded bytes and
// whatever "encodings" it likes -- the splice does not parse them.  The shipped library never contains or calls this.
#define WV_HOST_EMULATION 1
#include "../../stenos_amd/csrc/update_codec.h"

#include <stdlib.h>
#include <string.h>

#include <vector>

using namespace codec;

enum { GUARD = 64, GUARD_BYTE = 0xA5, PLAN_THREADS = UPDATE_PLAN_THREADS };

namespace {

size_t up64(size_t v) { return (v + 63) & ~(size_t)63; }

// One arena for everything a kernel may read.  In front the tables the planning kernels write (slot, touched, flags, new
// index: the only words they may write); then ppre, the piece table, the encoded stream and its offsets, the old index, the
// source rows, and LAST the frame, shifted off its 16-byte boundary: the arena ends with the frame's last byte, so a read
// behind the frame is a read outside the arena.
struct Arena {
	uint8_t* base = nullptr;
	size_t bytes = 0, w_end = 0;
	UpdateArgs a;
	uint32_t words[UPDATE_WORDS];
	~Arena() { free(base); }
	bool make(const uint8_t* frame, size_t size, const uint64_t* idx, uint32_t nsb, uint32_t sb, uint64_t total, uint32_t header, const uint32_t* ppre,
		  const GatherPiece* pieces, size_t npieces, const uint8_t* src, size_t src_bytes, const uint8_t* enc, size_t enc_bytes, const uint64_t* enc_off,
		  size_t nenc, int misalign)
	{
		const size_t o_slot = 0, o_touched = o_slot + up64(nsb * 4), o_flags = o_touched + up64(nsb * 4), o_new = o_flags + up64(nsb * 4);
		w_end = o_new + up64((nsb + 1) * 8);
		const size_t o_ppre = w_end, o_pieces = o_ppre + up64((nsb + 1) * 4), o_encoff = o_pieces + up64(npieces * sizeof(GatherPiece)),
			     o_enc = o_encoff + up64(nenc * 8), o_idx = o_enc + up64(enc_bytes) + 64, o_src = o_idx + up64((nsb + 1) * 8),
			     o_frame = o_src + up64(src_bytes) + 64 + (size_t)misalign;
		bytes = o_frame + size;
		if (posix_memalign((void**)&base, 64, bytes + 256))
			return false;
		memset(base, 0xEE, bytes + 256);
		memset(base + o_flags, 0, up64(nsb * 4)); // (zero on entry, update.h)
		memcpy(base + o_ppre, ppre, (nsb + 1) * 4);
		memcpy(base + o_pieces, pieces, npieces * sizeof(GatherPiece));
		if (nenc)
			memcpy(base + o_encoff, enc_off, nenc * 8);
		if (enc_bytes)
			memcpy(base + o_enc, enc, enc_bytes);
		memcpy(base + o_idx, idx, (nsb + 1) * 8);
		if (src_bytes)
			memcpy(base + o_src, src, src_bytes);
		memcpy(base + o_frame, frame, size);
		memset(words, 0, sizeof words);
		a = UpdateArgs();
		a.frame = base + o_frame;
		a.size = size;
		a.idx = (const uint64_t*)(base + o_idx);
		a.new_idx = (uint64_t*)(base + o_new);
		a.enc = base + o_enc;
		a.enc_off = (const uint64_t*)(base + o_encoff);
		a.src = base + o_src;
		a.total = total;
		a.sb = sb;
		a.nsb = nsb;
		a.T = 0;
		a.header = header;
		a.words = words;
		a.ppre = (const uint32_t*)(base + o_ppre);
		a.slot = (uint32_t*)(base + o_slot);
		a.touched = (uint32_t*)(base + o_touched);
		a.flags = (uint32_t*)(base + o_flags);
		a.pieces = (const GatherPiece*)(base + o_pieces);
		return true;
	}
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
	Audit(uint64_t* r, const Arena& A, const uint8_t* wlo, const uint8_t* whi) : report(r)
	{
#ifdef WV_AUDIT
		wv::AuditState& S = wv::audit_state();
		memset(&S, 0, sizeof S);
		S.lo[wv::WV_AUDIT_LDS] = S.hi[wv::WV_AUDIT_LDS] = A.base; // (these steps use no LDS through the accessors)
		S.lo[wv::WV_AUDIT_GREAD] = A.base;
		S.hi[wv::WV_AUDIT_GREAD] = A.base + A.bytes;
		S.lo[wv::WV_AUDIT_GWRITE] = wlo;
		S.hi[wv::WV_AUDIT_GWRITE] = whi;
		S.on = true;
#else
		(void)A;
		(void)wlo;
		(void)whi;
#endif
	}
	void next(const uint8_t* wlo, const uint8_t* whi)
	{
#ifdef WV_AUDIT
		wv::AuditState& S = wv::audit_state();
		S.lo[wv::WV_AUDIT_GWRITE] = wlo;
		S.hi[wv::WV_AUDIT_GWRITE] = whi;
#else
		(void)wlo;
		(void)whi;
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

} // namespace

extern "C" {

const char* emul_audit_first_name(void) { return Audit::g_name; }
int emul_update_audited(void)
{
#ifdef WV_AUDIT
	return 1;
#else
	return 0;
#endif
}

// update_plan, then update_apply over slots that hold `decoded` (the original array's bytes: the stand-in for update_decode).
// pieces: the grouped table (ppre: nsb + 1 prefixes); src: the source rows.  Out: slot[nsb], touched[nsb], flags[nsb],
// words[UPDATE_WORDS], raw[k * sb] (the slots after the apply).  Returns 0, (size_t)-7 if a byte outside the slots' bytes
// [0, (k - 1) * sb + bytes of the last touched superblock) changed, (size_t)-3 for no memory.
size_t emul_update_plan_apply(const uint8_t* frame, size_t size, const uint64_t* idx, uint32_t nsb, uint32_t sb, uint64_t total, uint32_t header, const uint32_t* ppre,
			      const void* pieces, size_t npieces, const uint8_t* src, size_t src_bytes, const uint8_t* decoded, int misalign, int raw_misalign,
			      uint32_t* slot, uint32_t* touched, uint32_t* flags, uint32_t* words, uint8_t* raw, uint64_t* report)
{
	Arena A;
	if (!A.make(frame, size, idx, nsb, sb, total, header, ppre, (const GatherPiece*)pieces, npieces, src, src_bytes, nullptr, 0, nullptr, 0, misalign))
		return (size_t)-3;
	UpdateArgs& a = A.a;
	Guarded R;
	size_t raw_bytes = 0;
	{
		Audit au(report, A, A.base, A.base + A.w_end);
		// update_plan: every thread counts, the workgroup's sums, every thread writes
		std::vector<uint32_t> t(PLAN_THREADS), pre(PLAN_THREADS);
		uint32_t k = 0;
		for (uint32_t th = 0; th < PLAN_THREADS; ++th) {
			uint32_t b, e;
			update_run_of_thread(nsb, th, &b, &e);
			t[th] = update_plan_count(a, b, e);
			pre[th] = k;
			k += t[th];
		}
		for (uint32_t th = 0; th < PLAN_THREADS; ++th) {
			uint32_t b, e, last = 0;
			update_run_of_thread(nsb, th, &b, &e);
			a.words[UPDATE_W_STATUS] |= update_plan_write(a, b, e, pre[th], &last);
			if (t[th] && last > a.words[UPDATE_W_LAST])
				a.words[UPDATE_W_LAST] = last;
		}
		a.words[UPDATE_W_K] = k;
		a.k = k;
		if (k) {
			const uint64_t lastb = (uint64_t)a.words[UPDATE_W_LAST] * sb;
			raw_bytes = (size_t)(k - 1) * sb + (size_t)(total - lastb < sb ? total - lastb : sb);
		}
		if (!R.make(raw_bytes, raw_misalign))
			return (size_t)-3;
		a.raw = R.at;
		for (uint32_t c = 0; c < k; ++c) { // (the stand-in for update_decode)
			const uint64_t s = a.touched[c], begin = s * sb;
			memcpy(a.raw + (size_t)c * sb, decoded + begin, (size_t)(total - begin < sb ? total - begin : sb));
		}
		au.next(R.at, R.at + raw_bytes);
		for (uint32_t c = 0; c < k; ++c)
			for (uint32_t w = 0; w < UPDATE_APPLY_WAVES; ++w)
				update_apply_wave(a, c, w);
	}
	memcpy(slot, a.slot, nsb * 4);
	memcpy(touched, a.touched, a.k * 4);
	memcpy(flags, a.flags, nsb * 4);
	memcpy(words, a.words, sizeof A.words);
	memcpy(raw, R.at, raw_bytes);
	return R.intact(raw_bytes) ? 0 : (size_t)-7;
}

// update_splice_plan and, if it raises no status bit and the new frame fits in out_cap, update_splice into an arena of out_cap
// bytes between guards.  slot: from the call above; enc / enc_off: the touched superblocks' new bytes, k + 1 offsets.
// Out: new_idx[nsb + 1], words, out[new total].  Returns the new total, (size_t)-4 / -2 for a refused index (INVALID /
// TRUNCATED), (size_t)-6 if it does not fit, (size_t)-7 if a byte of the arena outside [0, new total) changed -- after a refusal,
// any byte at all.
size_t emul_update_splice(const uint8_t* frame, size_t size, const uint64_t* idx, uint32_t nsb, uint32_t header, const uint32_t* slot, const uint8_t* enc,
			  size_t enc_bytes, const uint64_t* enc_off, uint32_t k, size_t out_cap, int misalign, int out_misalign, uint64_t* new_idx, uint32_t* words,
			  uint8_t* out, uint64_t* report)
{
	Arena A;
	std::vector<uint32_t> ppre(nsb + 1, 0);
	if (!A.make(frame, size, idx, nsb, 0, 0, header, ppre.data(), nullptr, 0, nullptr, 0, enc, enc_bytes, enc_off, (size_t)k + 1, misalign))
		return (size_t)-3;
	UpdateArgs& a = A.a;
	memcpy(a.slot, slot, nsb * 4);
	a.k = k;
	Guarded O;
	if (!O.make(out_cap, out_misalign))
		return (size_t)-3;
	a.out = O.at;
	size_t result;
	uint64_t total = 0;
	{
		Audit au(report, A, A.base, A.base + A.w_end);
		std::vector<uint64_t> sum(PLAN_THREADS), pre(PLAN_THREADS);
		uint32_t st = 0;
		for (uint32_t th = 0; th < PLAN_THREADS; ++th) {
			uint32_t b, e;
			update_run_of_thread(nsb, th, &b, &e);
			sum[th] = update_splice_sum(a, b, e, &st);
			pre[th] = total;
			total += sum[th];
		}
		a.words[UPDATE_W_STATUS] |= st;
		for (uint32_t th = 0; th < PLAN_THREADS; ++th) {
			uint32_t b, e;
			update_run_of_thread(nsb, th, &b, &e);
			update_splice_write(a, b, e, header + pre[th]);
		}
		total += header;
		a.new_idx[nsb] = total;
		a.words[UPDATE_W_TOTAL] = (uint32_t)total;
		a.words[UPDATE_W_TOTAL + 1] = (uint32_t)(total >> 32);
		// (the host's part, update_host.cpp: nothing is launched after a status bit or when the frame does not fit)
		if (st & UPDATE_ST_TRUNCATED)
			result = (size_t)-2;
		else if (st & UPDATE_ST_INVALID)
			result = (size_t)-4;
		else if (total > out_cap)
			result = (size_t)-6;
		else {
			result = (size_t)total;
			au.next(O.at, O.at + total);
			for (uint32_t s = 0; s < (nsb ? nsb : 1u); ++s)
				for (uint32_t w = 0; w < UPDATE_SPLICE_WAVES; ++w)
					update_splice_wave(a, s, w);
		}
	}
	memcpy(new_idx, a.new_idx, ((size_t)nsb + 1) * 8);
	memcpy(words, a.words, sizeof A.words);
	const size_t used = result == (size_t)total ? (size_t)total : 0;
	memcpy(out, O.at, used);
	return O.intact(used) ? result : (size_t)-7;
}

} // extern "C"
