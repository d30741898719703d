// tests/emul_append/emul_append.cpp -- TEST INFRASTRUCTURE.  What one thread or wavefront of append_plan, append_commit_plan
// and append_commit does (stenos_amd/csrc/append_codec.h), compiled for the host with WV_HOST_EMULATION as tests/emul_update
// compiles the update's steps: 64 lanes in lockstep, the threads of a grid one after the other.  Decoding the partial last
// superblock and encoding the new ones are the caller's: the test hands in whatever "encodings" it likes -- the commit does not
// parse them.  The shipped library never contains or calls this.
#define WV_HOST_EMULATION 1
#include "../../stenos_amd/csrc/append_codec.h"

#include <stdlib.h>
#include <string.h>

using namespace codec;

enum { GUARD = 64, GUARD_BYTE = 0xA5 };

namespace {

size_t up64(size_t v) { return (v + 63) & ~(size_t)63; }

// One allocation.  In front the words and the index (all the planning steps may write); then the encoder's offsets and its
// streams, shifted off their alignment; LAST the buffer of the frame between two guards, shifted as well.  What a kernel may
// read ends with the frame's last byte -- [base, frame + size) -- so a read behind the frame is a read outside the arena.
struct Arena {
	uint8_t *base = nullptr, *frame = nullptr;
	size_t w_end = 0, cap = 0;
	AppendArgs a;
	~Arena() { free(base); }
	bool make(const uint8_t* fr, size_t size, size_t capacity, const uint64_t* idx, size_t nidx, size_t idx_room, const uint8_t* enc, size_t enc_bytes,
		  const uint64_t* enc_off, size_t nenc, int mis_frame, int mis_enc)
	{
		const size_t o_idx = 64;
		w_end = o_idx + up64(idx_room * 8);
		const size_t o_encoff = w_end, o_enc = o_encoff + up64(nenc * 8) + 64 + (size_t)mis_enc, o_guard = up64(o_enc + enc_bytes) + 64,
			     o_frame = o_guard + GUARD + (size_t)mis_frame, bytes = o_frame + capacity + GUARD;
		cap = capacity;
		if (posix_memalign((void**)&base, 64, bytes + 64))
			return false;
		memset(base, 0xEE, o_guard);
		memset(base + o_guard, GUARD_BYTE, bytes + 64 - o_guard);
		memset(base, 0, 64); // (the words: zero on entry)
		memcpy(base + o_idx, idx, nidx * 8);
		if (nenc)
			memcpy(base + o_encoff, enc_off, nenc * 8);
		if (enc_bytes)
			memcpy(base + o_enc, enc, enc_bytes);
		frame = base + o_frame;
		memcpy(frame, fr, size);
		a = AppendArgs();
		a.frame = frame;
		a.size = size;
		a.idx = (uint64_t*)(base + o_idx);
		a.enc = base + o_enc;
		a.enc_off = (const uint64_t*)(base + o_encoff);
		a.words = (uint32_t*)base;
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
		S.hi[wv::WV_AUDIT_GREAD] = A.frame + A.a.size;
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

size_t status_code(uint32_t st)
{
	if (st & UPDATE_ST_TRUNCATED)
		return (size_t)-2;
	if (st & UPDATE_ST_INVALID)
		return (size_t)-4;
	return 0;
}

} // namespace

extern "C" {

const char* emul_audit_first_name(void) { return Audit::g_name; }
int emul_append_audited(void)
{
#ifdef WV_AUDIT
	return 1;
#else
	return 0;
#endif
}
uint32_t emul_append_plan_threads(void) { return APPEND_PLAN_THREADS; }
uint32_t emul_append_commit_chunk(void) { return APPEND_COMMIT_CHUNK; }

// append_plan; then, if it raises no error bit, append_commit_plan over the grid the launcher makes for k threads; then, if
// that raises none and the new frame fits in `capacity`, append_commit (the host's part, append_host.cpp: nothing is launched
// after a status bit or when the frame does not fit).  frame[0 .. size): the old frame, in a buffer of `capacity` bytes between
// guards; idx: nidx entries of its index (the call reads entries keep and, with r > 0, keep + 1); enc, enc_off: the new
// superblocks' bytes in one or two streams and the encoder's offsets (append_codec.h, AppendArgs).
// Out: new_idx[keep + k + 1] (the call's index afterwards), words[APPEND_WORDS], buffer[GUARD + capacity + GUARD] (the frame's
// buffer with both guards).  Returns the new total, (size_t)-4 / -2 for a refused index or stream (INVALID / TRUNCATED),
// (size_t)-6 if the new frame does not fit, (size_t)-3 for no memory.
size_t emul_append(const uint8_t* frame, size_t size, size_t capacity, const uint64_t* idx, size_t nidx, uint32_t keep, uint32_t r, uint32_t k, uint32_t k0,
		   uint32_t header, uint64_t new_bytes, const uint8_t* enc, size_t enc_bytes, uint64_t enc_base1, const uint64_t* enc_off, size_t nenc, int mis_frame,
		   int mis_enc, uint64_t* new_idx, uint32_t* words, uint8_t* buffer, uint64_t* report)
{
	Arena A;
	const size_t idx_room = (size_t)keep + k + 2 > nidx ? (size_t)keep + k + 2 : nidx;
	if (!A.make(frame, size, capacity, idx, nidx, idx_room, enc, enc_bytes, enc_off, nenc, mis_frame, mis_enc))
		return (size_t)-3;
	AppendArgs& a = A.a;
	a.enc_base1 = enc_base1;
	a.new_bytes = new_bytes;
	a.keep = keep;
	a.r = r;
	a.k = k;
	a.k0 = k0;
	a.header = header;
	size_t result;
	{
		Audit au(report, A, A.base, A.base + A.w_end);
		append_plan_thread(a);
		result = status_code(a.words[APPEND_W_STATUS]);
		if (!result) {
			const uint32_t groups = (k + APPEND_PLAN_THREADS - 1) / APPEND_PLAN_THREADS;
			for (uint32_t g = 0; g < groups; ++g)
				for (uint32_t t = 0; t < APPEND_PLAN_THREADS; ++t)
					a.words[APPEND_W_STATUS] |= append_commit_plan_thread(a, g * APPEND_PLAN_THREADS + t);
			result = status_code(a.words[APPEND_W_STATUS]);
		}
		if (!result) {
			const uint64_t total = append_word64(a.words, APPEND_W_TOTAL), p = append_word64(a.words, APPEND_W_P);
			if (total > capacity)
				result = (size_t)-6;
			else {
				result = (size_t)total;
				const uint64_t waves = append_commit_chunks(append_word64(a.words, APPEND_W_LEN0)) + append_commit_chunks(append_word64(a.words, APPEND_W_LEN1));
				const uint64_t groups = (waves + APPEND_COMMIT_WAVES - 1) / APPEND_COMMIT_WAVES;
				au.next(A.frame + 1, A.frame + 8);
				append_commit_size_field(a); // (wavefront 0: append_commit_wave)
				au.next(A.frame + p, A.frame + total);
				for (uint64_t g = 0; g < groups * APPEND_COMMIT_WAVES; ++g)
					append_commit_copy(a, g);
			}
		}
	}
	memcpy(new_idx, a.idx, ((size_t)keep + k + 1) * 8);
	memcpy(words, a.words, APPEND_WORDS * 4);
	memcpy(buffer, A.frame - GUARD, capacity + 2 * GUARD);
	return result;
}

} // extern "C"
