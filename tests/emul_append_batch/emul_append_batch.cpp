// tests/emul_append_batch/emul_append_batch.cpp -- TEST INFRASTRUCTURE.  What one thread or wavefront of append_batch_plan,
// append_batch_commit_plan, append_batch_index and append_batch_commit does (stenos_amd/csrc/append_batch_codec.h), compiled for
// the host with WV_HOST_EMULATION as tests/emul_append compiles the single call's steps: 64 lanes in lockstep, the threads of a
// grid one after the other.  Decoding the partial last superblocks, stitching and encoding the new ones are the caller's: the
// test hands in whatever "encodings" it likes -- the commit does not parse them.  The host's part between the kernels
// (append_batch_host.cpp: nothing is launched after a status bit or when a frame does not fit; the commit's chunk table) is
// done here as the host does it.  The shipped library never contains or calls this.
#define WV_HOST_EMULATION 1
#include "../../stenos_amd/csrc/append_batch_codec.h"

#include <stdlib.h>
#include <string.h>

#include <vector>

using namespace codec;

enum { GUARD = 64, GUARD_BYTE = 0xA5, DESC = 16 };
// a frame's row of the descriptor table
enum { D_SIZE, D_CAP, D_TOTAL, D_NEW_BYTES, D_FIRST, D_FIRST_NEW, D_ENC_BASE0, D_ENC_BASE1, D_ENC_FIRST, D_KEEP, D_R, D_K, D_K0, D_HEADER, D_START, D_MIS };

namespace {

size_t up64(size_t v) { return (v + 63) & ~(size_t)63; }

struct Audit {
	uint64_t* report;
	const uint8_t* base;
	explicit Audit(uint64_t* r, const uint8_t* b) : report(r), base(b)
	{
#ifdef WV_AUDIT
		wv::AuditState& S = wv::audit_state();
		memset(&S, 0, sizeof S);
		S.lo[wv::WV_AUDIT_LDS] = S.hi[wv::WV_AUDIT_LDS] = base; // (these steps use no LDS through the accessors)
		S.lo[wv::WV_AUDIT_GREAD] = S.hi[wv::WV_AUDIT_GREAD] = base;
		S.lo[wv::WV_AUDIT_GWRITE] = S.hi[wv::WV_AUDIT_GWRITE] = base;
		S.on = true;
#endif
	}
	// what the next thread or wavefront may read: [base, rhi); and write: [wlo, whi)
	void next(const uint8_t* rhi, const uint8_t* wlo, const uint8_t* whi)
	{
#ifdef WV_AUDIT
		wv::AuditState& S = wv::audit_state();
		S.hi[wv::WV_AUDIT_GREAD] = rhi;
		S.lo[wv::WV_AUDIT_GWRITE] = wlo;
		S.hi[wv::WV_AUDIT_GWRITE] = whi;
#else
		(void)rhi;
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
int emul_append_batch_audited(void)
{
#ifdef WV_AUDIT
	return 1;
#else
	return 0;
#endif
}
uint32_t emul_append_batch_plan_threads(void) { return APPEND_PLAN_THREADS; }
uint32_t emul_append_batch_commit_chunk(void) { return APPEND_COMMIT_CHUNK; }

// m frames, described by desc[m][16] (D_*); frames: the old frames, back to back; idx: nidx = S + m entries of the old index in
// the layout of the calls over many frames; enc, enc_off: the encoder's streams and offsets.  One allocation: in front the words,
// the compact tables and both indices (all the planning steps may write), then the frame table, the prefixes, the encoder's
// offsets and streams; LAST the frames' buffers, each between two guards, pre-filled with 0xA5 and shifted off their alignment.
// What the threads and wavefronts of frame f may read ends with that frame's last byte.
// Out: new_idx[nnew], flags[m], ends[m], totals[m], lens[2 m], *status, buffers (GUARD + capacity + GUARD per frame, back to
// back).  Returns 0, (size_t)-4 / -2 for a refused index or stream (INVALID / TRUNCATED), (size_t)-6 if a new frame does not
// fit, (size_t)-3 for no memory.
size_t emul_append_batch(uint32_t m, const uint64_t* desc, const uint8_t* frames, const uint64_t* idx, size_t nidx, const uint8_t* enc, size_t enc_bytes,
			 const uint64_t* enc_off, size_t nenc, int mis_enc, uint64_t* new_idx, size_t nnew, uint32_t* flags, uint64_t* ends, uint64_t* totals,
			 uint64_t* lens, uint32_t* status, uint8_t* buffers, uint64_t* report)
{
	const size_t o_words = 0, o_flags = o_words + up64((size_t)(m + 1) * APPEND_WORDS * 4), o_ends = o_flags + up64(m * 4), o_totals = o_ends + up64(m * 8),
		     o_lens = o_totals + up64(m * 8), o_idx = o_lens + up64(2 * (size_t)m * 8), o_new = o_idx + up64(nidx * 8), w_end = o_new + up64(nnew * 8),
		     o_af = w_end, o_kpre = o_af + up64(m * sizeof(AppendBatchFrame)), o_mpre = o_kpre + up64((m + 1) * 8), o_cpre = o_mpre + up64((m + 1) * 8),
		     o_encoff = o_cpre + up64((2 * (size_t)m + 1) * 8), o_enc = o_encoff + up64(nenc * 8) + 64 + (size_t)mis_enc, o_bufs = up64(o_enc + enc_bytes) + 64;
	std::vector<size_t> o_frame(m);
	size_t bytes = o_bufs;
	for (uint32_t f = 0; f < m; ++f) {
		const uint64_t* d = desc + (size_t)f * DESC;
		o_frame[f] = bytes + GUARD + (size_t)d[D_MIS];
		bytes = up64(o_frame[f] + (size_t)d[D_CAP] + GUARD);
	}
	uint8_t* base = nullptr;
	if (posix_memalign((void**)&base, 64, bytes + 64))
		return (size_t)-3;
	memset(base, 0xEE, o_bufs);
	memset(base + o_bufs, GUARD_BYTE, bytes + 64 - o_bufs);
	memset(base, 0, o_idx); // (words, flags, lengths: zero on entry)
	memcpy(base + o_idx, idx, nidx * 8);
	if (nenc)
		memcpy(base + o_encoff, enc_off, nenc * 8);
	if (enc_bytes)
		memcpy(base + o_enc, enc, enc_bytes);
	AppendBatchFrame* const af = (AppendBatchFrame*)(base + o_af);
	uint64_t* const kpre = (uint64_t*)(base + o_kpre);
	uint64_t* const mpre = (uint64_t*)(base + o_mpre);
	uint64_t* const cpre = (uint64_t*)(base + o_cpre);
	uint64_t K = 0, moved = 0;
	size_t at = 0;
	const uint64_t S = nidx - m;
	for (uint32_t f = 0; f < m; ++f) {
		const uint64_t* d = desc + (size_t)f * DESC;
		AppendBatchFrame& x = af[f];
		memset(&x, 0, sizeof x);
		x.frame = base + o_frame[f];
		memcpy(x.frame, frames + at, (size_t)d[D_SIZE]);
		at += (size_t)d[D_SIZE];
		x.size = d[D_SIZE];
		x.total = d[D_TOTAL];
		x.new_bytes = d[D_NEW_BYTES];
		x.first = d[D_FIRST];
		x.first_new = d[D_FIRST_NEW];
		x.enc_base0 = d[D_ENC_BASE0];
		x.enc_base1 = d[D_ENC_BASE1];
		x.enc_first = d[D_ENC_FIRST];
		x.keep = (uint32_t)d[D_KEEP];
		x.r = (uint32_t)d[D_R];
		x.k = (uint32_t)d[D_K];
		x.k0 = (uint32_t)d[D_K0];
		x.header = (uint32_t)d[D_HEADER];
		x.start = (uint32_t)d[D_START];
		const uint64_t nsb_old = (f + 1 < m ? desc[(size_t)(f + 1) * DESC + D_FIRST] : S) - x.first;
		kpre[f] = K;
		mpre[f] = moved;
		K += x.k;
		moved += x.k ? x.keep : (x.total ? nsb_old + 1 : 0); // (append_batch_host.cpp)
	}
	kpre[m] = K;
	mpre[m] = moved;

	AppendBatchArgs a = AppendBatchArgs();
	a.frames = af;
	a.kpre = kpre;
	a.mpre = mpre;
	a.cpre = cpre;
	a.idx = (uint64_t*)(base + o_idx);
	a.new_idx = (uint64_t*)(base + o_new);
	a.enc = base + o_enc;
	a.enc_off = (const uint64_t*)(base + o_encoff);
	a.words = (uint32_t*)(base + o_words);
	a.flags = (uint32_t*)(base + o_flags);
	a.ends = (uint64_t*)(base + o_ends);
	a.lens = (uint64_t*)(base + o_lens);
	a.totals = (uint64_t*)(base + o_totals);
	a.m = m;
	size_t result;
	{
		Audit au(report, base);
		auto frame_end = [&](uint32_t f) { return (const uint8_t*)af[f].frame + af[f].size; };
		const uint32_t threads = APPEND_PLAN_THREADS;
		for (uint64_t x = 0; x < (m + (uint64_t)threads - 1) / threads * threads; ++x)
			if (x < m) {
				au.next(frame_end((uint32_t)x), base, base + w_end);
				a.words[APPEND_W_STATUS] |= append_batch_plan_thread(a, (uint32_t)x);
			}
		result = status_code(a.words[APPEND_W_STATUS]);
		if (!result) {
			for (uint64_t x = 0; x < (K + threads - 1) / threads * threads; ++x) {
				au.next(x < K ? frame_end(gather_find64(kpre, m, x)) : base, base, base + w_end);
				a.words[APPEND_W_STATUS] |= append_batch_commit_plan_thread(a, x);
			}
			for (uint64_t x = 0; x < (moved + threads - 1) / threads * threads; ++x) {
				au.next(x < moved ? frame_end(gather_find64(mpre, m, x)) : base, base, base + w_end);
				append_batch_index_thread(a, x);
			}
			result = status_code(a.words[APPEND_W_STATUS]);
		}
		if (!result) {
			uint64_t chunks = 0;
			for (uint32_t f = 0; f < m; ++f) {
				cpre[2 * f] = chunks;
				chunks += append_commit_chunks(a.lens[2 * f]);
				cpre[2 * f + 1] = chunks;
				chunks += append_commit_chunks(a.lens[2 * f + 1]);
				if (af[f].k && a.totals[f] > desc[(size_t)f * DESC + D_CAP])
					result = (size_t)-6;
			}
			cpre[2 * (size_t)m] = chunks;
			const uint64_t waves = (chunks + APPEND_COMMIT_WAVES - 1) / APPEND_COMMIT_WAVES * APPEND_COMMIT_WAVES;
			for (uint64_t g = 0; !result && g < waves; ++g) {
				uint32_t s;
				uint64_t c;
				if (!append_batch_commit_chunk_of(a, g, &s, &c)) {
					au.next(base, base, base);
					append_batch_commit_wave(a, g);
					continue;
				}
				const uint32_t f = s >> 1;
				const uint32_t* const w = a.words + (size_t)APPEND_WORDS * (f + 1); // (the driver's own look at p_f: not an access of the kernel's)
				const uint64_t p = (uint64_t)w[APPEND_W_P] | ((uint64_t)w[APPEND_W_P + 1] << 32);
				au.next(frame_end(f), af[f].frame + 1, af[f].frame + 8);
				append_batch_commit_size_field(a, s, c);
				au.next(frame_end(f), af[f].frame + p, af[f].frame + a.totals[f]);
				append_batch_commit_copy(a, s, c);
			}
		}
	}
	memcpy(new_idx, a.new_idx, nnew * 8);
	memcpy(flags, a.flags, m * 4);
	memcpy(ends, a.ends, m * 8);
	memcpy(totals, a.totals, m * 8);
	memcpy(lens, a.lens, 2 * (size_t)m * 8);
	*status = a.words[APPEND_W_STATUS];
	size_t out = 0;
	for (uint32_t f = 0; f < m; ++f) {
		const size_t n = (size_t)desc[(size_t)f * DESC + D_CAP] + 2 * GUARD;
		memcpy(buffers + out, af[f].frame - GUARD, n);
		out += n;
	}
	free(base);
	return result;
}

} // extern "C"
