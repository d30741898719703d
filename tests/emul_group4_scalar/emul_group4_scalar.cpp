// tests/emul_group4_scalar/emul_group4_scalar.cpp -- TEST INFRASTRUCTURE.  Runs of full int32 blocks through encode_run (what one
// wave of the fused encoder does, superblock_codec.h) in the host emulation of tests/emul, as a program of its own: it is built
// plain and with the address and undefined-behaviour sanitizers (tests/test_group4_scalar_cpu.py).  The input is a malloc of
// exactly its size, the LDS one of exactly the layout's, so a read or a write outside either is reported.
// usage: emul_group4_scalar <input file> <output file> <blocks> [<blocks> ...]
//   the input file holds the runs back to back; one line per run: "<bytes> <groups of four> <packed emissions> <groups whose scan
//   against the expected planes was accepted>", the streams go to the output file back to back
// A run begins like a wave's first: it tries a group, and expects no planes.
#define WV_HOST_EMULATION 1
#define WV_PREDICATE_BRANCHES 1 // (the encoders' form of the shared copy helpers, as tests/emul's libstenos_emul_enc.so)
#include "../../stenos_amd/csrc/superblock_codec.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

using namespace codec;

int main(int argc, char** argv)
{
	if (argc < 4)
		return 2;
	FILE* in = fopen(argv[1], "rb");
	FILE* out = fopen(argv[2], "wb");
	if (!in || !out)
		return 2;
	const uint32_t T = 4;
	const Layout L = make_layout(T, true);
	for (int a = 3; a < argc; ++a) {
		const uint32_t nblocks = (uint32_t)atoi(argv[a]);
		const size_t bytes = (size_t)nblocks * 256 * T;
		uint8_t* src = (uint8_t*)malloc(bytes);
		if (!src || fread(src, 1, bytes, in) != bytes)
			return 3;
		uint8_t* lds = (uint8_t*)malloc(L.total);
		memset(lds, 0xCD, L.total); // (LDS is not zero-initialised on the device either)
		const size_t cap = (size_t)nblocks * max_block_bytes(T) + 16;
		uint8_t* stage = nullptr;
		if (posix_memalign((void**)&stage, 16, cap))
			return 3;
		memset(stage, 0xCD, cap);
		const uint64_t g4 = emul_group4_count(), pk = emul_group4_packed_count(), ex = emul_group4_expected_count();
		uint32_t hint = StreamSink::GROUP_TRY;
		const uint32_t n = encode_run(lds, L, T, src, nblocks, stage, true, NoPassHook(), nullptr, &hint);
		printf("%u %llu %llu %llu\n", n, (unsigned long long)(emul_group4_count() - g4), (unsigned long long)(emul_group4_packed_count() - pk),
		       (unsigned long long)(emul_group4_expected_count() - ex));
		if (fwrite(stage, 1, n, out) != n)
			return 3;
		free(stage);
		free(lds);
		free(src);
	}
	fclose(in);
	fclose(out);
	return 0;
}
