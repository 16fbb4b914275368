// The chunk load of four floats WITHOUT a GPU.  It stayed one copy per kernel file (lw_nm_chunk_lane in lw_kernels_norm.hip,
// lw_vd_chunk_lane in lw_kernels_vad.hip: sharing it changed either kernel's code), so both copies are held to one matrix here:
// n in {0, 1, 3, 4, 5, 255, 256, 257}, the line 0, 4, 8 and 12 bytes behind a 16-byte boundary, every lane of chunks 0 and 1.
// The line is a buffer of exactly n floats with a guarded front, so a read at or beyond n, or in front of the line, is
// AddressSanitizer's to report; what a lane returns must be what the elements give, +0.0 at and beyond n.  Built with
// -fsanitize=address,undefined; tests/test_host_lanes.py drives it.  No HIP code, no GPU.
//   chunk_host          "OK chunk n"
#define KERNEL_HOST_NO_HIP_OK 1
#define LW_KERNEL_HOST 1
#include "../../lewton_amd/csrc/lw_kernels_norm.hip"
#include "../../lewton_amd/csrc/lw_kernels_vad.hip"

#include "kernel_host.hpp"

static uint64_t bits_of(double d)
{
	uint64_t u;
	memcpy(&u, &d, 8);
	return u;
}

int main()
{
	const uint64_t ns[] = {0, 1, 3, 4, 5, 255, 256, 257};
	long cases = 0;
	for (unsigned off = 0; off < 16; off += 4)
		for (uint64_t n : ns) {
			const Guarded g = shifted((size_t)n * 4, off);
			float *x = g.as<float>();
			for (uint64_t i = 0; i < n; i++) // every window of four has sums and a peak of its own; the signs alternate
				x[i] = (i & 1 ? -1.0f : 1.0f) * (1.5f + (float)i * (float)i * 0.25f);
			LwNormArgs a{};
			a.src = x;
			for (uint32_t c = 0; c < 2; c++)
				for (uint32_t lane = 0; lane < 64; lane++) {
					double d[4];
					uint32_t pk = 0;
					for (int j = 0; j < 4; j++) {
						const uint64_t e = (uint64_t)c * 256u + lane * 4u + (uint64_t)j;
						const float v = e < n ? x[e] : 0.0f;
						uint32_t b;
						memcpy(&b, &v, 4);
						b &= 0x7fffffffu, pk = b > pk ? b : pk;
						d[j] = (double)v;
					}
					const double s1 = ((d[0] + d[1]) + d[2]) + d[3], s2 = ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) + d[3] * d[3];
					const LwNormTriple t = lw_nm_chunk_lane(a, 0u, n, c, lane);
					if (bits_of(t.s1) != bits_of(s1) || bits_of(t.s2) != bits_of(s2) || t.pk != pk)
						bad("norm: off %u n %llu chunk %u lane %u: %a %a %08x, the elements give %a %a %08x", off, (unsigned long long)n, c, lane, t.s1, t.s2,
								t.pk, s1, s2, pk);
					const double v = lw_vd_chunk_lane(x, 0u, n, c, lane);
					if (bits_of(v) != bits_of(s1))
						bad("vad: off %u n %llu chunk %u lane %u: %a, the elements give %a", off, (unsigned long long)n, c, lane, v, s1);
					cases++;
				}
			if (!guard_intact(g))
				bad("a store in front of the line");
			free(g.base);
		}
	printf("OK chunk %ld\n", cases);
	return 0;
}
