// The library's random numbers: Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) and
// two bounded draws, in plain C++ on unsigned integers, ONE source for the host and for the kernels.  A counter-based generator
// has no state: lw_philox(counter, key) is a pure function of its six words, so what is drawn for an item depends on the item's
// own numbers alone -- not on the batch it is in, the grid that works on it or the calls that went before.  No floats: the host,
// numpy and the GPU agree on every bit.  Known answers (Random123's): tests/test_specaug_model.py, tests/san/specaug_host.cpp.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define LW_RNG_HD __host__ __device__ static inline
#else
#define LW_RNG_HD static inline
#endif

#define LW_PHILOX_M0 0xD2511F53u // the multiplier on counter word 0
#define LW_PHILOX_M1 0xCD9E8D57u // ... on counter word 2
#define LW_PHILOX_W0 0x9E3779B9u // added to key word 0 before every round but the first
#define LW_PHILOX_W1 0xBB67AE85u // ... to key word 1
#define LW_PHILOX_ROUNDS 10

// x[0 .. 3] = Philox4x32-10 of the counter c[0 .. 3] under the key k[0 .. 1].  One round maps (c0, c1, c2, c3) to
// (hi(M1 * c2) ^ c1 ^ k0, lo(M1 * c2), hi(M0 * c0) ^ c3 ^ k1, lo(M0 * c0))
LW_RNG_HD void lw_philox(const uint32_t c[4], const uint32_t k[2], uint32_t x[4])
{
	uint32_t c0 = c[0], c1 = c[1], c2 = c[2], c3 = c[3], k0 = k[0], k1 = k[1];
	for (int r = 0; r < LW_PHILOX_ROUNDS; r++) {
		if (r)
			k0 += LW_PHILOX_W0, k1 += LW_PHILOX_W1;
		const uint64_t p0 = (uint64_t)LW_PHILOX_M0 * c0, p1 = (uint64_t)LW_PHILOX_M1 * c2;
		const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
		c0 = n0, c1 = (uint32_t)p1, c2 = n2, c3 = (uint32_t)p0;
	}
	x[0] = c0, x[1] = c1, x[2] = c2, x[3] = c3;
}

// ---- bounded draws: multiply-high, no rejection, so ONE draw per number whatever n is.  The value is in [0, n) for n > 0 (0 for
// n == 0) and no value is more likely than another by more than one part in 2^32 / n (2^64 / n): the bias is at most n / 2^32
// for lw_below32 and n / 2^64 for lw_below64
LW_RNG_HD uint32_t lw_below32(uint32_t x, uint32_t n)
{
	return (uint32_t)(((uint64_t)x * n) >> 32);
}

LW_RNG_HD uint64_t lw_below64(uint64_t x, uint64_t n) // the high 64 bits of the 128-bit product
{
#if defined(__HIP_DEVICE_COMPILE__)
	return __umul64hi(x, n);
#else
	return (uint64_t)(((unsigned __int128)x * n) >> 64);
#endif
}
