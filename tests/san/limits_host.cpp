// The size limits of the batch records and of the state pool WITHOUT a GPU (include/lewton_amd.h, "Limits"): the PRODUCT sources
// over stand-ins for the HIP runtime (hip_standins.inc: device memory = calloc), built with ASan + UBSan and -DLW_CHECK_NARROW.
// Prints what the library says; tests/test_host_limits.py holds the expected values (an independent model of the planner's
// offsets in Python integers).  Every stand-in allocation goes through calloc, which this file counts: a refusal must come
// before any of them.
//   usage: limits_host headers.bin
//   headers.bin: u32 len ident | u32 len setup
//   output: "SHAPE ch bs0 bs1 fstride", "MAX n", "REFUSE entry n ptr err allocs" per entry point and size,
//           "RESERVE_OVER rc allocs", "RESERVE n rc allocs", "SLOTS s0 s1 ... allocs", "RESERVE_BELOW rc allocs",
//           "GROW slot allocs", "POOL rc allocs" (device entropy stage: packets whose bytes pass the 32-bit word offsets)
#include "../../include/lewton_amd.h"

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static long g_allocs = 0; // allocations of the HIP stand-ins (hipMalloc, hipHostMalloc, streams, events)
static void *counted_calloc(size_t a, size_t b)
{
	g_allocs++;
	return calloc(a, b);
}
#define calloc(a, b) counted_calloc(a, b)
#include "hip_standins.inc"
#undef calloc

hipError_t lw_launch_rows(const void *, void *, const LwRowSeg *, uint32_t, int, hipStream_t) { return hipSuccess; } // (never reached)

static bool rdv(FILE *f, std::vector<uint8_t> &v)
{
	uint32_t n;
	if (fread(&n, 4, 1, f) != 1)
		return false;
	v.resize(n);
	return n == 0 || fread(v.data(), 1, n, f) == n;
}

int main(int argc, char **argv)
{
	if (argc < 2)
		return 2;
	FILE *f = fopen(argv[1], "rb");
	std::vector<uint8_t> idp, stp;
	if (!f || !rdv(f, idp) || !rdv(f, stp))
		return 2;
	fclose(f);
	int err = 0;
	lw_ident *id = lw_read_header_ident(idp.data(), idp.size(), &err);
	if (!id)
		return 3;
	lw_ident_info info;
	lw_ident_get_info(id, &info);
	lw_setup *setup = lw_read_header_setup(stp.data(), stp.size(), info.audio_channels, info.blocksize_0, info.blocksize_1, &err);
	if (!setup)
		return 3;
	lw_decoder *d = lw_decoder_create(id, setup, 0, &err);
	if (!d)
		return 3;
	printf("SHAPE %u %u %u %u\n", info.audio_channels, info.blocksize_0, info.blocksize_1, lw_setup_floor_stride(setup));
	const size_t max = lw_batch_max_packets(d);
	printf("MAX %zu\n", max);
	const size_t sizes[3] = {max + 1, 2 * max, SIZE_MAX / 64};
	const int dev0 = 0;
	for (size_t n : sizes) {
		long a0 = g_allocs;
		err = 0;
		void *p = lw_batch_create(d, n, LW_FMT_I16_PLANAR, &err);
		printf("REFUSE batch %zu %d %d %ld\n", n, p != nullptr, err, g_allocs - a0);
		a0 = g_allocs, err = 0;
		p = lw_ring_create(d, 2, n, LW_FMT_F32_PLANAR, &err);
		printf("REFUSE ring %zu %d %d %ld\n", n, p != nullptr, err, g_allocs - a0);
		a0 = g_allocs, err = 0;
		p = lw_sharder_create(id, setup, &dev0, 1, n, LW_FMT_I16_PLANAR, &err);
		printf("REFUSE sharder %zu %d %d %ld\n", n, p != nullptr, err, g_allocs - a0);
		a0 = g_allocs, err = 0;
		p = lw_rows_create(d, n, LW_FMT_I16_PLANAR, &err);
		printf("REFUSE rows %zu %d %d %ld\n", n, p != nullptr, err, g_allocs - a0);
	}
	// ---- the state pool
	const size_t slot_limit = ((size_t)1 << 31) - 1; // slots 0 .. 2^31 - 2 (int32_t prev = -(slot + 2))
	long a0 = g_allocs;
	int rc = lw_decoder_reserve_streams(d, slot_limit + 1);
	printf("RESERVE_OVER %d %ld\n", rc, g_allocs - a0);
	a0 = g_allocs;
	rc = lw_decoder_reserve_streams(d, 10);
	printf("RESERVE 10 %d %ld\n", rc, g_allocs - a0);
	a0 = g_allocs;
	std::vector<lw_pwr *> pw;
	printf("SLOTS");
	for (int k = 0; k < 10; k++) {
		pw.push_back(lw_pwr_new(d));
		printf(" %d", lw_debug_pwr_slot(pw.back()));
	}
	printf(" %ld\n", g_allocs - a0);
	a0 = g_allocs;
	rc = lw_decoder_reserve_streams(d, 5);
	printf("RESERVE_BELOW %d %ld\n", rc, g_allocs - a0);
	a0 = g_allocs;
	pw.push_back(lw_pwr_new(d)); // the eleventh handle: the pool grows (doubling), the slot numbers go on
	printf("GROW %d %ld\n", lw_debug_pwr_slot(pw.back()), g_allocs - a0);
	// ---- device entropy stage: packets whose stated lengths pass 2^32 words (only their prologues are read before the refusal)
	if (lw_decoder_supports_device_entropy(d, nullptr) && argc > 2) {
		FILE *g = fopen(argv[2], "rb");
		std::vector<uint8_t> pk;
		if (!g || !rdv(g, pk))
			return 2;
		fclose(g);
		lw_batch *b = lw_batch_create(d, 8, LW_FMT_I16_PLANAR, &err);
		if (!b || lw_batch_set_entropy_on_device(b, 1) != LW_OK)
			return 3;
		lw_packet six[6];
		for (int k = 0; k < 6; k++)
			six[k] = lw_packet{pk.data(), pk.size(), pw[k]};
		rc = lw_batch_entropy(b, six, 6, 1);
		printf("POOL_SMALL %d\n", rc);
		for (int k = 0; k < 6; k++) {
			lw_pwr_reset(pw[k]);
			six[k].len = (size_t)3 << 30; // six "3 GiB" packets: 6 x 0.75 G words pass 2^32 at the sixth
		}
		a0 = g_allocs;
		rc = lw_batch_entropy(b, six, 6, 1);
		printf("POOL %d %ld\n", rc, g_allocs - a0);
		lw_batch_destroy(b);
	}
	for (lw_pwr *p : pw)
		lw_pwr_free(p);
	lw_decoder_destroy(d);
	lw_setup_free(setup);
	lw_ident_free(id);
	return 0;
}
