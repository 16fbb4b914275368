// The complex output of the spectral frames (LW_SPEC_OUT_COMPLEX, k_spec_complex) WITHOUT a GPU: lw_spec.cpp linked against
// hip_standins.inc, and the kernel source, lw_kernels_spec.hip, compiled for the host (LW_SPEC_HOST, per-lane fmaf chains): the
// stand-in for lw_launch_spec below runs the kernel body's phases in the kernel's own order for BOTH outputs, lane by lane, with an
// LDS buffer of exactly the kernel's size and exact-size buffers, under AddressSanitizer.  tests/test_host_spec_complex.py drives it.
//   spec_complex_host create NFFT WIN HOP WINDOW CENTER NMELS DC ENERGY OUTPUT    "RC err" and "F features" (lw_spec_create_ex)
//   spec_complex_host run NFFT WIN HOP WINDOW CENTER PAD OUTPUT IN OUT BASIS      one row (raw f32 IN) through lw_spec_create_ex with
//        output OUTPUT (-1: through lw_spec_create, the entry point without the field) and pad mode PAD, [F][frames] raw f32 into
//        OUT in a sentinel-filled exact-size destination of one frame more, the basis into BASIS: "RC rc", "F features frames"
#include "../../include/lewton_amd.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "hip_standins.inc"
#include "kernel_host.hpp"

#define LW_SPEC_HOST 1
#include "../../lewton_amd/csrc/lw_kernels_spec.hip"

static void run_tile(const LwSpecArgs &a, uint32_t bx, uint32_t by, uint32_t bz)
{
	LwSpTile t;
	if (!lw_sp_tile(a, bx, by, bz, t))
		return;
	float *lds = (float *)malloc((size_t)LW_SP_LDS_FLOATS * 4);
	for (size_t i = 0; i < LW_SP_LDS_FLOATS; i++)
		lds[i] = NAN;
	std::vector<LwSpLane> st(LW_SP_THREADS);
	const uint32_t T = LW_SP_THREADS;
	for (uint32_t pass = 0; pass < a.passes; pass++) {
		for (uint32_t tid = 0; tid < T; tid++)
			lw_sp_zero_acc(st[tid]);
		for (uint32_t kt = 0; kt < a.k_pad / LW_SP_KT; kt++) {
			for (uint32_t tid = 0; tid < T; tid++)
				lw_sp_stage(a, t, pass, kt, tid, lds);
			for (uint32_t tid = 0; tid < T; tid++)
				lw_sp_mma<LW_SP_ROUTE_FMA>(a, pass, tid, lds, st[tid]);
		}
		if (a.output) { // the kernel body's OUT = 1 branch, a barrier between any two of these
			for (uint32_t tid = 0; tid < T; tid++)
				lw_sp_part<0>(a, pass, tid, lds, st[tid]);
			for (uint32_t tid = 0; tid < T; tid++)
				lw_sp_store_lines(a, t, pass, tid, lds, 0u);
			for (uint32_t tid = 0; tid < T; tid++)
				lw_sp_part<1>(a, pass, tid, lds, st[tid]);
			for (uint32_t tid = 0; tid < T; tid++)
				lw_sp_store_lines(a, t, pass, tid, lds, a.bins);
			continue;
		}
		for (uint32_t tid = 0; tid < T; tid++)
			lw_sp_power(a, pass, tid, lds, st[tid]);
		for (uint32_t tid = 0; tid < T; tid++)
			lw_sp_store_power(a, t, pass, tid, lds);
	}
	free(lds);
}

hipError_t lw_launch_spec(const LwSpecArgs &a, int route, uint32_t tiles, uint32_t ch, uint32_t n_rows, hipStream_t)
{
	if (!a.rows || !a.basis || a.n_mels || a.remove_dc || a.energy || a.output > 1u || (route != 0 && route != 1) || a.k_pad % LW_SP_KT)
		bad("arguments");
	for (uint32_t bz = 0; bz < n_rows; bz++)
		for (uint32_t by = 0; by < ch; by++)
			for (uint32_t bx = 0; bx < tiles; bx++)
				run_tile(a, bx, by, bz);
	return hipSuccess;
}

static uint32_t u32(const char *s)
{
	return (uint32_t)strtoul(s, nullptr, 10);
}

int main(int argc, char **argv)
{
	if (argc < 2)
		return 2;
	const std::string mode = argv[1];
	int err = 0;
	if (mode == "create" && argc >= 11) {
		std::vector<float> fb((size_t)u32(argv[7]) * 2048 + 1, 0.5f);
		lw_spec_params p{};
		p.n_fft = u32(argv[2]), p.win_length = u32(argv[3]), p.hop = u32(argv[4]), p.window = atoi(argv[5]), p.center = atoi(argv[6]);
		p.n_mels = u32(argv[7]), p.fb = p.n_mels ? fb.data() : nullptr, p.remove_dc = atoi(argv[8]), p.energy = atoi(argv[9]), p.output = atoi(argv[10]);
		p.scale = 1.0;
		lw_spec *sp = lw_spec_create_ex(0, &p, &err);
		printf("RC %d\nF %u\n", err, lw_spec_features(sp));
		if ((sp == nullptr) != (err != 0))
			return 3;
		lw_spec_destroy(sp);
		return 0;
	}
	if (mode != "run" || argc < 12)
		return 2;
	const int output = atoi(argv[8]), pad = atoi(argv[7]);
	lw_spec *sp;
	if (output < 0) {
		sp = lw_spec_create(0, u32(argv[2]), u32(argv[3]), u32(argv[4]), atoi(argv[5]), atoi(argv[6]), 0, nullptr, &err);
	} else {
		lw_spec_params p{};
		p.n_fft = u32(argv[2]), p.win_length = u32(argv[3]), p.hop = u32(argv[4]), p.window = atoi(argv[5]), p.center = atoi(argv[6]);
		p.scale = 1.0, p.output = output;
		sp = lw_spec_create_ex(0, &p, &err);
	}
	if (!sp || lw_spec_set_pad_mode(sp, pad) != LW_OK || lw_spec_set_route(sp, LW_SP_ROUTE_FMA) != LW_OK)
		return 2;
	const std::vector<float> in = slurp_f32(argv[9]);
	const size_t n = in.size();
	float *x = (float *)malloc(n ? n * 4 : 4); // an exact-size source
	std::copy(in.begin(), in.end(), x);
	const uint64_t len = n, frames = lw_spec_frames(sp, len);
	const uint32_t F = lw_spec_features(sp);
	const size_t fcap = frames + 1, dn = (size_t)F * fcap;
	float *y = (float *)malloc(dn * 4); // ... and destination
	fill32(y, dn, SENT_ABC);
	const int rc = lw_spec_rows(sp, LW_FMT_F32_PLANAR, 1, x, 1, n, &len, nullptr, y, 1, fcap, nullptr);
	printf("RC %d\nF %u %llu\n", rc, F, (unsigned long long)frames);
	File(argv[10], "wb").put(y, dn);
	std::vector<float> b(lw_spec_basis(sp, nullptr));
	lw_spec_basis(sp, b.data());
	File(argv[11], "wb").put(b.data(), b.size());
	free(x), free(y);
	lw_spec_destroy(sp);
	return 0;
}
