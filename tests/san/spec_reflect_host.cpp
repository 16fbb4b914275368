// Reflect-padded spectral frames WITHOUT a GPU (LW_SPEC_PAD_REFLECT; include/lewton_amd.h "spectral frames of rows", reflect):
// lw_spec.cpp linked against hip_standins.inc and the kernel source, lw_kernels_spec.hip, compiled for the host (LW_SPEC_HOST: the
// route with per-lane fmaf chains) and run workgroup by workgroup, lane by lane, phase by phase, as tests/san/spec_host.cpp does.
// The kernel is instantiated per pad mode on the device (k_spec<ROUTE, PAD>); here lw_sp_stage runs with LW_SP_PAD_ARGS, the
// run-time test of a.pad_mode in front of the same lw_sp_reflect and the same clamped load: this program covers the reflected
// indices and the loads, not the device's two instantiations, which tests/rows_feat_gpu_cases.py compares bit for bit.
// Built with -fsanitize=address,undefined; tests/test_host_spec_reflect.py drives it.
//   spec_reflect_host index LEN I...                    "X i r": where x[i] of a row of LEN samples is read (lw_sp_reflect)
//   spec_reflect_host mode CENTER MODE                  "RC rc MODE m": lw_spec_set_pad_mode on a (400, 400, 160) object, and the
//                                                       mode it is in afterwards (CENTER "null": a NULL object)
//   spec_reflect_host refuse NFFT WIN HOP LEN           "RC rc", "LAUNCHES n": one row of LEN samples under reflect
//   spec_reflect_host basis NFFT WIN HOP WINDOW FILE    the basis [2][WIN][B] as raw f32 into FILE
//   spec_reflect_host run NFFT WIN HOP WINDOW MODES IN OUT   the power spectrum of one row (raw f32 IN, exact size) as [B][frames]
//                                                       raw f32 into OUT; MODES is a string of 0 / 1, one call per letter in that
//                                                       pad mode on ONE object, the last call's output is kept
#include "../../include/lewton_amd.h"

#include <algorithm>
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

static LaunchLog<LwSpecRow> g_log;

static void run_tile(const LwSpecArgs &a, uint32_t bx, uint32_t by, uint32_t bz)
{
	LwSpTile t;
	if (!lw_sp_tile(a, bx, by, bz, t))
		return;
	float *lds = (float *)malloc((size_t)LW_SP_LDS_FLOATS * 4); // exactly the kernel's size
	for (size_t i = 0; i < LW_SP_LDS_FLOATS; i++)
		lds[i] = NAN;
	std::vector<LwSpLane> st(LW_SP_THREADS);
	const uint32_t T = LW_SP_THREADS;
	for (uint32_t tid = 0; tid < T; tid++)
		lw_sp_zero_mel(st[tid]);
	for (uint32_t pass = 0; pass < a.passes; pass++) {
		for (uint32_t tid = 0; tid < T; tid++)
			lw_sp_zero_acc(st[tid]);
		for (uint32_t kt = 0; kt < a.k_pad / LW_SP_KT; kt++) {
			for (uint32_t tid = 0; tid < T; tid++)
				lw_sp_stage(a, t, pass, kt, tid, lds);
			for (uint32_t tid = 0; tid < T; tid++)
				lw_sp_mma<LW_SP_ROUTE_FMA>(a, pass, tid, lds, st[tid]);
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
	g_log.launch();
	if (!a.rows || !a.basis || a.n_mels || route != LW_SP_ROUTE_FMA || ch == 0 || n_rows > 65535u || a.k_pad % LW_SP_KT)
		bad("arguments");
	for (uint32_t bz = 0; bz < n_rows; bz++)
		for (uint32_t by = 0; by < ch; by++)
			for (uint32_t bx = 0; bx < tiles; bx++)
				run_tile(a, bx, by, bz);
	return hipSuccess;
}

int main(int argc, char **argv)
{
	if (argc < 2)
		return 2;
	const std::string mode = argv[1];
	int err = 0;
	if (mode == "index" && argc >= 4) {
		LwSpTile t{};
		t.len = strtoull(argv[2], nullptr, 10);
		for (int i = 3; i < argc; i++) {
			const int64_t at = strtoll(argv[i], nullptr, 10);
			printf("X %lld %lld\n", (long long)at, (long long)lw_sp_reflect(t, at));
		}
		return 0;
	}
	if (mode == "mode" && argc >= 4) {
		const bool null = std::string(argv[2]) == "null";
		lw_spec *sp = null ? nullptr : lw_spec_create(0, 400, 400, 160, LW_SPEC_HANN, atoi(argv[2]), 0, nullptr, &err);
		if (!null && (!sp || lw_spec_pad_mode(sp) != LW_SPEC_PAD_ZERO))
			return 3;
		const int rc = lw_spec_set_pad_mode(sp, atoi(argv[3]));
		printf("RC %d MODE %d\n", rc, lw_spec_pad_mode(sp));
		lw_spec_destroy(sp);
		return 0;
	}
	if (argc < 6)
		return 2;
	const uint32_t n_fft = (uint32_t)strtoul(argv[2], nullptr, 10), win = (uint32_t)strtoul(argv[3], nullptr, 10), hop = (uint32_t)strtoul(argv[4], nullptr, 10);
	if (mode == "refuse") {
		lw_spec *sp = lw_spec_create(0, n_fft, win, hop, LW_SPEC_HANN, 1, 0, nullptr, &err);
		if (!sp || lw_spec_set_pad_mode(sp, LW_SPEC_PAD_REFLECT) != LW_OK || lw_spec_set_route(sp, LW_SP_ROUTE_FMA) != LW_OK)
			return 3;
		const uint64_t len[2] = {(uint64_t)n_fft * 4, strtoull(argv[5], nullptr, 10)}; // (the LAST row is the short one)
		const size_t cap = (size_t)std::max(len[0], len[1]), fcap = (size_t)lw_spec_frames(sp, cap);
		std::vector<float> x(2 * cap, 0.5f), y(2 * (size_t)lw_spec_bins(sp) * fcap, 0.0f);
		const int rc = lw_spec_rows(sp, LW_FMT_F32_PLANAR, 1, x.data(), 2, cap, len, nullptr, y.data(), 2, fcap, nullptr);
		printf("RC %d\nLAUNCHES %d\n", rc, g_log.launches);
		lw_spec_destroy(sp);
		return 0;
	}
	if (mode == "basis" && argc >= 7) {
		lw_spec *sp = lw_spec_create(0, n_fft, win, hop, atoi(argv[5]), 1, 0, nullptr, &err);
		if (!sp)
			return 3;
		std::vector<float> b(lw_spec_basis(sp, nullptr));
		if (lw_spec_basis(sp, b.data()) != b.size())
			return 2;
		File(argv[6], "wb").put(b.data(), b.size());
		lw_spec_destroy(sp);
		return 0;
	}
	if (mode == "run" && argc >= 9) {
		lw_spec *sp = lw_spec_create(0, n_fft, win, hop, atoi(argv[5]), 1, 0, nullptr, &err);
		if (!sp || lw_spec_set_route(sp, LW_SP_ROUTE_FMA) != LW_OK)
			return 3;
		const std::vector<float> in = slurp_f32(argv[7]);
		const size_t n = in.size();
		float *x = (float *)malloc(n ? n * 4 : 4); // exact size: a reflected index outside [0, len) is an ASan report
		std::copy(in.begin(), in.end(), x);
		const uint64_t len = n, frames = lw_spec_frames(sp, len);
		const size_t B = lw_spec_bins(sp);
		float *y = (float *)malloc(B * frames ? B * frames * 4 : 4);
		int rc = LW_OK;
		for (const char *m = argv[6]; *m && rc == LW_OK; m++) {
			if (lw_spec_set_pad_mode(sp, *m - '0') != LW_OK || lw_spec_pad_mode(sp) != *m - '0')
				return 3;
			for (size_t i = 0; i < B * frames; i++)
				y[i] = NAN;
			rc = lw_spec_rows(sp, LW_FMT_F32_PLANAR, 1, x, 1, n, &len, nullptr, y, 1, frames, nullptr);
		}
		printf("RC %d\nF %zu %llu\n", rc, B, (unsigned long long)frames);
		File(argv[8], "wb").put(y, B * frames);
		free(x), free(y);
		lw_spec_destroy(sp);
		return 0;
	}
	return 2;
}
