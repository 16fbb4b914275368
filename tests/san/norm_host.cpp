// Normalising rows WITHOUT a GPU: lw_norm.cpp linked against hip_standins.inc (device memory = calloc), and the KERNEL source
// itself, lw_kernels_norm.hip, compiled for the host (LW_NORM_HOST): the stand-ins for the three launchers below run it workgroup
// by workgroup and wave by wave in the kernels' own order (every wave of a level before the next: the barrier), the 64 lanes'
// entries folded by the contract's adjacent-pair tree in place of the shuffles, so AddressSanitizer sees every load and store the
// kernels make.  Built with -fsanitize=address,undefined; tests/test_host_norm.py drives it.
//   norm_host scalars CENTER SCALE EPS TARGET IN OUT   IN: u64 K, f64 S1[K], f64 S2[K], u64 N[K], f32 P[K];  OUT: f64 m[K], f64 g[K]
//   norm_host create CENTER SCALE SCOPE RESERVED EPS TARGET [DEVICE]   "RC err" (CENTER "null": NULL parameters; the stand-ins
//                                   have ONE device, 0)
//   norm_host refuse CASE           "RC rc", "LAUNCHES n", "LAST n": CASE is one of the refusals of lw_norm_rows (main below)
//   norm_host two                   two calls queued back to back: "ROWS n/fill_end/chunks..." per launch, read at the end
//   norm_host run CENTER SCALE SCOPE EPS TARGET CH F ROWS CAP INPLACE WANTSTATS FILL SHIFT_SRC SHIFT_DST IN OUT
//                                   IN: u64 n[ROWS], u64 fill_to[ROWS], f32 x[ROWS][CH][F][CAP];  OUT: the destination
//                                   (sentinel-filled before the call unless INPLACE), then the stats as f64.  The buffers are
//                                   exact-size, start SHIFT elements behind a 16-byte boundary and have a guarded front.
//                                   "RC rc", "LAUNCHES n"
#include "../../include/lewton_amd.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "hip_standins.inc"
#include "kernel_host.hpp"

#define LW_NORM_HOST 1
#include "../../lewton_amd/csrc/lw_kernels_norm.hip"

static LaunchLog<LwNormRow> g_log;

static void check(const LwNormArgs &a, uint32_t n_rows, bool ok)
{
	g_log.launch(a.rows + a.row0, n_rows);
	if (!a.rows || n_rows == 0 || n_rows > 65535u || (uint64_t)a.plan.scopes * a.plan.scope_lines != (uint64_t)a.ch * a.F || !ok)
		bad("arguments");
}

hipError_t lw_launch_norm_sum(const LwNormArgs &a, uint32_t n_rows, hipStream_t)
{
	check(a, n_rows, !a.plain && a.src && a.part && a.plan.sum_chunks && a.plan.sum_per_wave &&
			(uint64_t)a.plan.sum_tiles * a.plan.sum_per_wave * LW_NM_WAVES >= (uint64_t)a.ch * a.F * a.plan.sum_chunks);
	if (!g_log.run)
		return hipSuccess;
	for (uint32_t bz = 0; bz < n_rows; bz++)
		for (uint32_t bx = 0; bx < a.plan.sum_tiles; bx++)
			for (uint32_t w = 0; w < LW_NM_WAVES; w++)
				lw_nm_sum_wave(a, bx, bz, w, 0);
	return hipSuccess;
}

hipError_t lw_launch_norm_fold(const LwNormArgs &a, uint32_t n_rows, hipStream_t)
{
	check(a, n_rows, a.sc && (a.plan.fold_wave || (a.scratch && a.plan.fold_scratch)));
	if (!g_log.run)
		return hipSuccess;
	for (uint32_t bz = 0; bz < n_rows; bz++) {
		if (a.plan.fold_wave) {
			for (uint32_t bx = 0; bx < (a.plan.scopes + LW_NM_WAVES - 1u) / LW_NM_WAVES; bx++)
				for (uint32_t w = 0; w < LW_NM_WAVES; w++)
					lw_nm_fold_wave(a, bx, bz, w, 0);
			continue;
		}
		for (uint32_t bx = 0; bx < a.plan.scopes; bx++) {
			LwNmLevels v;
			lw_nm_levels(a, bx, bz, v);
			while (v.len > 1) {
				for (uint32_t w = 0; w < LW_NM_WAVES; w++)
					lw_nm_level_wave(v, w, 0);
				lw_nm_level_next(v);
			}
			lw_nm_levels_out(a, bx, bz, v);
		}
	}
	return hipSuccess;
}

hipError_t lw_launch_norm_apply(const LwNormArgs &a, uint32_t n_rows, hipStream_t)
{
	check(a, n_rows, (a.plain || a.sc) && a.plan.tiles && a.plan.per_wave && (uint64_t)a.plan.runs_per_line * a.F == a.plan.runs &&
			(uint64_t)a.plan.tiles * a.plan.per_wave * LW_NM_WAVES >= a.plan.runs);
	if (!g_log.run)
		return hipSuccess;
	for (uint32_t bz = 0; bz < n_rows; bz++)
		for (uint32_t by = 0; by < a.ch; by++)
			for (uint32_t bx = 0; bx < a.plan.tiles; bx++) {
				LwNmTile t;
				lw_nm_tile(a, bx, by, bz, t);
				for (uint32_t tid = 0; tid < LW_NM_THREADS; tid++)
					lw_nm_tile_apply(a, t, by, tid);
			}
	return hipSuccess;
}

static const uint32_t SENT = SENT_DEAD;

static lw_norm *make(const char *center, const char *scale, const char *scope, const char *reserved, const char *eps, const char *target, int *err,
		int device = 0)
{
	lw_norm_params p{atoi(center), atoi(scale), atoi(scope), atoi(reserved), strtod(eps, nullptr), strtod(target, nullptr)};
	return lw_norm_create(device, std::string(center) == "null" ? nullptr : &p, err);
}

int main(int argc, char **argv)
{
	if (argc < 2)
		return 2;
	const std::string mode = argv[1];
	int err = 0;
	if (mode == "scalars" && argc >= 8) {
		lw_norm *nm = make(argv[2], argv[3], "0", "0", argv[4], argv[5], &err);
		if (!nm)
			return 2;
		File in(argv[6], "rb");
		uint64_t k = 0;
		in.get(&k, 1);
		std::vector<double> s1(k), s2(k), m(k), g(k);
		std::vector<uint64_t> cnt(k);
		std::vector<float> pk(k);
		in.get(s1.data(), k), in.get(s2.data(), k), in.get(cnt.data(), k), in.get(pk.data(), k);
		in.close();
		for (uint64_t i = 0; i < k; i++)
			if (lw_norm_scalars(nm, s1[i], s2[i], pk[i], cnt[i], &m[i], &g[i]) != LW_OK)
				return 3;
		if (lw_norm_scalars(nullptr, 0, 0, 0, 1, &m[0], &g[0]) != LW_ERR_NULL_ARG || lw_norm_scalars(nm, 0, 0, 0, 1, nullptr, &g[0]) != LW_ERR_NULL_ARG)
			return 3;
		File out(argv[7], "wb");
		out.put(m.data(), k), out.put(g.data(), k);
		out.close();
		lw_norm_destroy(nm);
		return 0;
	}
	if (mode == "create" && argc >= 8) {
		lw_norm *nm = make(argv[2], argv[3], argv[4], argv[5], argv[6], argv[7], &err, argc >= 9 ? atoi(argv[8]) : 0);
		printf("RC %d\n", err);
		if ((nm == nullptr) != (err != 0))
			return 3;
		lw_norm_destroy(nm);
		return 0;
	}
	if (mode == "run" && argc >= 18) {
		lw_norm *nm = make(argv[2], argv[3], argv[4], "0", argv[5], argv[6], &err);
		if (!nm)
			return 2;
		const int scope = atoi(argv[4]);
		const uint32_t ch = (uint32_t)atoi(argv[7]), F = (uint32_t)atoi(argv[8]);
		const size_t rows = (size_t)atoll(argv[9]), cap = (size_t)atoll(argv[10]);
		const bool inplace = atoi(argv[11]) != 0, want_stats = atoi(argv[12]) != 0, fill = atoi(argv[13]) != 0;
		const size_t n = rows * ch * F * cap, ns = 2 * rows * (scope == LW_NORM_SCOPE_ROW ? 1 : scope == LW_NORM_SCOPE_CHANNEL ? ch : ch * F);
		std::vector<uint64_t> cnt(rows + 1), fill_to(rows + 1);
		const Guarded gs = shifted(4 * n, 4u * (unsigned)atoi(argv[14])), gd = inplace ? gs : shifted(4 * n, 4u * (unsigned)atoi(argv[15]));
		float *src = gs.as<float>(), *dst = gd.as<float>();
		double *stats = (double *)malloc(ns * 8); // exact size: one double beyond it is a report
		if (!stats)
			return 2;
		{
			File in(argv[16], "rb");
			in.get(cnt.data(), rows), in.get(fill_to.data(), rows), in.get(src, n);
		}
		if (!inplace)
			fill32(dst, n, SENT);
		memset(stats, 0xee, ns * 8);
		const int rc = lw_norm_rows(nm, ch, F, src, dst, rows, cap, cnt.data(), fill ? fill_to.data() : nullptr, want_stats ? stats : nullptr, nullptr);
		printf("RC %d\nLAUNCHES %d\n", rc, g_log.launches);
		if (rc == LW_OK && lw_norm_last_launches(nm) != g_log.launches)
			return 3;
		{
			File out(argv[17], "wb");
			out.put(dst, n), out.put(stats, ns);
		}
		if (!guard_intact(gs) || !guard_intact(gd))
			bad("a store in front of a buffer");
		free(gs.base), free(stats);
		if (!inplace)
			free(gd.base);
		lw_norm_destroy(nm);
		return 0;
	}
	// ---- calls on a small fixture: 3 rows of 2 channels of 5 lines, capacity 300, wav2vec 2.0's parameters
	lw_norm_params p{1, LW_NORM_SCALE_STD, LW_NORM_SCOPE_CHANNEL, 0, 1e-7, 1.0};
	lw_norm *nm = lw_norm_create(0, &p, &err);
	if (!nm)
		return 2;
	const size_t cap = 300;
	std::vector<float> buf(3 * 2 * 5 * cap, 0.25f);
	std::vector<double> stats(3 * 2 * 2, 0.0);
	uint64_t cnt[3] = {300, 0, 4}, fill[3] = {300, 3, 2};
	g_log.run = false;
	if (mode == "two") {
		uint64_t cnt_b[3] = {1, 257, 3};
		int rc = lw_norm_rows(nm, 2, 5, buf.data(), buf.data(), 3, cap, cnt, fill, nullptr, nullptr);
		printf("RC %d LAST %d\n", rc, lw_norm_last_launches(nm));
		cnt[0] = 1, fill[1] = 7; // the first call has copied its arrays: the caller's are free
		rc = lw_norm_rows(nm, 2, 5, buf.data(), buf.data(), 3, cap, cnt_b, nullptr, nullptr, nullptr);
		printf("RC %d LAST %d\n", rc, lw_norm_last_launches(nm));
		g_log.print([](const LwNormRow &r) { printf(" %llu/%llu/%u", (unsigned long long)r.n, (unsigned long long)r.fill_end, r.chunks); });
	} else if (mode == "refuse" && argc >= 3) {
		const std::string cs = argv[2];
		uint32_t ch = 2, F = 5;
		const void *s = buf.data();
		void *d = buf.data();
		const uint64_t *n = cnt, *fl = fill;
		double *st = nullptr;
		size_t rows = 3, c = cap;
		lw_norm *h = nm;
		lw_norm *plain = nullptr;
		if (cs == "null_nm")
			h = nullptr;
		else if (cs == "null_n")
			n = nullptr;
		else if (cs == "null_src")
			s = nullptr;
		else if (cs == "null_dst")
			d = nullptr;
		else if (cs == "null_dst_fill_only")
			cnt[0] = cnt[2] = 0, s = nullptr, d = nullptr; // nothing to read, but row 1 is filled to 3
		else if (cs == "n_over")
			cnt[2] = cap + 1; // (the LAST row: every row is checked before anything is queued)
		else if (cs == "fill_over")
			fill[2] = cap + 1;
		else if (cs == "ch0")
			ch = 0;
		else if (cs == "ch256")
			ch = 256;
		else if (cs == "f0")
			F = 0;
		else if (cs == "f65536")
			F = 65536;
		else if (cs == "too_large")
			c = (size_t)1 << 62;
		else if (cs == "too_many_chunks")
			c = (size_t)1 << 40, F = 65535, cnt[0] = c, ch = 1; // 2^32 chunks and more in a row
		else if (cs == "too_many_runs")
			c = (size_t)1 << 40, F = 65535, cnt[0] = 0, fill[0] = c, ch = 1; // ... and of runs to fill
		else if (cs == "ok_nothing")
			cnt[0] = cnt[2] = 0, fl = nullptr, s = nullptr, d = nullptr; // no element, no fill: accepted, nothing queued
		else if (cs == "ok_no_rows")
			rows = 0, n = nullptr;
		else if (cs == "ok_stats")
			st = stats.data();
		else if (cs == "ok_stats_of_nothing")
			cnt[0] = cnt[2] = 0, fl = nullptr, s = nullptr, d = nullptr, st = stats.data(); // (m, g) of empty scopes are still owed
		else if (cs == "ok_fill_only")
			cnt[0] = cnt[2] = 0, s = nullptr; // no sums: the fold's (+0.0, 1.0), and the fill
		else if (cs == "ok_plain" || cs == "ok_plain_stats") {
			lw_norm_params q{0, LW_NORM_SCALE_NONE, LW_NORM_SCOPE_LINE, 0, 0.0, 0.0};
			h = plain = lw_norm_create(0, &q, &err);
			if (!h)
				return 2;
			if (cs == "ok_plain_stats")
				stats.resize(3 * 2 * 5 * 2), st = stats.data();
		} else if (cs != "ok")
			return 2;
		const int rc = lw_norm_rows(h, ch, F, s, d, rows, c, n, fl, st, nullptr);
		printf("RC %d\nLAUNCHES %d\nLAST %d\n", rc, g_log.launches, lw_norm_last_launches(plain ? plain : nm));
		lw_norm_destroy(plain);
	} else {
		return 2;
	}
	lw_norm_destroy(nm);
	return 0;
}
