// Finishing feature rows WITHOUT a GPU: lw_feat.cpp linked against hip_standins.inc (device memory = calloc), and the KERNEL
// source itself, lw_kernels_feat.hip, compiled for the host (LW_FEAT_HOST): the stand-ins for the two launchers below run it
// workgroup by workgroup and lane by lane, phase by phase in the kernels' own order (every lane of a phase before the next: the
// barrier), the workgroup's maximum of the lanes' keys taken here in place of the shuffles, so AddressSanitizer sees every load
// and store the kernels make.  Built with -fsanitize=address,undefined; tests/test_host_feat.py drives it.
//   feat_host log KIND IN OUT       lw_feat_log of every f32 of IN (raw) into OUT
//   feat_host create LOG SCOPE FLOOR TOP ADD MUL [DEVICE]   "RC err" (LOG "null": NULL parameters; the stand-ins have ONE device, 0)
//   feat_host refuse CASE           "RC rc", "LAUNCHES n", "LAST n": CASE is one of the refusals of lw_feat_rows (main below)
//   feat_host two                   two calls queued back to back: "ROWS n_frames/fill_end..." per launch, read at the end
//   feat_host run LOG SCOPE FLOOR TOP ADD MUL CH F ROWS CAP INPLACE WANTMAX FILL SHIFT_SRC SHIFT_DST IN OUT
//                                   IN: u64 n_frames[ROWS], u64 fill_to[ROWS], f32 x[ROWS][CH][F][CAP];  OUT: the destination
//                                   (sentinel-filled before the call unless INPLACE), then M.  The buffers are exact-size, start
//                                   SHIFT elements behind a 16-byte boundary and have a guarded front.  "RC rc", "LAUNCHES n"
#include "../../include/lewton_amd.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "hip_standins.inc"
#include "kernel_host.hpp"

#define LW_FEAT_HOST 1
#include "../../lewton_amd/csrc/lw_kernels_feat.hip"

static LaunchLog<LwFeatRow> g_log;

static void check(const LwFeatArgs &a, uint32_t n_rows, bool fin)
{
	g_log.launch(a.rows + a.row0, n_rows);
	if (!a.rows || n_rows == 0 || n_rows > 65535u || !a.plan.tiles || !a.plan.per_wave || (uint64_t)a.plan.runs_per_line * a.F != a.plan.runs ||
			(uint64_t)a.plan.tiles * a.plan.per_wave * LW_FT_WAVES < a.plan.runs || (!a.final && !a.part) || (fin && a.final))
		bad("arguments");
}

static int32_t wg_max(const std::vector<int32_t> &keys)
{
	int32_t m = keys[0];
	for (int32_t k : keys)
		m = k > m ? k : m;
	return m;
}

hipError_t lw_launch_feat_log(const LwFeatArgs &a, uint32_t n_rows, hipStream_t)
{
	check(a, n_rows, false);
	if (!g_log.run)
		return hipSuccess;
	std::vector<int32_t> keys(LW_FT_THREADS);
	for (uint32_t bz = 0; bz < n_rows; bz++)
		for (uint32_t by = 0; by < a.ch; by++)
			for (uint32_t bx = 0; bx < a.plan.tiles; bx++) {
				LwFtTile t;
				lw_ft_tile(a, bx, by, bz, t);
				for (uint32_t tid = 0; tid < LW_FT_THREADS; tid++)
					keys[tid] = lw_ft_tile_log(a, t, tid);
				if (!a.final)
					lw_ft_tile_part(a, t, bx, wg_max(keys));
			}
	return hipSuccess;
}

hipError_t lw_launch_feat_fin(const LwFeatArgs &a, uint32_t n_rows, hipStream_t)
{
	check(a, n_rows, true);
	if (!g_log.run)
		return hipSuccess;
	std::vector<int32_t> keys(LW_FT_THREADS);
	for (uint32_t bz = 0; bz < n_rows; bz++)
		for (uint32_t by = 0; by < a.ch; by++)
			for (uint32_t bx = 0; bx < a.plan.tiles; bx++) {
				LwFtTile t;
				lw_ft_tile(a, bx, by, bz, t);
				for (uint32_t tid = 0; tid < LW_FT_THREADS; tid++)
					keys[tid] = lw_ft_scope_key(a, t, by, tid);
				const int32_t m = wg_max(keys);
				for (uint32_t tid = 0; tid < LW_FT_THREADS; tid++)
					lw_ft_tile_fin(a, t, bx, by, bz, tid, m);
			}
	return hipSuccess;
}

static const uint32_t SENT = SENT_DEAD;

static lw_feat *make(char **v, int *err, int device = 0)
{
	lw_feat_params p{atoi(v[0]), atoi(v[1]), strtof(v[2], nullptr), strtof(v[3], nullptr), strtof(v[4], nullptr), strtof(v[5], nullptr)};
	return lw_feat_create(device, std::string(v[0]) == "null" ? nullptr : &p, err);
}

int main(int argc, char **argv)
{
	if (argc < 2)
		return 2;
	const std::string mode = argv[1];
	int err = 0;
	if (mode == "log" && argc >= 5) {
		lw_feat_params p{atoi(argv[2]), 0, 1e-10f, 8.0f, 4.0f, 0.25f};
		lw_feat *ft = lw_feat_create(0, &p, &err);
		if (!ft)
			return 2;
		std::vector<float> x = slurp_f32(argv[3]);
		for (auto &v : x)
			v = lw_feat_log(ft, v);
		File(argv[4], "wb").put(x.data(), x.size());
		lw_feat_destroy(ft);
		return 0;
	}
	if (mode == "create" && argc >= 8) {
		lw_feat *ft = make(argv + 2, &err, argc >= 9 ? atoi(argv[8]) : 0);
		printf("RC %d\n", err);
		if ((ft == nullptr) != (err != 0))
			return 3;
		lw_feat_destroy(ft);
		return 0;
	}
	if (mode == "run" && argc >= 19) {
		lw_feat *ft = make(argv + 2, &err);
		if (!ft)
			return 2;
		const uint32_t ch = (uint32_t)atoi(argv[8]), F = (uint32_t)atoi(argv[9]);
		const size_t rows = (size_t)atoll(argv[10]), cap = (size_t)atoll(argv[11]);
		const bool inplace = atoi(argv[12]) != 0, want_max = atoi(argv[13]) != 0, fill = atoi(argv[14]) != 0;
		const int scope = atoi(argv[3]);
		const size_t n = rows * ch * F * cap, nm = rows * (scope == LW_FEAT_SCOPE_CHANNEL ? ch : 1);
		std::vector<uint64_t> nf(rows + 1), ft_to(rows + 1);
		const Guarded gs = shifted(4 * n, 4u * (unsigned)atoi(argv[15])), gd = inplace ? gs : shifted(4 * n, 4u * (unsigned)atoi(argv[16])), gm = shifted(4 * nm, 0);
		float *src = gs.as<float>(), *dst = gd.as<float>(), *mx = gm.as<float>();
		{
			File in(argv[17], "rb");
			in.get(nf.data(), rows), in.get(ft_to.data(), rows), in.get(src, n);
		}
		if (!inplace)
			fill32(dst, n, SENT);
		fill32(mx, nm, SENT);
		const int rc = lw_feat_rows(ft, ch, F, src, dst, rows, cap, nf.data(), fill ? ft_to.data() : nullptr, want_max ? mx : nullptr, nullptr);
		printf("RC %d\nLAUNCHES %d\n", rc, g_log.launches);
		if (rc == LW_OK && lw_feat_last_launches(ft) != g_log.launches)
			return 3;
		{
			File out(argv[18], "wb");
			out.put(dst, n), out.put(mx, nm);
		}
		if (!guard_intact(gs) || !guard_intact(gd) || !guard_intact(gm))
			bad("a store in front of a buffer");
		free(gs.base), free(gm.base);
		if (!inplace)
			free(gd.base);
		lw_feat_destroy(ft);
		return 0;
	}
	// ---- calls on a small fixture: 3 rows of 2 channels of 5 lines, capacity 9, Whisper's parameters
	lw_feat_params p{LW_FEAT_LOG_LOG10, LW_FEAT_SCOPE_ROW, 1e-10f, 8.0f, 4.0f, 0.25f};
	lw_feat *ft = lw_feat_create(0, &p, &err);
	if (!ft)
		return 2;
	const size_t cap = 9;
	std::vector<float> buf(3 * 2 * 5 * cap, 0.25f), mx(3, 0.0f);
	uint64_t nf[3] = {9, 0, 4}, fill[3] = {9, 3, 2};
	g_log.run = false;
	if (mode == "two") {
		uint64_t nf_b[3] = {1, 2, 3};
		int rc = lw_feat_rows(ft, 2, 5, buf.data(), buf.data(), 3, cap, nf, fill, nullptr, nullptr);
		printf("RC %d LAST %d\n", rc, lw_feat_last_launches(ft));
		nf[0] = 1, fill[1] = 7; // the first call has copied its arrays: the caller's are free
		rc = lw_feat_rows(ft, 2, 5, buf.data(), buf.data(), 3, cap, nf_b, nullptr, nullptr, nullptr);
		printf("RC %d LAST %d\n", rc, lw_feat_last_launches(ft));
		g_log.print([](const LwFeatRow &r) { printf(" %llu/%llu", (unsigned long long)r.n_frames, (unsigned long long)r.fill_end); });
	} else if (mode == "refuse" && argc >= 3) {
		const std::string cs = argv[2];
		uint32_t ch = 2, F = 5;
		const void *s = buf.data();
		void *d = buf.data();
		const uint64_t *n = nf, *fl = fill;
		float *m = nullptr;
		size_t rows = 3, c = cap;
		lw_feat *h = ft;
		if (cs == "null_ft")
			h = nullptr;
		else if (cs == "null_frames")
			n = nullptr;
		else if (cs == "null_src")
			s = nullptr;
		else if (cs == "null_dst")
			d = nullptr;
		else if (cs == "null_dst_fill_only")
			nf[0] = nf[2] = 0, s = nullptr, d = nullptr; // nothing to read, but row 1 is filled to 3
		else if (cs == "frames_over")
			nf[2] = cap + 1; // (the LAST row: every row is checked before anything is queued)
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
		else if (cs == "too_many_runs")
			c = (size_t)1 << 40, F = 65535, fill[0] = c, ch = 1; // 2^32 runs and more in a channel
		else if (cs == "ok_nothing")
			nf[0] = nf[2] = 0, fl = nullptr, s = nullptr, d = nullptr; // no frame, no fill: accepted, nothing queued
		else if (cs == "ok_no_rows")
			rows = 0, n = nullptr;
		else if (cs == "ok_max")
			m = mx.data();
		else if (cs == "ok_max_of_nothing")
			nf[0] = nf[2] = 0, fl = nullptr, s = nullptr, d = nullptr, m = mx.data(); // M of empty scopes is still owed
		else if (cs != "ok")
			return 2;
		const int rc = lw_feat_rows(h, ch, F, s, d, rows, c, n, fl, m, nullptr);
		printf("RC %d\nLAUNCHES %d\nLAST %d\n", rc, g_log.launches, lw_feat_last_launches(ft));
	} else {
		return 2;
	}
	lw_feat_destroy(ft);
	return 0;
}
