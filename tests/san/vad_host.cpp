// The energy VAD WITHOUT a GPU: lw_vad.cpp linked against hip_standins.inc (device memory = calloc), and the KERNEL source itself,
// lw_kernels_vad.hip, compiled for the host (LW_VAD_HOST): the stand-ins for the launchers below run it workgroup by workgroup, the
// phases in the kernels' own order (every wave or lane of a phase before the next: the barrier), the LDS an allocation of its exact
// size, so AddressSanitizer sees every load and store the kernels make.  Built with -fsanitize=address,undefined;
// tests/test_host_vad.py drives it.  Float parameters travel as the bit patterns of their float32 values (THR SCALE PROP below).
//   vad_host create DEVICE THR SCALE CTX PROP LINE RESERVED   "RC err" (the stand-ins have ONE device, 0)
//   vad_host tile TILE                 "RC rc TILE t": lw_vad_set_tile_frames(TILE), then lw_vad_tile_frames
//   vad_host route ROUTE               "RC rc": lw_vad_set_route(ROUTE)
//   vad_host scalars THR SCALE PROP IN OUT
//                                      IN: u64 n, n x (f64 S, u64 T), u64 m, m x (u64 num, u64 den); OUT: n x f32 lw_vad_threshold,
//                                      m x u8 lw_vad_voiced
//   vad_host refuse CASE               "RC rc", "LAUNCHES n", "LAST n", "THR ...": CASE is one of the calls of main below
//   vad_host two                       two calls queued back to back: "ROWS n/fill_end..." per decide launch, read at the end
//   vad_host run TILE ROUTE CH F LINE ROWS CAP FILL WANT_THR OFF_SRC OFF_MASK THR SCALE CTX PROP IN OUT
//                                      IN: u64 n[ROWS], u64 fill_to[ROWS], f32 x[ROWS][CH][F][CAP]; OUT: the mask u8 [ROWS][CH][CAP],
//                                      sentinel-filled before the call, then f32 thr[ROWS][CH] (sentinel-filled too).  FILL,
//                                      WANT_THR: 0 = the array is NULL.  The buffers are exact-size, start OFF_* BYTES behind a
//                                      16-byte boundary and have a guarded front.  "RC rc", "LAUNCHES n", "TILE n"
//   vad_host far TILE BASE KEEP THR SCALE CTX PROP IN OUT
//                                      ONE row and channel of T = BASE + KEEP frames, capacity T, F = 1, of which only frames
//                                      [BASE, T) exist (BASE a multiple of TILE, past 2^32): IN holds f32 e[KEEP]; the pointers are
//                                      moved BASE frames in front of the data; the chunks in front of BASE are not summed and
//                                      count as 256 frames of 12.0, the tiles in front of BASE + TILE are not run (the halo of
//                                      the first one would reach in front of the data).  OUT: u8 mask[KEEP], then f32 thr
#include "../../include/lewton_amd.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "hip_standins.inc"
#include "kernel_host.hpp"

#define LW_VAD_HOST 1
#include "../../lewton_amd/csrc/lw_kernels_vad.hip"

static LaunchLog<LwVadRow> g_log; // (the records of the decide launches)
static uint64_t g_from_frame = 0; // far: what lies in front of this frame does not exist
static const double FAR_CHUNK = 256.0 * 12.0;
static const unsigned char SENT_MASK = 0xa5;

static void check(const LwVadArgs &a, uint32_t n_rows, bool decide)
{
	if (!a.rows || n_rows == 0 || n_rows > 65535u || !lw_vad_tile_ok(a.tile) || a.ctx > LW_VD_MAX_CONTEXT || a.line >= a.F || a.ch == 0 ||
			(decide && (a.tiles == 0 || a.tiles > LW_VD_MAX_TILES)))
		bad("arguments");
}

#define WAVES(stmt) \
	for (uint32_t wave = 0; wave < LW_VD_WAVES; wave++) \
	stmt
#define LANES(stmt) \
	for (uint32_t tid = 0; tid < LW_VD_THREADS; tid++) \
	stmt

// a decide workgroup, the phases in lw_vd_workgroup's order
static void decide_workgroups(const LwVadArgs &a, uint32_t n_rows, bool sums)
{
	LwVdLds *l = (LwVdLds *)malloc(sizeof(LwVdLds));
	for (uint32_t bz = 0; bz < n_rows; bz++)
		for (uint32_t by = 0; by < a.ch; by++)
			for (uint32_t bx = 0; bx < a.tiles; bx++) {
				LwVdTile t;
				lw_vd_tile(a, bx, by, bz, t);
				const bool owes = lw_vd_owes_thr(a, t), frames = t.t0 < t.n;
				if (t.t0 >= t.fill_end && !owes)
					continue;
				if (g_from_frame && t.t0 < g_from_frame + a.tile)
					continue;
				memset(l, 0xff, sizeof(LwVdLds));
				float thr = a.energy_threshold;
				if (frames || owes) {
					if (sums) {
						if (t.n && a.energy_mean_scale != 0.0f) {
							WAVES(lw_vd_sum_lds(a, t, *l, wave, 0u);)
							thr = lw_vad_threshold_value(a.energy_threshold, a.energy_mean_scale, lw_vd_fold_lds(*l, t.chunks, 0u), t.n);
						}
					} else if (a.thr) {
						thr = a.thr[t.thr_at];
					}
				}
				if (owes)
					a.d_thr[t.thr_at] = thr;
				if (frames)
					WAVES(lw_vd_stage_wave(a, t, thr, *l, wave, 0u);)
				LANES(lw_vd_write(a, t, *l, tid);)
			}
	free(l);
}

hipError_t lw_launch_vad(const LwVadArgs &a, uint32_t n_rows, hipStream_t)
{
	g_log.launch(a.rows + a.row0, n_rows);
	check(a, n_rows, true);
	if ((uint64_t)a.tiles * a.tile > LW_VD_FUSED_MAX + LW_VD_MAX_TILE - 1u || a.thr_out != 1u)
		bad("arguments of the fused form");
	if (g_log.run)
		decide_workgroups(a, n_rows, true);
	return hipSuccess;
}

hipError_t lw_launch_vad_decide(const LwVadArgs &a, uint32_t n_rows, hipStream_t)
{
	g_log.launch(a.rows + a.row0, n_rows);
	check(a, n_rows, true);
	if ((a.thr != nullptr) == (a.thr_out != 0u))
		bad("the thresholds come from the fold or are stored by tile 0, not both");
	if (g_log.run)
		decide_workgroups(a, n_rows, false);
	return hipSuccess;
}

hipError_t lw_launch_vad_sum(const LwVadArgs &a, uint32_t n_rows, hipStream_t)
{
	g_log.launch();
	check(a, n_rows, false);
	if (!a.src || !a.part || !a.sum_chunks || !a.sum_per_wave || !a.sum_tiles || (uint64_t)a.sum_tiles * a.sum_per_wave * LW_VD_WAVES < a.sum_chunks)
		bad("arguments of the sums");
	if (!g_log.run)
		return hipSuccess;
	if (g_from_frame) { // far: the row's chunks in front of the data are constants, the others are summed a chunk at a time
		LwVdTile t;
		lw_vd_tile(a, 0u, 0u, 0u, t);
		for (uint64_t c = 0; c < t.chunks; c++)
			a.part[t.list_at + c] = c * LW_VD_CHUNK < g_from_frame ? FAR_CHUNK : lw_vd_chunk(a.src, t.src_at, t.n, (uint32_t)c, 0u);
		return hipSuccess;
	}
	for (uint32_t bz = 0; bz < n_rows; bz++)
		for (uint32_t by = 0; by < a.ch; by++)
			for (uint32_t bx = 0; bx < a.sum_tiles; bx++)
				WAVES(lw_vd_sum_wave(a, bx, by, bz, wave, 0u);)
	return hipSuccess;
}

hipError_t lw_launch_vad_fold(const LwVadArgs &a, uint32_t n_rows, hipStream_t)
{
	g_log.launch();
	check(a, n_rows, false);
	if (!a.thr || !a.scratch || !a.fold_scratch || !a.part)
		bad("arguments of the fold");
	if (!g_log.run)
		return hipSuccess;
	for (uint32_t bz = 0; bz < n_rows; bz++)
		for (uint32_t by = 0; by < a.ch; by++) {
			LwVdLevels v;
			lw_vd_levels(a, by, bz, v);
			while (v.len > 1) {
				WAVES(lw_vd_level_wave(v, wave, 0u);)
				lw_vd_level_next(v);
			}
			lw_vd_levels_out(a, v);
		}
	return hipSuccess;
}

hipError_t lw_launch_vad_fill(float *d_thr, uint64_t n, float value, hipStream_t)
{
	g_log.launch();
	if (!d_thr || !n)
		bad("arguments of the fill");
	for (uint64_t i = 0; i < n; i++)
		d_thr[i] = value;
	return hipSuccess;
}

static float f32_of(const char *bits)
{
	const uint32_t u = (uint32_t)strtoul(bits, nullptr, 10);
	float f;
	memcpy(&f, &u, 4);
	return f;
}

static lw_vad_params params(const char *thr, const char *scale, const char *ctx, const char *prop, uint32_t line = 0, uint32_t reserved = 0)
{
	lw_vad_params p;
	p.energy_threshold = f32_of(thr), p.energy_mean_scale = f32_of(scale), p.frames_context = (uint32_t)strtoul(ctx, nullptr, 10);
	p.proportion_threshold = f32_of(prop), p.line = line, p.reserved = reserved;
	return p;
}

int main(int argc, char **argv)
{
	if (argc < 2)
		return 2;
	const std::string mode = argv[1];
	int err = 0;
	lw_vad_params dflt{5.0f, 0.5f, 0u, 0.6f, 0u, 0u};
	if (mode == "create" && argc >= 9) {
		const lw_vad_params p = params(argv[3], argv[4], argv[5], argv[6], (uint32_t)strtoul(argv[7], nullptr, 10), (uint32_t)strtoul(argv[8], nullptr, 10));
		lw_vad *v = lw_vad_create(atoi(argv[2]), &p, &err);
		printf("RC %d\n", err);
		if ((v == nullptr) != (err != 0))
			return 3;
		if (v && (lw_vad_tile_frames(v) != LW_VD_TILE || lw_vad_last_launches(v) != -1))
			return 3;
		float thr = 0.0f;
		if (lw_vad_tile_frames(nullptr) != 0 || lw_vad_set_tile_frames(nullptr, 256) != LW_ERR_NULL_ARG || lw_vad_last_launches(nullptr) != -1 ||
				lw_vad_set_route(nullptr, 0) != LW_ERR_NULL_ARG || lw_vad_threshold(nullptr, 0.0, 1, &thr) != LW_ERR_NULL_ARG ||
				(v && lw_vad_threshold(v, 0.0, 1, nullptr) != LW_ERR_NULL_ARG) || lw_vad_voiced(nullptr, 1, 1) != -1 ||
				lw_vad_create(0, nullptr, &err) != nullptr || err != LW_ERR_NULL_ARG)
			return 3;
		lw_vad_destroy(v);
		return 0;
	}
	if ((mode == "tile" || mode == "route") && argc >= 3) {
		lw_vad *v = lw_vad_create(0, &dflt, &err);
		if (!v)
			return 2;
		if (mode == "tile") {
			const int rc = lw_vad_set_tile_frames(v, (uint32_t)atoi(argv[2]));
			printf("RC %d TILE %u\n", rc, lw_vad_tile_frames(v));
		} else {
			printf("RC %d\n", lw_vad_set_route(v, atoi(argv[2])));
		}
		lw_vad_destroy(v);
		return 0;
	}
	if (mode == "scalars" && argc >= 7) {
		const lw_vad_params p = params(argv[2], argv[3], "0", argv[4]);
		lw_vad *v = lw_vad_create(0, &p, &err);
		if (!v)
			return 2;
		File in(argv[5], "rb"), out(argv[6], "wb");
		uint64_t n = 0;
		in.get(&n, 1);
		for (uint64_t i = 0; i < n; i++) {
			double S;
			uint64_t T;
			float thr;
			in.get(&S, 1), in.get(&T, 1);
			if (lw_vad_threshold(v, S, T, &thr) != LW_OK)
				return 3;
			out.put(&thr, 1);
		}
		in.get(&n, 1);
		for (uint64_t i = 0; i < n; i++) {
			uint64_t nd[2];
			in.get(nd, 2);
			const int r = lw_vad_voiced(v, nd[0], nd[1]);
			if (r != 0 && r != 1)
				return 3;
			const uint8_t b = (uint8_t)r;
			out.put(&b, 1);
		}
		lw_vad_destroy(v);
		return 0;
	}
	if (mode == "run" && argc >= 19) {
		const uint32_t tile = (uint32_t)atoi(argv[2]), ch = (uint32_t)atoi(argv[4]), F = (uint32_t)atoi(argv[5]), line = (uint32_t)atoi(argv[6]);
		const int route = atoi(argv[3]);
		const size_t rows = (size_t)atoll(argv[7]), cap = (size_t)atoll(argv[8]);
		const bool fill = atoi(argv[9]) != 0, want_thr = atoi(argv[10]) != 0;
		const size_t nm = rows * ch * cap, nb = nm * F * 4, nt = rows * ch * 4;
		std::vector<uint64_t> cnt(rows + 1), fill_to(rows + 1);
		const Guarded gs = shifted(nb, (unsigned)atoi(argv[11])), gm = shifted(nm, (unsigned)atoi(argv[12])), gt = shifted(nt, 4);
		{
			File in(argv[17], "rb");
			in.get(cnt.data(), rows), in.get(fill_to.data(), rows), in.get(gs.at, nb);
		}
		const lw_vad_params p = params(argv[13], argv[14], argv[15], argv[16], line);
		lw_vad *v = lw_vad_create(0, &p, &err);
		if (!v || lw_vad_set_tile_frames(v, tile) != LW_OK || lw_vad_set_route(v, route) != LW_OK)
			return 2;
		memset(gm.at, SENT_MASK, nm);
		memset(gt.at, 0xee, nt);
		const int rc = lw_vad_rows(v, ch, F, gs.at, (uint8_t *)gm.at, want_thr ? (float *)gt.at : nullptr, rows, cap, cnt.data(), fill ? fill_to.data() : nullptr,
				nullptr);
		printf("RC %d\nLAUNCHES %d\nTILE %u\n", rc, g_log.launches, lw_vad_tile_frames(v));
		if (rc == LW_OK && lw_vad_last_launches(v) != g_log.launches)
			return 3;
		{
			File out(argv[18], "wb");
			out.put(gm.at, nm), out.put(gt.at, nt);
		}
		if (!guard_intact(gs) || !guard_intact(gm) || !guard_intact(gt))
			bad("a store in front of a buffer");
		free(gs.base), free(gm.base), free(gt.base);
		lw_vad_destroy(v);
		return 0;
	}
	if (mode == "far" && argc >= 11) {
		const uint32_t tile = (uint32_t)atoi(argv[2]);
		const uint64_t base = strtoull(argv[3], nullptr, 10), keep = strtoull(argv[4], nullptr, 10), T = base + keep;
		if (base % tile || base % LW_VD_CHUNK || keep <= tile)
			return 2;
		std::vector<float> x((size_t)keep);
		std::vector<uint8_t> m((size_t)keep, SENT_MASK);
		{
			File in(argv[9], "rb");
			in.get(x.data(), x.size());
		}
		const lw_vad_params p = params(argv[5], argv[6], argv[7], argv[8]);
		lw_vad *v = lw_vad_create(0, &p, &err);
		if (!v || lw_vad_set_tile_frames(v, tile) != LW_OK)
			return 2;
		g_from_frame = base;
		float thr = 0.0f;
		const uintptr_t s = (uintptr_t)x.data() - (uintptr_t)base * 4u, d = (uintptr_t)m.data() - (uintptr_t)base;
		const int rc = lw_vad_rows(v, 1, 1, (const void *)s, (uint8_t *)d, &thr, 1, (size_t)T, &T, nullptr, nullptr);
		printf("RC %d\nLAUNCHES %d\n", rc, g_log.launches);
		{
			File out(argv[10], "wb");
			out.put(m.data(), m.size()), out.put(&thr, 1);
		}
		lw_vad_destroy(v);
		return 0;
	}
	// ---- calls on a small fixture: 3 rows of 2 channels, 5 lines, capacity 3000
	const size_t cap = 3000;
	std::vector<float> src(3 * 2 * 5 * cap, 0.25f);
	std::vector<uint8_t> msk(3 * 2 * cap, 7);
	std::vector<float> thr(3 * 2, 77.0f);
	uint64_t cnt[3] = {3000, 0, 4}, fill[3] = {3000, 3, 0};
	g_log.run = false;
	if (mode == "two") {
		lw_vad *v = lw_vad_create(0, &dflt, &err);
		if (!v)
			return 2;
		uint64_t cnt_b[3] = {1, 257, 13};
		int rc = lw_vad_rows(v, 2, 5, src.data(), msk.data(), thr.data(), 3, cap, cnt, fill, nullptr);
		printf("RC %d LAST %d\n", rc, lw_vad_last_launches(v));
		cnt[0] = 1, fill[1] = 7; // the first call has copied its arrays: the caller's are free
		if (lw_vad_set_route(v, LW_VAD_ROUTE_SPLIT) != LW_OK)
			return 3;
		rc = lw_vad_rows(v, 2, 5, src.data(), msk.data(), nullptr, 3, cap, cnt_b, nullptr, nullptr);
		printf("RC %d LAST %d\n", rc, lw_vad_last_launches(v));
		g_log.print([](const LwVadRow &r) { printf(" %llu/%llu", (unsigned long long)r.n, (unsigned long long)r.fill_end); });
		lw_vad_destroy(v);
		return 0;
	}
	if (mode != "refuse" || argc < 3)
		return 2;
	const std::string cs = argv[2];
	uint32_t ch = 2, F = 5;
	const void *s = src.data();
	uint8_t *mk = msk.data();
	const uint64_t *n = cnt, *fl = fill;
	float *dt = thr.data();
	size_t rows = 3, c = cap;
	int route = LW_VAD_ROUTE_AUTO;
	bool null_v = false;
	std::vector<uint64_t> many;
	if (cs == "null_v")
		null_v = true;
	else if (cs == "null_n")
		n = nullptr;
	else if (cs == "null_src")
		s = nullptr;
	else if (cs == "null_src_scale0")
		s = nullptr, dflt.energy_mean_scale = 0.0f; // the frames are read for their decisions all the same
	else if (cs == "null_mask")
		mk = nullptr;
	else if (cs == "null_mask_fill_only")
		cnt[0] = cnt[2] = 0, s = nullptr, mk = nullptr; // nothing to read, but rows 0 and 1 are filled
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
	else if (cs == "line_over")
		dflt.line = 5;
	else if (cs == "too_large")
		c = (size_t)1 << 60, fl = nullptr;
	else if (cs == "too_many_tiles") // 2^24 tiles of 1024 frames to fill, one more than a grid counts
		c = (size_t)1 << 35, ch = 1, F = 1, rows = 1, cnt[0] = 0, fill[0] = (uint64_t)1024 << 24;
	else if (cs == "fused_too_long")
		route = LW_VAD_ROUTE_FUSED, c = 20000, cnt[0] = 100, fill[0] = LW_VAD_FUSED_MAX + 1; // (the span, not the frames alone)
	else if (cs == "ok_most_tiles")
		c = (size_t)1 << 35, ch = 1, F = 1, rows = 1, cnt[0] = 0, fill[0] = ((uint64_t)1024 << 24) - 1024; // 2^24 - 1 tiles: accepted
	else if (cs == "ok_fused_longest")
		route = LW_VAD_ROUTE_FUSED, c = 20000, cnt[0] = LW_VAD_FUSED_MAX, fill[0] = 0; // (nothing runs here: the buffers are only looked at)
	else if (cs == "ok_auto_long")
		c = 20000, cnt[0] = LW_VAD_FUSED_MAX + 1, fill[0] = 0; // one frame past the fused form: three launches
	else if (cs == "ok_split")
		route = LW_VAD_ROUTE_SPLIT;
	else if (cs == "ok_scale0" || cs == "ok_scale0_split")
		dflt.energy_mean_scale = 0.0f, route = cs == "ok_scale0" ? LW_VAD_ROUTE_AUTO : LW_VAD_ROUTE_SPLIT;
	else if (cs == "ok_nothing")
		cnt[0] = cnt[2] = 0, fl = nullptr, s = nullptr, mk = nullptr; // all rows empty, no fill: the thresholds alone, by one workgroup
	else if (cs == "ok_nothing_no_thr")
		cnt[0] = cnt[2] = 0, fl = nullptr, s = nullptr, mk = nullptr, dt = nullptr;
	else if (cs == "ok_no_rows")
		rows = 0, n = nullptr;
	else if (cs == "ok_fill_only")
		cnt[0] = cnt[2] = 0, s = nullptr; // no row has a frame: nothing is summed, the decide launch fills
	else if (cs == "ok_rows65536" || cs == "ok_rows65536_split") // two launch groups
		rows = 65536, many.assign(rows, 0), many[65535] = 4, n = many.data(), fl = nullptr, ch = 1, F = 1, c = 4,
		route = cs == "ok_rows65536" ? LW_VAD_ROUTE_AUTO : LW_VAD_ROUTE_SPLIT, dt = nullptr;
	else if (cs != "ok")
		return 2;
	lw_vad *v = lw_vad_create(0, &dflt, &err);
	if (!v || lw_vad_set_route(v, route) != LW_OK)
		return 2;
	const int rc = lw_vad_rows(null_v ? nullptr : v, ch, F, s, mk, dt, rows, c, n, fl, nullptr);
	printf("RC %d\nLAUNCHES %d\nLAST %d\n", rc, g_log.launches, lw_vad_last_launches(v));
	printf("THR");
	for (float t : thr)
		printf(" %g", t);
	printf("\n");
	lw_vad_destroy(v);
	return 0;
}
