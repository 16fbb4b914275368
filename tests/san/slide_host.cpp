// Sliding-window normalisation WITHOUT a GPU: lw_slide.cpp linked against hip_standins.inc (device memory = calloc), and the KERNEL
// source itself, lw_kernels_slide.hip, compiled for the host (LW_SLIDE_HOST): the stand-in for the launcher below runs it
// workgroup by workgroup, the phases in the kernel's own order (every lane of a phase before the next: the barrier), the LDS image
// an exact-size allocation, so AddressSanitizer sees every load and store the kernel makes.  Built with
// -fsanitize=address,undefined; tests/test_host_slide.py drives it.
//   slide_host create W MIN CENTER NORM_VARS [DEVICE]      "RC err" (the stand-ins have ONE device, 0)
//   slide_host window W MIN CENTER T                       "s e" of lw_slide_window for t = 0 .. T - 1, then "RC rc" for t = T
//   slide_host plan F W TILE                               "TILE t COLS c PITCH p NB n LINES l LDS b", or "REFUSED"
//   slide_host tile W TILE BAD                             "RC rc TILE t": lw_slide_set_tile_frames(TILE), then (BAD)
//   slide_host refuse CASE                                 "RC rc", "LAUNCHES n", "LAST n": CASE is one of the refusals of lw_slide_rows
//   slide_host two                                         two calls queued back to back: "ROWS n/fill_end..." per launch, read at the end
//   slide_host run W MIN CENTER NORM_VARS TILE CH F ROWS CAP FILL OFF_SRC OFF_DST IN OUT
//                                   IN: u64 n[ROWS], u64 fill_to[ROWS], f32 x[ROWS][CH][F][CAP]; OUT: the destination, sentinel-filled
//                                   before the call.  FILL 0 = the array is NULL.  The buffers are exact-size, start OFF_* BYTES
//                                   behind a 16-byte boundary and have a guarded front.  "RC rc", "LAUNCHES n", "TILE n"
//   slide_host far W MIN CENTER NORM_VARS TILE F BASE KEEP IN OUT
//                                   ONE row and channel of T = BASE + KEEP frames, capacity T, of which only frames [BASE, T) exist:
//                                   IN holds f32 x[F][KEEP], the source pointer is moved BASE frames in front of it, and only the
//                                   workgroups whose tiles lie wholly at or beyond BASE + 2 W + TILE are run.  OUT: f32 [F][KEEP]
//                                   (sentinel where nothing ran).  BASE is past 2^32: the offsets of a tile far up a row.
#include "../../include/lewton_amd.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "hip_standins.inc"
#include "kernel_host.hpp"

#define LW_SLIDE_HOST 1
#include "../../lewton_amd/csrc/lw_kernels_slide.hip"

static LaunchLog<LwSlideRow> g_log;
static uint64_t g_from_frame = 0; // far: only tiles that start at or beyond this frame are run

template <bool NV>
static void block(const LwSlideArgs &a, const LwSlTile &t, const float *src, float *dst, double *bs, float *xf)
{
	if (t.fill_hi > t.fill_lo)
		for (uint32_t tid = 0; tid < LW_SL_THREADS; tid++)
			lw_sl_fill(a, t, dst, tid);
	if (!t.nt)
		return;
	memset(bs, 0xff, (size_t)a.plan.lds); // what a stale image would show: NaNs, as floats and as doubles
	for (uint32_t tid = 0; tid < LW_SL_THREADS; tid++)
		lw_sl_load(a, t, src, xf, tid);
	for (uint32_t tid = 0; tid < LW_SL_THREADS; tid++) // (behind the barrier)
		lw_sl_blocks<NV>(a, t, xf, bs, tid);
	for (uint32_t tid = 0; tid < LW_SL_THREADS; tid++) // (behind the barrier)
		lw_sl_apply<NV>(a, t, xf, bs, dst, tid);
}

hipError_t lw_launch_slide(const LwSlideArgs &a, const float *src, float *dst, uint32_t tiles, uint32_t n_rows, hipStream_t)
{
	g_log.launch(a.rows + a.row0, n_rows);
	LwSlidePlan p;
	if (!a.rows || n_rows == 0 || n_rows > 65535u || tiles == 0 || !dst || !lw_slide_plan(a.F, a.W, a.plan.tile, p) || p.cols != a.plan.cols ||
			p.pitch != a.plan.pitch || p.nb != a.plan.nb || p.lines != a.plan.lines || p.lds != a.plan.lds || p.lds > LW_SL_LDS_BUDGET ||
			a.groups != (a.F + p.lines - 1u) / p.lines || (uint64_t)tiles * a.groups > LW_SL_MAX_TILES)
		bad("arguments");
	if (!g_log.run)
		return hipSuccess;
	double *bs = (double *)malloc(a.plan.lds); // exact size: one dword beyond the image is a report
	float *xf = (float *)(bs + 2u * a.plan.lines * a.plan.nb);
	for (uint32_t bz = 0; bz < n_rows; bz++)
		for (uint32_t by = 0; by < a.ch; by++)
			for (uint32_t bx = 0; bx < tiles * a.groups; bx++) {
				if ((uint64_t)(bx / a.groups) * a.plan.tile < g_from_frame)
					continue;
				LwSlTile t;
				if (!lw_sl_tile(a, bx, by, bz, t))
					continue;
				if (t.len > a.plan.cols)
					bad("a span of %u frames in an image of %u", t.len, a.plan.cols);
				if (a.norm_vars)
					block<true>(a, t, src, dst, bs, xf);
				else
					block<false>(a, t, src, dst, bs, xf);
			}
	free(bs);
	return hipSuccess;
}

static lw_slide_params params(char **v) // W MIN CENTER NORM_VARS
{
	lw_slide_params p{};
	p.cmn_window = (uint32_t)strtoul(v[0], nullptr, 10), p.min_cmn_window = (uint32_t)strtoul(v[1], nullptr, 10);
	p.center = atoi(v[2]), p.norm_vars = atoi(v[3]);
	return p;
}

int main(int argc, char **argv)
{
	if (argc < 2)
		return 2;
	const std::string mode = argv[1];
	int err = 0;
	if (mode == "create" && argc >= 6) {
		lw_slide_params p = params(argv + 2);
		lw_slide *sl = lw_slide_create(argc >= 7 ? atoi(argv[6]) : 0, &p, &err);
		printf("RC %d\n", err);
		if ((sl == nullptr) != (err != 0))
			return 3;
		if (sl && (lw_slide_tile_frames(sl) != LW_SL_TILE || lw_slide_last_launches(sl) != -1))
			return 3;
		lw_slide_destroy(sl);
		return 0;
	}
	if (mode == "window" && argc >= 6) {
		lw_slide_params p{};
		p.cmn_window = (uint32_t)atoi(argv[2]), p.min_cmn_window = (uint32_t)atoi(argv[3]), p.center = atoi(argv[4]);
		lw_slide *sl = lw_slide_create(0, &p, &err);
		if (!sl)
			return 2;
		const uint64_t T = strtoull(argv[5], nullptr, 10);
		uint64_t s = 0, e = 0;
		for (uint64_t t = 0; t < T; t++) {
			if (lw_slide_window(sl, t, T, &s, &e) != LW_OK)
				return 3;
			printf("%llu %llu\n", (unsigned long long)s, (unsigned long long)e);
		}
		printf("RC %d\n", lw_slide_window(sl, T, T, &s, &e));
		if (lw_slide_window(nullptr, 0, 1, &s, &e) != LW_ERR_NULL_ARG || lw_slide_window(sl, 0, 1, nullptr, &e) != LW_ERR_NULL_ARG ||
				lw_slide_window(sl, 0, 1, &s, nullptr) != LW_ERR_NULL_ARG || lw_slide_tile_frames(nullptr) != 0 ||
				lw_slide_set_tile_frames(nullptr, 16) != LW_ERR_NULL_ARG || lw_slide_last_launches(nullptr) != -1)
			return 3;
		lw_slide_destroy(sl);
		return 0;
	}
	if (mode == "plan" && argc >= 5) {
		LwSlidePlan p;
		if (!lw_slide_plan((uint32_t)atoi(argv[2]), (uint32_t)atoi(argv[3]), (uint32_t)atoi(argv[4]), p))
			printf("REFUSED\n");
		else
			printf("TILE %u COLS %u PITCH %u NB %u LINES %u LDS %u\n", p.tile, p.cols, p.pitch, p.nb, p.lines, p.lds);
		return 0;
	}
	if (mode == "tile" && argc >= 4) {
		lw_slide_params p{};
		p.cmn_window = (uint32_t)atoi(argv[2]), p.min_cmn_window = 1;
		lw_slide *sl = lw_slide_create(0, &p, &err);
		if (!sl)
			return 2;
		const int rc = lw_slide_set_tile_frames(sl, (uint32_t)atoi(argv[3]));
		printf("RC %d TILE %u\n", rc, lw_slide_tile_frames(sl));
		lw_slide_destroy(sl);
		return 0;
	}
	if (mode == "run" && argc >= 16) {
		lw_slide_params p = params(argv + 2);
		const uint32_t tile = (uint32_t)atoi(argv[6]), ch = (uint32_t)atoi(argv[7]), F = (uint32_t)atoi(argv[8]);
		const size_t rows = (size_t)atoll(argv[9]), cap = (size_t)atoll(argv[10]);
		const bool fill = atoi(argv[11]) != 0;
		const size_t nb = rows * ch * F * cap * 4;
		std::vector<uint64_t> cnt(rows + 1), fill_to(rows + 1);
		const Guarded gs = shifted(nb, (unsigned)atoi(argv[12])), gd = shifted(nb, (unsigned)atoi(argv[13]));
		{
			File in(argv[14], "rb");
			in.get(cnt.data(), rows), in.get(fill_to.data(), rows), in.get(gs.at, nb);
		}
		lw_slide *sl = lw_slide_create(0, &p, &err);
		if (!sl || lw_slide_set_tile_frames(sl, tile) != LW_OK)
			return 2;
		fill32(gd.at, nb / 4, SENT_DEAD);
		const int rc = lw_slide_rows(sl, ch, F, gs.at, gd.at, rows, cap, cnt.data(), fill ? fill_to.data() : nullptr, nullptr);
		printf("RC %d\nLAUNCHES %d\nTILE %u\n", rc, g_log.launches, lw_slide_tile_frames(sl));
		if (rc == LW_OK && lw_slide_last_launches(sl) != g_log.launches)
			return 3;
		File(argv[15], "wb").put(gd.at, nb);
		if (!guard_intact(gs) || !guard_intact(gd))
			bad("a store in front of a buffer");
		free(gs.base), free(gd.base);
		lw_slide_destroy(sl);
		return 0;
	}
	if (mode == "far" && argc >= 12) {
		lw_slide_params p = params(argv + 2);
		const uint32_t tile = (uint32_t)atoi(argv[6]), F = (uint32_t)atoi(argv[7]);
		const uint64_t base = strtoull(argv[8], nullptr, 10), keep = strtoull(argv[9], nullptr, 10), T = base + keep;
		std::vector<float> x((size_t)(F * keep)), y((size_t)(F * keep));
		File(argv[10], "rb").get(x.data(), x.size());
		fill32(y.data(), y.size(), SENT_DEAD);
		// line g of the row starts g * T elements behind line 0, so only its last `keep` frames are backed by memory: one buffer per
		// line would be needed for F > 1 with capacity T, so the row has capacity T and the lines are run ONE per call, each with
		// its pointer moved `base` frames in front of its data
		lw_slide *sl = lw_slide_create(0, &p, &err);
		if (!sl || lw_slide_set_tile_frames(sl, tile) != LW_OK)
			return 2;
		g_from_frame = base + 2u * (uint64_t)p.cmn_window + tile;
		g_from_frame += (tile - g_from_frame % tile) % tile;
		int rc = 0;
		for (uint32_t g = 0; g < F && rc == 0; g++) {
			const uintptr_t s = (uintptr_t)(x.data() + (size_t)g * keep) - (uintptr_t)base * 4u, d = (uintptr_t)(y.data() + (size_t)g * keep) - (uintptr_t)base * 4u;
			rc = lw_slide_rows(sl, 1, 1, (const void *)s, (void *)d, 1, (size_t)T, &T, nullptr, nullptr);
		}
		printf("RC %d\nLAUNCHES %d\nFROM %llu\n", rc, g_log.launches, (unsigned long long)(g_from_frame - base));
		File(argv[11], "wb").put(y.data(), y.size());
		lw_slide_destroy(sl);
		return 0;
	}
	// ---- calls on a small fixture: 3 rows of 2 channels, 5 lines, the x-vector window, capacity 700
	lw_slide_params p{};
	p.cmn_window = 300, p.min_cmn_window = 100, p.center = 1, p.norm_vars = 1;
	lw_slide *sl = lw_slide_create(0, &p, &err);
	if (!sl)
		return 2;
	const size_t cap = 700;
	std::vector<float> src(3 * 2 * 5 * cap, 0.25f), dst(3 * 2 * 5 * cap, 0.0f);
	uint64_t cnt[3] = {700, 0, 4}, fill[3] = {700, 3, 0};
	g_log.run = false;
	if (mode == "two") {
		uint64_t cnt_b[3] = {1, 257, 13};
		int rc = lw_slide_rows(sl, 2, 5, src.data(), dst.data(), 3, cap, cnt, fill, nullptr);
		printf("RC %d LAST %d\n", rc, lw_slide_last_launches(sl));
		cnt[0] = 1, fill[1] = 7; // the first call has copied its arrays: the caller's are free
		rc = lw_slide_rows(sl, 2, 5, src.data(), dst.data(), 3, cap, cnt_b, nullptr, nullptr);
		printf("RC %d LAST %d\n", rc, lw_slide_last_launches(sl));
		g_log.print([](const LwSlideRow &r) { printf(" %llu/%llu", (unsigned long long)r.n, (unsigned long long)r.fill_end); });
	} else if (mode == "refuse" && argc >= 3) {
		const std::string cs = argv[2];
		uint32_t ch = 2, F = 5;
		const void *s = src.data();
		void *d = dst.data();
		const uint64_t *n = cnt, *fl = fill;
		size_t rows = 3, c = cap;
		lw_slide *h = sl;
		if (cs == "null_sl")
			h = nullptr;
		else if (cs == "null_n")
			n = nullptr;
		else if (cs == "null_src")
			s = nullptr;
		else if (cs == "null_dst")
			d = nullptr;
		else if (cs == "null_dst_fill_only")
			cnt[0] = cnt[2] = 0, s = nullptr, d = nullptr; // nothing to read, but rows 0 and 1 are filled
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
			c = (size_t)1 << 60, fl = nullptr;
		else if (cs == "too_many_tiles") // 2^24 tiles of 1024 frames to fill, one more than a grid counts
			c = (size_t)1 << 35, ch = 1, F = 1, rows = 1, cnt[0] = 0, fill[0] = (uint64_t)1024 << 24;
		else if (cs == "too_many_groups") // 80 lines are 10 groups: 2^21 tiles of them are more than a grid counts
			c = (size_t)1 << 32, ch = 1, F = 80, rows = 1, cnt[0] = 0, fill[0] = (uint64_t)1024 << 21;
		else if (cs == "ok_most_tiles")
			c = (size_t)1 << 35, ch = 1, F = 1, rows = 1, cnt[0] = 0, fill[0] = ((uint64_t)1024 << 24) - 1024; // 2^24 - 1 tiles: accepted
		else if (cs == "ok_nothing")
			cnt[0] = cnt[2] = 0, fl = nullptr, s = nullptr, d = nullptr; // all rows empty, no fill: accepted, nothing queued
		else if (cs == "ok_no_rows")
			rows = 0, n = nullptr;
		else if (cs == "ok_fill_only")
			cnt[0] = cnt[2] = 0, s = nullptr;
		else if (cs != "ok")
			return 2;
		const int rc = lw_slide_rows(h, ch, F, s, d, rows, c, n, fl, nullptr);
		printf("RC %d\nLAUNCHES %d\nLAST %d\n", rc, g_log.launches, lw_slide_last_launches(sl));
		for (float v : dst)
			if (v != 0.0f)
				return 3; // (nothing runs in this mode; a refusal has written nothing either way)
	} else {
		return 2;
	}
	lw_slide_destroy(sl);
	return 0;
}
