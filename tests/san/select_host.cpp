// Frame selection WITHOUT a GPU: lw_select.cpp linked against hip_standins.inc (device memory = calloc), and the KERNEL source
// itself, lw_kernels_select.hip, compiled for the host (LW_SELECT_HOST): the stand-ins for the launchers below run it workgroup by
// workgroup, the phases in the kernels' own order (every lane of a phase before the next: the barrier), the LDS an allocation of
// its exact size, so AddressSanitizer sees every load and store the kernels make.  Built with -fsanitize=address,undefined;
// tests/test_host_select.py drives it.
//   select_host create [DEVICE]                  "RC err" (the stand-ins have ONE device, 0)
//   select_host tile TILE                        "RC rc TILE t": lw_select_set_tile_frames(TILE), then lw_select_tile_frames
//   select_host refuse CASE                      "RC rc", "LAUNCHES n", "LAST n": CASE is one of the refusals of lw_select_rows (main below)
//   select_host two                              two calls queued back to back: "ROWS n/fill_end..." per launch, read at the end
//   select_host run TILE CH F ROWS CAP FILL COUNTS OFF_SRC OFF_DST IN OUT
//                                   IN: u64 n[ROWS], u64 fill_to[ROWS], u8 mask[ROWS][CH][CAP], f32 x[ROWS][CH][F][CAP]; OUT: the
//                                   destination, sentinel-filled before the call, then u64 counts[ROWS][CH] (sentinel-filled too).
//                                   FILL, COUNTS: 0 = the array is NULL.  The buffers are exact-size, start OFF_* BYTES behind a
//                                   16-byte boundary and have a guarded front.  "RC rc", "LAUNCHES n", "TILE n"
//   select_host far TILE F BASE KEEP IN OUT
//                                   ONE row and channel of T = BASE + KEEP frames, capacity T, of which only frames [BASE, T) exist
//                                   (BASE a multiple of TILE, past 2^32): IN holds u8 mask[KEEP], f32 x[F][KEEP]; the pointers are
//                                   moved BASE frames in front of the data, the tiles in front of BASE are not run and count as
//                                   kept whole, so the kept frames land from position BASE on.  OUT: f32 [F][KEEP], then u64 K
#include "../../include/lewton_amd.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "hip_standins.inc"
#include "kernel_host.hpp"

#define LW_SELECT_HOST 1
#include "../../lewton_amd/csrc/lw_kernels_select.hip"

static LaunchLog<LwSelectRow> g_log; // (the records of the k_select launches)
static uint64_t g_from_frame = 0; // far: the tiles in front of this frame are not run and count as kept whole

static void check(const LwSelectArgs &a, uint32_t n_rows)
{
	if (!a.rows || !a.tile_counts || n_rows == 0 || n_rows > 65535u || !lw_select_tile_ok(a.tile) || a.tiles == 0 ||
			a.groups != (a.F + LW_SE_LINES - 1u) / LW_SE_LINES || (uint64_t)a.tiles * a.groups > LW_SE_MAX_TILES)
		bad("arguments");
}

#define LANES(stmt) \
	for (uint32_t tid = 0; tid < LW_SE_THREADS; tid++) \
	stmt

hipError_t lw_launch_select_count(const LwSelectArgs &a, const uint8_t *mask, uint32_t n_rows, hipStream_t)
{
	g_log.launch();
	check(a, n_rows);
	if (!mask)
		bad("arguments");
	if (!g_log.run)
		return hipSuccess;
	LwSeLds *l = (LwSeLds *)malloc(sizeof(LwSeLds));
	for (uint32_t bz = 0; bz < n_rows; bz++)
		for (uint32_t by = 0; by < a.ch; by++)
			for (uint32_t bx = 0; bx < a.tiles; bx++) {
				LwSeTile t;
				lw_se_tile(a, bx, 0u, by, bz, t);
				if (!t.nt)
					continue;
				if (t.t0 < g_from_frame) {
					a.tile_counts[t.list_at + t.tile_i] = a.tile;
					continue;
				}
				memset(l, 0xff, sizeof(LwSeLds));
				LANES(lw_se_count(a, t, mask, *l, tid);)
				LANES(lw_se_groups(*l, tid);)
				a.tile_counts[t.list_at + t.tile_i] = lw_se_total(*l);
			}
	free(l);
	return hipSuccess;
}

hipError_t lw_launch_select(const LwSelectArgs &a, const uint32_t *src, const uint8_t *mask, uint32_t *dst, uint32_t n_rows, hipStream_t)
{
	g_log.launch(a.rows + a.row0, n_rows);
	check(a, n_rows);
	if (!g_log.run)
		return hipSuccess;
	LwSeLds *l = (LwSeLds *)malloc(sizeof(LwSeLds));
	for (uint32_t bz = 0; bz < n_rows; bz++)
		for (uint32_t by = 0; by < a.ch; by++)
			for (uint32_t bx = 0; bx < a.tiles * a.groups; bx++) {
				LwSeTile t;
				lw_se_tile(a, bx / a.groups, bx % a.groups, by, bz, t);
				const bool counts = a.d_counts && t.tile_i == 0 && t.grp == 0;
				if ((t.t0 >= t.fill_end && !counts) || (t.t0 < g_from_frame && !counts))
					continue;
				const bool far_front = t.t0 < g_from_frame; // (far: tile 0 is there for the count alone, its frames do not exist)
				memset(l, far_front ? 0 : 0xff, sizeof(LwSeLds));
				LANES(lw_se_partial(a, t, *l, tid);)
				if (!far_front)
					LANES(lw_se_count(a, t, mask, *l, tid);)
				LANES(lw_se_fold(*l, tid);)
				LANES(lw_se_groups(*l, tid);)
				const uint64_t base = lw_se_sum(*l, 0u), K = lw_se_sum(*l, 1u);
				const uint32_t kept = lw_se_total(*l);
				if (counts)
					a.d_counts[t.cnt_at] = K;
				if (far_front)
					continue;
				LANES(lw_se_places(a, t, mask, *l, tid);)
				LANES(lw_se_copy(a, t, src, dst, *l, base, K, kept, tid);)
			}
	free(l);
	return hipSuccess;
}

int main(int argc, char **argv)
{
	if (argc < 2)
		return 2;
	const std::string mode = argv[1];
	int err = 0;
	if (mode == "create") {
		lw_select *se = lw_select_create(argc >= 3 ? atoi(argv[2]) : 0, &err);
		printf("RC %d\n", err);
		if ((se == nullptr) != (err != 0))
			return 3;
		if (se && (lw_select_tile_frames(se) != LW_SE_TILE || lw_select_last_launches(se) != -1))
			return 3;
		if (lw_select_tile_frames(nullptr) != 0 || lw_select_set_tile_frames(nullptr, 256) != LW_ERR_NULL_ARG || lw_select_last_launches(nullptr) != -1)
			return 3;
		lw_select_destroy(se);
		return 0;
	}
	if (mode == "tile" && argc >= 3) {
		lw_select *se = lw_select_create(0, &err);
		if (!se)
			return 2;
		const int rc = lw_select_set_tile_frames(se, (uint32_t)atoi(argv[2]));
		printf("RC %d TILE %u\n", rc, lw_select_tile_frames(se));
		lw_select_destroy(se);
		return 0;
	}
	if (mode == "run" && argc >= 13) {
		const uint32_t tile = (uint32_t)atoi(argv[2]), ch = (uint32_t)atoi(argv[3]), F = (uint32_t)atoi(argv[4]);
		const size_t rows = (size_t)atoll(argv[5]), cap = (size_t)atoll(argv[6]);
		const bool fill = atoi(argv[7]) != 0, want_counts = atoi(argv[8]) != 0;
		const size_t nm = rows * ch * cap, nb = nm * F * 4, nc = rows * ch * 8;
		std::vector<uint64_t> cnt(rows + 1), fill_to(rows + 1);
		const Guarded gs = shifted(nb, (unsigned)atoi(argv[9])), gd = shifted(nb, (unsigned)atoi(argv[10])), gm = shifted(nm, 3), gc = shifted(nc, 8);
		{
			File in(argv[11], "rb");
			in.get(cnt.data(), rows), in.get(fill_to.data(), rows), in.get(gm.at, nm), in.get(gs.at, nb);
		}
		lw_select *se = lw_select_create(0, &err);
		if (!se || lw_select_set_tile_frames(se, tile) != LW_OK)
			return 2;
		fill32(gd.at, nb / 4, SENT_DEAD);
		memset(gc.at, 0xee, nc);
		const int rc = lw_select_rows(se, ch, F, gs.at, (const uint8_t *)gm.at, gd.at, want_counts ? (uint64_t *)gc.at : nullptr, rows, cap, cnt.data(),
				fill ? fill_to.data() : nullptr, nullptr);
		printf("RC %d\nLAUNCHES %d\nTILE %u\n", rc, g_log.launches, lw_select_tile_frames(se));
		if (rc == LW_OK && lw_select_last_launches(se) != g_log.launches)
			return 3;
		{
			File out(argv[12], "wb");
			out.put(gd.at, nb), out.put(gc.at, nc);
		}
		if (!guard_intact(gs) || !guard_intact(gd) || !guard_intact(gm) || !guard_intact(gc))
			bad("a store in front of a buffer");
		free(gs.base), free(gd.base), free(gm.base), free(gc.base);
		lw_select_destroy(se);
		return 0;
	}
	if (mode == "far" && argc >= 8) {
		const uint32_t tile = (uint32_t)atoi(argv[2]), F = (uint32_t)atoi(argv[3]);
		const uint64_t base = strtoull(argv[4], nullptr, 10), keep = strtoull(argv[5], nullptr, 10), T = base + keep;
		std::vector<uint8_t> m((size_t)keep);
		std::vector<float> x((size_t)(F * keep)), y((size_t)(F * keep));
		if (base % tile)
			return 2;
		{
			File in(argv[6], "rb");
			in.get(m.data(), m.size()), in.get(x.data(), x.size());
		}
		fill32(y.data(), y.size(), SENT_DEAD);
		lw_select *se = lw_select_create(0, &err);
		if (!se || lw_select_set_tile_frames(se, tile) != LW_OK)
			return 2;
		g_from_frame = base;
		uint64_t K = 0, K0 = 0;
		int rc = 0;
		for (uint32_t g = 0; g < F && rc == 0; g++) { // (a line at a time, as in slide_host.cpp's far)
			const uintptr_t s = (uintptr_t)(x.data() + (size_t)g * keep) - (uintptr_t)base * 4u, d = (uintptr_t)(y.data() + (size_t)g * keep) - (uintptr_t)base * 4u;
			rc = lw_select_rows(se, 1, 1, (const void *)s, (const uint8_t *)((uintptr_t)m.data() - (uintptr_t)base), (void *)d, &K, 1, (size_t)T, &T, nullptr,
					nullptr);
			if (g == 0)
				K0 = K;
			else if (K != K0)
				return 3;
		}
		printf("RC %d\nLAUNCHES %d\n", rc, g_log.launches);
		if (K < base)
			return 3;
		K -= base;
		{
			File out(argv[7], "wb");
			out.put(y.data(), y.size()), out.put(&K, 1);
		}
		lw_select_destroy(se);
		return 0;
	}
	// ---- calls on a small fixture: 3 rows of 2 channels, 5 lines, capacity 3000
	lw_select *se = lw_select_create(0, &err);
	if (!se)
		return 2;
	const size_t cap = 3000;
	std::vector<float> src(3 * 2 * 5 * cap, 0.25f), dst(3 * 2 * 5 * cap, 0.0f);
	std::vector<uint8_t> msk(3 * 2 * cap, 1);
	std::vector<uint64_t> counts(3 * 2, 77);
	uint64_t cnt[3] = {3000, 0, 4}, fill[3] = {3000, 3, 0};
	g_log.run = false;
	if (mode == "two") {
		uint64_t cnt_b[3] = {1, 257, 13};
		int rc = lw_select_rows(se, 2, 5, src.data(), msk.data(), dst.data(), counts.data(), 3, cap, cnt, fill, nullptr);
		printf("RC %d LAST %d\n", rc, lw_select_last_launches(se));
		cnt[0] = 1, fill[1] = 7; // the first call has copied its arrays: the caller's are free
		rc = lw_select_rows(se, 2, 5, src.data(), msk.data(), dst.data(), nullptr, 3, cap, cnt_b, nullptr, nullptr);
		printf("RC %d LAST %d\n", rc, lw_select_last_launches(se));
		g_log.print([](const LwSelectRow &r) { printf(" %llu/%llu", (unsigned long long)r.n, (unsigned long long)r.fill_end); });
	} else if (mode == "refuse" && argc >= 3) {
		const std::string cs = argv[2];
		uint32_t ch = 2, F = 5;
		const void *s = src.data();
		const uint8_t *mk = msk.data();
		void *d = dst.data();
		const uint64_t *n = cnt, *fl = fill;
		size_t rows = 3, c = cap;
		lw_select *h = se;
		if (cs == "null_se")
			h = nullptr;
		else if (cs == "null_n")
			n = nullptr;
		else if (cs == "null_src")
			s = nullptr;
		else if (cs == "null_mask")
			mk = nullptr;
		else if (cs == "null_dst")
			d = nullptr;
		else if (cs == "null_dst_fill_only")
			cnt[0] = cnt[2] = 0, s = nullptr, mk = nullptr, d = nullptr; // nothing to read, but rows 0 and 1 are filled
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
		else if (cs == "ok_most_tiles")
			c = (size_t)1 << 35, ch = 1, F = 1, rows = 1, cnt[0] = 0, fill[0] = ((uint64_t)1024 << 24) - 1024; // 2^24 - 1 tiles: accepted
		else if (cs == "ok_nothing")
			cnt[0] = cnt[2] = 0, fl = nullptr, s = nullptr, mk = nullptr, d = nullptr; // all rows empty, no fill: the counts alone, by a memset
		else if (cs == "ok_no_rows")
			rows = 0, n = nullptr;
		else if (cs == "ok_fill_only")
			cnt[0] = cnt[2] = 0, s = nullptr, mk = nullptr;
		else if (cs != "ok")
			return 2;
		const int rc = lw_select_rows(h, ch, F, s, mk, d, counts.data(), rows, c, n, fl, nullptr);
		printf("RC %d\nLAUNCHES %d\nLAST %d\n", rc, g_log.launches, lw_select_last_launches(se));
		printf("COUNTS");
		for (uint64_t v : counts)
			printf(" %llu", (unsigned long long)v);
		printf("\n");
	} else {
		return 2;
	}
	lw_select_destroy(se);
	return 0;
}
