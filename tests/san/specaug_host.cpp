// SpecAugment WITHOUT a GPU: lw_specaug.cpp linked against hip_standins.inc (device memory = calloc), and the KERNEL source itself,
// lw_kernels_specaug.hip, compiled for the host (LW_KERNEL_HOST): the stand-in for the launcher below runs it workgroup by
// workgroup through lw_sa_workgroup, the kernels' own driver of the phases (every lane of a phase before the next: the barrier),
// the LDS an allocation of exactly the masks' size, so AddressSanitizer sees every load and store the kernel makes.  Built with
// -fsanitize=address,undefined;
// tests/test_host_specaug.py drives it.  P below is the twelve numbers of lw_specaug_params in the structure's order:
// SEED NUM_T MIN_T MAX_T RATIO_NUM RATIO_DEN NUM_F MIN_F MAX_F PER_CHANNEL FILL RESERVED, FILL as the bits of the float32.
//   specaug_host philox C0 C1 C2 C3 K0 K1      "X x0 x1 x2 x3" in hex: lw_philox
//   specaug_host below IN OUT                  IN: u64 n, n x (u64 x, u64 m); OUT: n x (u64 lw_below32(x, m) of the low words, u64 lw_below64)
//   specaug_host create DEVICE P               "RC err" (the stand-ins have ONE device, 0)
//   specaug_host tile TILE                     "RC rc TILE t": lw_specaug_set_tile_frames(TILE), then lw_specaug_tile_frames
//   specaug_host plans P IN OUT                IN: u64 n, n x (u64 id, u64 group, u64 T, u64 F); OUT: n x (i64 rc, then [masks][2] i64 of
//                                              lw_specaug_plan, sentinel-filled before the call)
//   specaug_host refuse CASE                   "RC rc", "LAUNCHES n", "LAST n", "DST untouched", "SPANS untouched": CASE is one of the
//                                              calls of main below
//   specaug_host two                           two calls queued back to back: "ROWS n/fill_end/id ..." per launch, read at the end
//   specaug_host run TILE CH F ROWS CAP FILL IDS IN_PLACE WANT_SPANS OFF_SRC OFF_DST P IN OUT
//                                              IN: u64 n[ROWS], u64 fill_to[ROWS], u64 ids[ROWS], u32 x[ROWS][CH][F][CAP]; OUT: the
//                                              destination u32 [ROWS][CH][F][CAP] (out of place: sentinel-filled before the call; in
//                                              place: the source's buffer), then the spans i64 [ROWS][G][masks][2] (sentinel-filled
//                                              too).  FILL, IDS, WANT_SPANS: 0 = the array is NULL.  The buffers are exact-size,
//                                              start OFF_* BYTES behind a 16-byte boundary and have a guarded front; out of place the
//                                              source is poisoned at and beyond every line's T.  "RC rc", "LAUNCHES n", "TILE n"
#include "../../include/lewton_amd.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "hip_standins.inc"
#include "kernel_host.hpp"

#define LW_KERNEL_HOST 1
#include "../../lewton_amd/csrc/lw_kernels_specaug.hip"

static LaunchLog<LwSaRow> g_log;
static const int64_t SENT_SPAN = -0x5a5a5a5a5a5a5a5aLL;

hipError_t lw_launch_specaug(const LwSaArgs &a, uint32_t n_rows, hipStream_t)
{
	g_log.launch(a.rows + a.row0, n_rows);
	const uint32_t masks = a.rule.num_t + a.rule.num_f;
	if (!a.rows || n_rows == 0 || n_rows > 65535u || !lw_sa_tile_ok(a.tile) || a.ch == 0 || a.F == 0 || a.tiles == 0 || (uint64_t)a.tiles * a.F > LW_SA_MAX_TILES ||
			a.rule.num_t > LW_SA_MAX_MASKS || a.rule.num_f > LW_SA_MAX_MASKS || a.per_channel > 1u)
		bad("arguments");
	if (!g_log.run)
		return hipSuccess;
	const bool in_place = a.src == a.dst;
	LwSaLds *l = (LwSaLds *)malloc(masks ? masks * sizeof(l->span[0]) : 1); // exactly the masks' pairs
	for (uint32_t bz = 0; bz < n_rows; bz++)
		for (uint32_t by = 0; by < a.ch; by++)
			for (uint32_t bx = 0; bx < a.tiles * a.F; bx++) {
				memset((void *)l, 0xff, masks * sizeof(l->span[0]));
				const auto lanes = [](const auto &phase, bool) { // every lane of a phase before the next: the barrier
					for (uint32_t tid = 0; tid < LW_SA_THREADS; tid++)
						phase(tid);
				};
				in_place ? lw_sa_workgroup<true>(a, *l, bx, by, bz, lanes) : lw_sa_workgroup<false>(a, *l, bx, by, bz, lanes);
			}
	free(l);
	return hipSuccess;
}

static uint64_t u64_of(const char *s)
{
	return strtoull(s, nullptr, 10);
}

static lw_specaug_params params(char **v) // the twelve numbers of P
{
	lw_specaug_params p;
	memset(&p, 0, sizeof p);
	p.seed = u64_of(v[0]);
	p.num_t = (uint32_t)u64_of(v[1]), p.min_t = (uint32_t)u64_of(v[2]), p.max_t = (uint32_t)u64_of(v[3]);
	p.ratio_num = (uint32_t)u64_of(v[4]), p.ratio_den = (uint32_t)u64_of(v[5]);
	p.num_f = (uint32_t)u64_of(v[6]), p.min_f = (uint32_t)u64_of(v[7]), p.max_f = (uint32_t)u64_of(v[8]);
	p.per_channel = (uint32_t)u64_of(v[9]);
	const uint32_t bits = (uint32_t)u64_of(v[10]);
	memcpy(&p.fill, &bits, 4);
	p.reserved = (uint32_t)u64_of(v[11]);
	return p;
}

int main(int argc, char **argv)
{
	if (argc < 2)
		return 2;
	const std::string mode = argv[1];
	int err = 0;
	lw_specaug_params dflt;
	memset(&dflt, 0, sizeof dflt);
	dflt.seed = 2024, dflt.num_t = 2, dflt.max_t = 50, dflt.num_f = 2, dflt.max_f = 10;
	if (mode == "philox" && argc >= 8) {
		uint32_t c[4], k[2], x[4];
		for (int i = 0; i < 4; i++)
			c[i] = (uint32_t)u64_of(argv[2 + i]);
		k[0] = (uint32_t)u64_of(argv[6]), k[1] = (uint32_t)u64_of(argv[7]);
		lw_philox(c, k, x);
		printf("X %08x %08x %08x %08x\n", x[0], x[1], x[2], x[3]);
		return 0;
	}
	if (mode == "below" && argc >= 4) {
		File in(argv[2], "rb"), out(argv[3], "wb");
		uint64_t n = 0;
		in.get(&n, 1);
		for (uint64_t i = 0; i < n; i++) {
			uint64_t xm[2], r[2];
			in.get(xm, 2);
			r[0] = lw_below32((uint32_t)xm[0], (uint32_t)xm[1]), r[1] = lw_below64(xm[0], xm[1]);
			out.put(r, 2);
		}
		return 0;
	}
	if (mode == "create" && argc >= 15) {
		const lw_specaug_params p = params(argv + 3);
		lw_specaug *sa = lw_specaug_create(atoi(argv[2]), &p, &err);
		printf("RC %d\n", err);
		if ((sa == nullptr) != (err != 0))
			return 3;
		if (sa && (lw_specaug_tile_frames(sa) != LW_SA_TILE || lw_specaug_last_launches(sa) != -1))
			return 3;
		int64_t sp[4 * LW_SA_MAX_MASKS];
		if (lw_specaug_tile_frames(nullptr) != 0 || lw_specaug_set_tile_frames(nullptr, 256) != LW_ERR_NULL_ARG || lw_specaug_last_launches(nullptr) != -1 ||
				lw_specaug_plan(nullptr, 0, 0, 1, 1, sp) != LW_ERR_NULL_ARG || (sa && lw_specaug_plan(sa, 0, 0, 1, 1, nullptr) != LW_ERR_NULL_ARG) ||
				lw_specaug_create(0, nullptr, &err) != nullptr || err != LW_ERR_NULL_ARG)
			return 3;
		lw_specaug_destroy(sa);
		return 0;
	}
	if (mode == "tile" && argc >= 3) {
		lw_specaug *sa = lw_specaug_create(0, &dflt, &err);
		if (!sa)
			return 2;
		const int rc = lw_specaug_set_tile_frames(sa, (uint32_t)u64_of(argv[2]));
		printf("RC %d TILE %u\n", rc, lw_specaug_tile_frames(sa));
		lw_specaug_destroy(sa);
		return 0;
	}
	if (mode == "plans" && argc >= 16) {
		const lw_specaug_params p = params(argv + 2);
		lw_specaug *sa = lw_specaug_create(0, &p, &err);
		if (!sa)
			return 2;
		File in(argv[14], "rb"), out(argv[15], "wb");
		uint64_t n = 0;
		in.get(&n, 1);
		const size_t masks = p.num_t + p.num_f;
		std::vector<int64_t> sp(2 * masks + 1);
		for (uint64_t i = 0; i < n; i++) {
			uint64_t q[4];
			in.get(q, 4);
			std::fill(sp.begin(), sp.end(), SENT_SPAN);
			const int64_t rc = lw_specaug_plan(sa, q[0], (uint32_t)(q[1] > UINT32_MAX ? UINT32_MAX : q[1]), q[2], (uint32_t)(q[3] > UINT32_MAX ? UINT32_MAX : q[3]), sp.data());
			if (sp[2 * masks] != SENT_SPAN)
				bad("lw_specaug_plan wrote behind its pairs");
			out.put(&rc, 1), out.put(sp.data(), 2 * masks);
		}
		lw_specaug_destroy(sa);
		return 0;
	}
	if (mode == "run" && argc >= 27) {
		const uint32_t tile = (uint32_t)atoi(argv[2]), ch = (uint32_t)atoi(argv[3]), F = (uint32_t)atoi(argv[4]);
		const size_t rows = (size_t)atoll(argv[5]), cap = (size_t)atoll(argv[6]);
		const bool fill = atoi(argv[7]) != 0, with_ids = atoi(argv[8]) != 0, in_place = atoi(argv[9]) != 0, want_spans = atoi(argv[10]) != 0;
		const lw_specaug_params p = params(argv + 13);
		const size_t ne = rows * ch * F * cap, nb = ne * 4, masks = p.num_t + p.num_f, G = p.per_channel ? ch : 1, ns = rows * G * masks * 2;
		std::vector<uint64_t> cnt(rows + 1), fill_to(rows + 1), ids(rows + 1);
		const Guarded gs = shifted(nb, (unsigned)atoi(argv[11])), gd = shifted(in_place ? 0 : nb, (unsigned)atoi(argv[12])), gp = shifted(ns * 8, 8);
		{
			File in(argv[25], "rb");
			in.get(cnt.data(), rows), in.get(fill_to.data(), rows), in.get(ids.data(), rows), in.get(gs.at, nb);
		}
		lw_specaug *sa = lw_specaug_create(0, &p, &err);
		if (!sa || lw_specaug_set_tile_frames(sa, tile) != LW_OK)
			return 2;
		if (!in_place) {
			fill32(gd.at, ne, SENT_ABC);
			for (size_t ln = 0; ln < rows * ch * F; ln++) { // nothing at or beyond T of a line may be read
				const uint64_t T = cnt[ln / ((size_t)ch * F)];
				if (T > cap)
					continue; // (a call that is refused)
				const uintptr_t b = ((uintptr_t)gs.at + (ln * cap + T) * 4 + 7u) & ~(uintptr_t)7, e = ((uintptr_t)gs.at + (ln + 1) * cap * 4) & ~(uintptr_t)7;
				if (b < e)
					ASAN_POISON_MEMORY_REGION((void *)b, e - b);
			}
		}
		for (size_t i = 0; i < ns; i++)
			gp.as<int64_t>()[i] = SENT_SPAN;
		void *dst = in_place ? (void *)gs.at : (void *)gd.at;
		const int rc = lw_specaug_rows(sa, ch, F, gs.at, dst, rows, cap, cnt.data(), fill ? fill_to.data() : nullptr, with_ids ? ids.data() : nullptr,
				want_spans ? gp.as<int64_t>() : nullptr, nullptr);
		printf("RC %d\nLAUNCHES %d\nTILE %u\n", rc, g_log.launches, lw_specaug_tile_frames(sa));
		if (rc == LW_OK && lw_specaug_last_launches(sa) != g_log.launches)
			return 3;
		ASAN_UNPOISON_MEMORY_REGION(gs.at, nb);
		{
			File out(argv[26], "wb");
			out.put((const char *)dst, nb), out.put(gp.at, ns * 8);
		}
		if (!guard_intact(gs) || !guard_intact(gd) || !guard_intact(gp))
			bad("a store in front of a buffer");
		free(gs.base), free(gd.base), free(gp.base);
		lw_specaug_destroy(sa);
		return 0;
	}
	// ---- calls on a small fixture: 3 rows of 2 channels, 5 lines, capacity 3000
	const size_t cap = 3000;
	std::vector<uint32_t> src(3 * 2 * 5 * cap, 0x3e800000u), dstv(3 * 2 * 5 * cap, SENT_ABC);
	std::vector<int64_t> spans(3 * 2 * 64 * 2, SENT_SPAN);
	uint64_t cnt[3] = {3000, 0, 4}, fill[3] = {3000, 3, 0}, idv[3] = {7, (uint64_t)1 << 40, 0};
	g_log.run = false;
	if (mode == "two") {
		lw_specaug *sa = lw_specaug_create(0, &dflt, &err);
		if (!sa)
			return 2;
		uint64_t cnt_b[3] = {1, 257, 13};
		int rc = lw_specaug_rows(sa, 2, 5, src.data(), dstv.data(), 3, cap, cnt, fill, idv, spans.data(), nullptr);
		printf("RC %d LAST %d\n", rc, lw_specaug_last_launches(sa));
		cnt[0] = 1, fill[1] = 7, idv[0] = 99; // the first call has copied its arrays: the caller's are free
		rc = lw_specaug_rows(sa, 2, 5, src.data(), src.data(), 3, cap, cnt_b, nullptr, nullptr, nullptr, nullptr);
		printf("RC %d LAST %d\n", rc, lw_specaug_last_launches(sa));
		g_log.print([](const LwSaRow &r) { printf(" %llu/%llu/%llu", (unsigned long long)r.n, (unsigned long long)r.fill_end, (unsigned long long)r.id); });
		lw_specaug_destroy(sa);
		return 0;
	}
	if (mode != "refuse" || argc < 3)
		return 2;
	const std::string cs = argv[2];
	uint32_t ch = 2, F = 5;
	const void *s = src.data();
	void *d = dstv.data();
	const uint64_t *n = cnt, *fl = fill, *id = idv;
	int64_t *sp = spans.data();
	size_t rows = 3, c = cap;
	bool null_sa = false;
	std::vector<uint64_t> many;
	if (cs == "null_sa")
		null_sa = true;
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
	else if (cs == "too_many_tiles_by_lines") // 2^23 tiles in each of two lines
		c = (size_t)1 << 34, ch = 1, F = 2, rows = 1, cnt[0] = 0, fill[0] = (uint64_t)1024 << 23;
	else if (cs == "ok_most_tiles")
		c = (size_t)1 << 35, ch = 1, F = 1, rows = 1, cnt[0] = 0, fill[0] = ((uint64_t)1024 << 24) - 1024; // 2^24 - 1 tiles: accepted
	else if (cs == "ok_in_place")
		d = src.data();
	else if (cs == "ok_no_rows")
		rows = 0, n = nullptr;
	else if (cs == "ok_no_masks_in_place") // no masks configured, no fill span, no spans owed (there are none): nothing can be written
		dflt.num_t = dflt.num_f = 0, d = src.data(), fl = nullptr;
	else if (cs == "ok_no_masks_in_place_fill")
		dflt.num_t = dflt.num_f = 0, d = src.data();
	else if (cs == "ok_no_masks_out_of_place") // a copy and the fill
		dflt.num_t = dflt.num_f = 0;
	else if (cs == "ok_nothing") // all rows empty, no fill, no spans
		cnt[0] = cnt[2] = 0, fl = nullptr, s = nullptr, d = nullptr, sp = nullptr;
	else if (cs == "ok_nothing_but_spans") // ... with spans: rows with T == 0 are included
		cnt[0] = cnt[2] = 0, fl = nullptr, s = nullptr, d = nullptr;
	else if (cs == "ok_in_place_no_frames") // masks, but no row has a frame, and no fill span
		cnt[0] = cnt[2] = 0, fl = nullptr, d = src.data(), sp = nullptr;
	else if (cs == "ok_fill_only")
		cnt[0] = cnt[2] = 0, s = nullptr; // no row has a frame: nothing is read
	else if (cs == "ok_rows65535" || cs == "ok_rows65536") // one launch, two launches
		rows = cs == "ok_rows65535" ? 65535 : 65536, many.assign(rows, 0), many[rows - 1] = 4, n = many.data(), fl = nullptr, id = nullptr, ch = 1, F = 1, c = 4,
		sp = nullptr;
	else if (cs != "ok")
		return 2;
	lw_specaug *sa = lw_specaug_create(0, &dflt, &err);
	if (!sa || lw_specaug_set_tile_frames(sa, 1024) != LW_OK) // (the cases that count tiles count tiles of 1024 frames)
		return 2;
	const int rc = lw_specaug_rows(null_sa ? nullptr : sa, ch, F, s, d, rows, c, n, fl, id, sp, nullptr);
	printf("RC %d\nLAUNCHES %d\nLAST %d\n", rc, g_log.launches, lw_specaug_last_launches(sa));
	bool dst_ok = true, sp_ok = true;
	for (uint32_t v : dstv)
		dst_ok = dst_ok && v == SENT_ABC;
	for (int64_t v : spans)
		sp_ok = sp_ok && v == SENT_SPAN;
	printf("DST %s\nSPANS %s\n", dst_ok ? "untouched" : "written", sp_ok ? "untouched" : "written");
	lw_specaug_destroy(sa);
	return 0;
}
