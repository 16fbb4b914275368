// Segments of a frame mask WITHOUT a GPU: lw_segment.cpp linked against hip_standins.inc (device memory = calloc), and the KERNEL
// source itself, lw_kernels_segment.hip, compiled for the host (LW_SEGMENT_HOST): the stand-ins for the launchers below run it
// workgroup by workgroup, the phases in the kernels' own order (every wave or lane of a phase before the next: the barrier), the
// LDS an allocation of its exact size, so AddressSanitizer sees every load and store the kernels make.  Built with
// -fsanitize=address,undefined; tests/test_host_segment.py drives it.
//   segment_host create DEVICE PON POFF MOFF MON RESERVED   "RC err" (the stand-ins have ONE device, 0)
//   segment_host tile TILE             "RC rc TILE t": lw_segment_set_tile_frames(TILE), then lw_segment_tile_frames
//   segment_host refuse CASE           "RC rc", "LAUNCHES n", "LAST n", "OUT s c m z": whether spans, counts and the smoothed mask
//                                      still hold their fill, and whether the counts are all 0; CASE is one of the calls of main
//   segment_host two                   two calls queued back to back: "ROWS n/fill_end..." per launch, read at the end
//   segment_host run TILE CH ROWS CAP SEGCAP FILL SPANS COUNTS SMOOTH OFF_MASK OFF_SMOOTH PON POFF MOFF MON IN OUT
//                                      IN: u64 n[ROWS], u64 fill_to[ROWS], u8 mask[ROWS][CH][CAP]; OUT: u64 spans[ROWS][CH][SEGCAP][2],
//                                      u64 counts[ROWS][CH], u8 smooth[ROWS][CH][CAP], each sentinel-filled before the call.  FILL,
//                                      SPANS, COUNTS, SMOOTH: 0 = the array is NULL.  The buffers are exact-size, the masks start
//                                      OFF_* BYTES behind a 16-byte boundary and have a guarded front.  "RC rc", "LAUNCHES n", "TILE n"
//   segment_host far TILE BASE KEEP SEGCAP PON POFF MOFF MON IN OUT
//                                      ONE row and channel of T = BASE + KEEP frames, capacity T, of which only frames [BASE, T)
//                                      exist (BASE a multiple of TILE, past 2^32): IN holds u8 mask[KEEP]; the pointers are moved
//                                      BASE frames in front of the data; the tiles whose halo would reach in front of the data
//                                      are not run (tile 0 adds up the list and stores the count all the same).  OUT: u64
//                                      spans[SEGCAP][2], u64 count, u8 smooth[KEEP]
#include "../../include/lewton_amd.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "hip_standins.inc"
#include "kernel_host.hpp"

#define LW_SEGMENT_HOST 1
#include "../../lewton_amd/csrc/lw_kernels_segment.hip"

static LaunchLog<LwSegmentRow> g_log;
static uint64_t g_from_frame = 0; // far: what lies in front of this frame does not exist
static const unsigned char SENT_MASK = 0xa5;
static const uint64_t SENT_SPAN = 0x7e7e7e7e7e7e7e7eull;

static void check(const LwSegmentArgs &a, uint32_t n_rows)
{
	if (!a.rows || n_rows == 0 || n_rows > 65535u || !lw_segment_tile_ok(a.tile) || a.ch == 0 || a.tiles == 0 || a.tiles > LW_SG_MAX_TILES ||
			!a.tile_counts || a.pad_onset > LW_SG_MAX_SPAN || a.pad_offset > LW_SG_MAX_SPAN || a.min_off > LW_SG_MAX_SPAN || a.min_on > LW_SG_MAX_SPAN ||
			(a.d_spans && !a.seg_capacity))
		bad("arguments");
}

#define WAVES(stmt) \
	for (uint32_t wave = 0; wave < LW_SG_WAVES; wave++) \
	stmt
#define LANES(stmt) \
	for (uint32_t tid = 0; tid < LW_SG_THREADS; tid++) \
	stmt

static bool out_of_reach(const LwSgTile &t) // far: the tile's window would begin in front of the data
{
	return g_from_frame && t.t0 < g_from_frame + t.halo;
}

// lw_sg_rule
static void rule(const LwSegmentArgs &a, const LwSgTile &t, LwSgLds &l)
{
	WAVES(lw_sg_load(a, t, l, wave, 0u);)
	WAVES(lw_sg_pad(a, t, l, wave, 0u);)
	WAVES(lw_sg_fill(a, t, l, wave, 0u);)
	WAVES(lw_sg_drop(a, t, l, wave, 0u);)
	WAVES(lw_sg_edges(t, l, wave, 0u);)
}

hipError_t lw_launch_segment_count(const LwSegmentArgs &a, uint32_t n_rows, hipStream_t)
{
	g_log.launch(a.rows + a.row0, n_rows);
	check(a, n_rows);
	if (!a.mask || (!a.d_spans && !a.d_counts))
		bad("arguments of the count");
	if (!g_log.run)
		return hipSuccess;
	LwSgLds *l = (LwSgLds *)malloc(sizeof(LwSgLds));
	for (uint32_t bz = 0; bz < n_rows; bz++)
		for (uint32_t by = 0; by < a.ch; by++)
			for (uint32_t bx = 0; bx < a.tiles; bx++) {
				LwSgTile t;
				lw_sg_tile(a, bx, by, bz, t);
				if (!t.nt || out_of_reach(t))
					continue;
				memset(l, 0xff, sizeof(LwSgLds));
				rule(a, t, *l);
				a.tile_counts[t.list_at + t.tile_i] = lw_sg_starts(t, *l);
			}
	free(l);
	return hipSuccess;
}

hipError_t lw_launch_segment(const LwSegmentArgs &a, uint32_t n_rows, hipStream_t)
{
	g_log.launch(a.rows + a.row0, n_rows);
	check(a, n_rows);
	if (!a.d_spans && !a.d_counts && !a.d_smooth)
		bad("a launch with nothing to write");
	if (!g_log.run)
		return hipSuccess;
	LwSgLds *l = (LwSgLds *)malloc(sizeof(LwSgLds));
	for (uint32_t bz = 0; bz < n_rows; bz++)
		for (uint32_t by = 0; by < a.ch; by++)
			for (uint32_t bx = 0; bx < a.tiles; bx++) {
				LwSgTile t;
				lw_sg_tile(a, bx, by, bz, t);
				const bool count = lw_sg_owes_count(a, t);
				bool spans = lw_sg_owes_spans(a, t), smooth = lw_sg_owes_smooth(a, t);
				if (out_of_reach(t))
					spans = smooth = false;
				if (!count && !spans && !smooth)
					continue;
				memset(l, 0xff, sizeof(LwSgLds));
				uint64_t base = 0;
				if (count || spans) {
					LANES(lw_sg_partial(a, t, *l, tid);)
					LANES(lw_sg_fold(*l, tid);)
					base = lw_sg_sum(*l);
					if (count)
						a.d_counts[t.cnt_at] = base;
					if (t.tile_i == 0)
						base = 0;
				}
				const bool passes = lw_sg_passes(a, t) && (spans || smooth);
				if (passes)
					rule(a, t, *l);
				if (spans)
					LANES(lw_sg_spans(a, t, *l, base, tid);)
				if (smooth)
					LANES(lw_sg_smooth(a, t, *l, passes, tid);)
			}
	free(l);
	return hipSuccess;
}

static lw_segment_params params(char **argv, uint32_t reserved = 0)
{
	lw_segment_params p;
	p.pad_onset = (uint32_t)strtoul(argv[0], nullptr, 10), p.pad_offset = (uint32_t)strtoul(argv[1], nullptr, 10);
	p.min_off = (uint32_t)strtoul(argv[2], nullptr, 10), p.min_on = (uint32_t)strtoul(argv[3], nullptr, 10), p.reserved = reserved;
	return p;
}

template <class T>
static bool all_are(const std::vector<T> &v, T x)
{
	for (const T &e : v)
		if (e != x)
			return false;
	return true;
}

int main(int argc, char **argv)
{
	if (argc < 2)
		return 2;
	const std::string mode = argv[1];
	int err = 0;
	lw_segment_params dflt{2u, 8u, 10u, 5u, 0u};
	if (mode == "create" && argc >= 8) {
		const lw_segment_params p = params(argv + 3, (uint32_t)strtoul(argv[7], nullptr, 10));
		lw_segment *sg = lw_segment_create(atoi(argv[2]), &p, &err);
		printf("RC %d\n", err);
		if ((sg == nullptr) != (err != 0))
			return 3;
		if (sg && (lw_segment_tile_frames(sg) != LW_SG_TILE || lw_segment_last_launches(sg) != -1))
			return 3;
		if (lw_segment_tile_frames(nullptr) != 0 || lw_segment_set_tile_frames(nullptr, 256) != LW_ERR_NULL_ARG || lw_segment_last_launches(nullptr) != -1 ||
				lw_segment_create(0, nullptr, &err) != nullptr || err != LW_ERR_NULL_ARG)
			return 3;
		lw_segment_destroy(sg);
		lw_segment_destroy(nullptr);
		return 0;
	}
	if (mode == "tile" && argc >= 3) {
		lw_segment *sg = lw_segment_create(0, &dflt, &err);
		if (!sg)
			return 2;
		const int rc = lw_segment_set_tile_frames(sg, (uint32_t)atoi(argv[2]));
		printf("RC %d TILE %u\n", rc, lw_segment_tile_frames(sg));
		lw_segment_destroy(sg);
		return 0;
	}
	if (mode == "run" && argc >= 19) {
		const uint32_t tile = (uint32_t)atoi(argv[2]), ch = (uint32_t)atoi(argv[3]);
		const size_t rows = (size_t)atoll(argv[4]), cap = (size_t)atoll(argv[5]), segcap = (size_t)atoll(argv[6]);
		const bool fill = atoi(argv[7]) != 0, want_spans = atoi(argv[8]) != 0, want_counts = atoi(argv[9]) != 0, want_smooth = atoi(argv[10]) != 0;
		const size_t nm = rows * ch * cap, ns = rows * ch * segcap * 2, nc = rows * ch;
		std::vector<uint64_t> cnt(rows + 1), fill_to(rows + 1);
		const Guarded gm = shifted(nm, (unsigned)atoi(argv[11])), go = shifted(nm, (unsigned)atoi(argv[12])), gs = shifted(ns * 8, 0), gc = shifted(nc * 8, 8);
		{
			File in(argv[17], "rb");
			in.get(cnt.data(), rows), in.get(fill_to.data(), rows), in.get(gm.at, nm);
		}
		const lw_segment_params p = params(argv + 13);
		lw_segment *sg = lw_segment_create(0, &p, &err);
		if (!sg || lw_segment_set_tile_frames(sg, tile) != LW_OK)
			return 2;
		memset(go.at, SENT_MASK, nm);
		for (size_t i = 0; i < ns; i++)
			gs.as<uint64_t>()[i] = SENT_SPAN;
		for (size_t i = 0; i < nc; i++)
			gc.as<uint64_t>()[i] = SENT_SPAN;
		const int rc = lw_segment_rows(sg, ch, (const uint8_t *)gm.at, want_spans ? gs.as<uint64_t>() : nullptr, want_counts ? gc.as<uint64_t>() : nullptr,
				want_smooth ? (uint8_t *)go.at : nullptr, rows, cap, segcap, cnt.data(), fill ? fill_to.data() : nullptr, nullptr);
		printf("RC %d\nLAUNCHES %d\nTILE %u\n", rc, g_log.launches, lw_segment_tile_frames(sg));
		if (rc == LW_OK && lw_segment_last_launches(sg) != g_log.launches)
			return 3;
		{
			File out(argv[18], "wb");
			out.put(gs.as<uint64_t>(), ns), out.put(gc.as<uint64_t>(), nc), out.put(go.at, nm);
		}
		if (!guard_intact(gm) || !guard_intact(go) || !guard_intact(gs) || !guard_intact(gc))
			bad("a store in front of a buffer");
		free(gm.base), free(go.base), free(gs.base), free(gc.base);
		lw_segment_destroy(sg);
		return 0;
	}
	if (mode == "far" && argc >= 12) {
		const uint32_t tile = (uint32_t)atoi(argv[2]);
		const uint64_t base = strtoull(argv[3], nullptr, 10), keep = strtoull(argv[4], nullptr, 10), T = base + keep;
		const size_t segcap = (size_t)atoll(argv[5]);
		if (base % tile || keep <= tile)
			return 2;
		std::vector<uint8_t> m((size_t)keep), o((size_t)keep, SENT_MASK);
		std::vector<uint64_t> spans(segcap * 2, SENT_SPAN);
		uint64_t count = SENT_SPAN;
		{
			File in(argv[10], "rb");
			in.get(m.data(), m.size());
		}
		const lw_segment_params p = params(argv + 6);
		lw_segment *sg = lw_segment_create(0, &p, &err);
		if (!sg || lw_segment_set_tile_frames(sg, tile) != LW_OK)
			return 2;
		g_from_frame = base;
		const uintptr_t s = (uintptr_t)m.data() - (uintptr_t)base, d = (uintptr_t)o.data() - (uintptr_t)base;
		const int rc = lw_segment_rows(sg, 1, (const uint8_t *)s, spans.data(), &count, (uint8_t *)d, 1, (size_t)T, segcap, &T, nullptr, nullptr);
		printf("RC %d\nLAUNCHES %d\n", rc, g_log.launches);
		{
			File out(argv[11], "wb");
			out.put(spans.data(), spans.size()), out.put(&count, 1), out.put(o.data(), o.size());
		}
		lw_segment_destroy(sg);
		return 0;
	}
	// ---- calls on a small fixture: 3 rows of 2 channels, capacity 3000, 8 spans per row and channel
	const size_t cap = 3000;
	std::vector<uint8_t> msk(3 * 2 * cap, 1), smo(3 * 2 * cap, 7);
	std::vector<uint64_t> sp(3 * 2 * 8 * 2, 77), kc(3 * 2, 77);
	uint64_t cnt[3] = {3000, 0, 4}, fill[3] = {3000, 3, 0};
	g_log.run = false;
	if (mode == "two") {
		lw_segment *sg = lw_segment_create(0, &dflt, &err);
		if (!sg)
			return 2;
		uint64_t cnt_b[3] = {1, 257, 13};
		int rc = lw_segment_rows(sg, 2, msk.data(), sp.data(), kc.data(), smo.data(), 3, cap, 8, cnt, fill, nullptr);
		printf("RC %d LAST %d\n", rc, lw_segment_last_launches(sg));
		cnt[0] = 1, fill[1] = 7; // the first call has copied its arrays: the caller's are free
		rc = lw_segment_rows(sg, 2, msk.data(), nullptr, nullptr, smo.data(), 3, cap, 8, cnt_b, nullptr, nullptr);
		printf("RC %d LAST %d\n", rc, lw_segment_last_launches(sg));
		g_log.print([](const LwSegmentRow &r) { printf(" %llu/%llu", (unsigned long long)r.n, (unsigned long long)r.fill_end); });
		lw_segment_destroy(sg);
		return 0;
	}
	if (mode != "refuse" || argc < 3)
		return 2;
	const std::string cs = argv[2];
	uint32_t ch = 2;
	const uint8_t *mk = msk.data();
	uint64_t *s = sp.data(), *k = kc.data();
	uint8_t *o = smo.data();
	const uint64_t *n = cnt, *fl = fill;
	size_t rows = 3, c = cap, segcap = 8;
	bool null_sg = false;
	std::vector<uint64_t> many;
	if (cs == "null_sg")
		null_sg = true;
	else if (cs == "null_n")
		n = nullptr;
	else if (cs == "null_mask")
		mk = nullptr;
	else if (cs == "n_over")
		cnt[2] = cap + 1; // (the LAST row: every row is checked before anything is queued)
	else if (cs == "fill_over")
		fill[2] = cap + 1;
	else if (cs == "fill_over_no_smooth")
		fill[2] = cap + 1, o = nullptr; // (refused whether or not anything would be filled)
	else if (cs == "ch0")
		ch = 0;
	else if (cs == "ch256")
		ch = 256;
	else if (cs == "segcap0")
		segcap = 0;
	else if (cs == "too_large")
		c = (size_t)1 << 63, fl = nullptr;
	else if (cs == "too_large_spans")
		segcap = (size_t)1 << 60;
	else if (cs == "too_many_tiles") // 2^24 tiles of 1024 frames to fill, one more than a grid counts
		c = (size_t)1 << 35, ch = 1, rows = 1, cnt[0] = 0, fill[0] = (uint64_t)1024 << 24;
	else if (cs == "ok_most_tiles")
		c = (size_t)1 << 35, ch = 1, rows = 1, cnt[0] = 0, fill[0] = ((uint64_t)1024 << 24) - 1024; // 2^24 - 1 tiles: accepted (nothing runs here)
	else if (cs == "ok_segcap0_no_spans")
		segcap = 0, s = nullptr;
	else if (cs == "ok_smooth_only")
		s = nullptr, k = nullptr; // nothing needs the list: the second launch alone
	else if (cs == "ok_counts_only")
		s = nullptr, o = nullptr;
	else if (cs == "ok_spans_only")
		k = nullptr, o = nullptr;
	else if (cs == "ok_no_frames")
		cnt[0] = cnt[2] = 0, mk = nullptr; // no row has a frame: nothing is counted, the second launch fills and stores K = 0
	else if (cs == "ok_nothing")
		cnt[0] = cnt[2] = 0, fl = nullptr, mk = nullptr; // all rows empty, no fill: the counts by a memset
	else if (cs == "ok_fill_without_smooth")
		cnt[0] = cnt[2] = 0, mk = nullptr, o = nullptr; // fill_to means nothing without the smoothed mask
	else if (cs == "ok_no_outputs")
		s = nullptr, k = nullptr, o = nullptr;
	else if (cs == "ok_no_rows")
		rows = 0, n = nullptr;
	else if (cs == "ok_rows65536") // two launch groups
		rows = 65536, many.assign(rows, 0), many[65535] = 4, n = many.data(), fl = nullptr, ch = 1, c = 4, segcap = 1, s = nullptr, o = nullptr, k = nullptr,
		sp.assign(rows * 2, 77), s = sp.data();
	else if (cs != "ok")
		return 2;
	lw_segment *sg = lw_segment_create(0, &dflt, &err);
	if (!sg)
		return 2;
	const int rc = lw_segment_rows(null_sg ? nullptr : sg, ch, mk, s, k, o, rows, c, segcap, n, fl, nullptr);
	printf("RC %d\nLAUNCHES %d\nLAST %d\n", rc, g_log.launches, lw_segment_last_launches(sg));
	printf("OUT %d %d %d %d\n", (int)all_are<uint64_t>(sp, 77), (int)all_are<uint64_t>(kc, 77), (int)all_are<uint8_t>(smo, 7), (int)all_are<uint64_t>(kc, 0));
	lw_segment_destroy(sg);
	return 0;
}
