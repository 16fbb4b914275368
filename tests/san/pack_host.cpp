// Frame-major model input WITHOUT a GPU: lw_pack.cpp linked against hip_standins.inc (device memory = calloc), and the KERNEL
// source itself, lw_kernels_pack.hip, compiled for the host (LW_PACK_HOST): the stand-in for the launcher below runs it
// workgroup by workgroup, the phases in the kernel's own order (every lane of a phase before the next: the barrier), the LDS image
// an exact-size allocation, so AddressSanitizer sees every load and store the kernel makes.  Built with
// -fsanitize=address,undefined; tests/test_host_pack.py drives it.
//   pack_host create F LEFT RIGHT STRIDE EDGE DTYPE PAD [DEVICE]   "RC err" (PAD: a number or "nan"; the stand-ins have ONE device, 0)
//   pack_host frames LEFT RIGHT STRIDE EDGE      "T_OUT ..." of lw_pack_frames for T = 0 .. 200
//   pack_host plan F LEFT RIGHT STRIDE           "TILE t PITCH p LINES l LDS b"
//   pack_host convert DTYPE IN OUT               lw_pack_convert of every f32 of IN (raw) into OUT (u32 each)
//   pack_host refuse CASE                        "RC rc", "LAUNCHES n", "LAST n": CASE is one of the refusals of lw_pack_rows (main below)
//   pack_host two                                two calls queued back to back: "ROWS n/n_out/fill_end..." per launch, read at the end
//   pack_host run F LEFT RIGHT STRIDE EDGE DTYPE CH ROWS CAP OUT_CAP FILL SHIFT SCALE MASK OFF_SRC OFF_DST IN OUT
//                                   IN: u64 n[ROWS], u64 fill_to[ROWS], f32 shift[D], f32 scale[D], f32 pad, f32 x[ROWS][CH][F][CAP];
//                                   OUT: the destination, sentinel-filled before the call, then the mask.  FILL, SHIFT, SCALE, MASK:
//                                   0 = the array is NULL.  The buffers are exact-size, start OFF_* BYTES behind a 16-byte boundary
//                                   and have a guarded front.  "RC rc", "LAUNCHES n", "TILE n", "VEC v" (the last launch's)
#include "../../include/lewton_amd.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "hip_standins.inc"
#include "kernel_host.hpp"

#define LW_PACK_HOST 1
#include "../../lewton_amd/csrc/lw_kernels_pack.hip"

static LaunchLog<LwPackRow> g_log;
static uint32_t g_vec = 0;

// one workgroup, as lw_pk_block runs it on the device
template <int E>
static void block(const LwPackArgs &a, const LwPkTile &t, const uint32_t *src, void *dst, uint32_t *img)
{
	if (t.fill_hi > t.fill_lo)
		for (uint32_t tid = 0; tid < LW_PK_THREADS; tid++)
			lw_pk_fill<E>(a, t, dst, tid);
	if (!t.nu)
		return;
	for (uint32_t f0 = 0; f0 < a.F; f0 += LW_PK_GROUP) {
		const uint32_t left = a.F - f0, G = left < LW_PK_GROUP ? left : LW_PK_GROUP;
		for (uint32_t i = 0; i < a.plan.lds / 4u; i++)
			img[i] = 0x7fc0bad0u; // what a stale image would show
		for (uint32_t tid = 0; tid < LW_PK_THREADS; tid++)
			lw_pk_load(a, t, src, img, f0, G, tid);
		for (uint32_t tid = 0; tid < LW_PK_THREADS; tid++) // (behind the barrier)
			lw_pk_store<E>(a, t, img, dst, f0, G, tid);
	}
}

hipError_t lw_launch_pack(const LwPackArgs &a, const float *src, void *dst, uint8_t *mask, uint32_t tiles, uint32_t n_rows, hipStream_t)
{
	g_log.launch(a.rows + a.row0, n_rows);
	g_vec = a.vec;
	const LwPackPlan p = lw_pack_plan(a.F, a.W, a.stride);
	const uint32_t E = a.dtype == LW_PK_F32 ? 4u : 8u;
	if (!a.rows || n_rows == 0 || n_rows > 65535u || tiles == 0 || tiles > LW_PK_MAX_TILES || !dst || a.D != a.W * a.F || p.tile != a.plan.tile ||
			p.pitch != a.plan.pitch || p.lines != a.plan.lines || p.lds != a.plan.lds || (a.vec && (a.F % E || ((uintptr_t)dst & 15u))))
		bad("arguments");
	if (!g_log.run)
		return hipSuccess;
	uint32_t *img = (uint32_t *)malloc(a.plan.lds); // exact size: one dword beyond the image is a report
	for (uint32_t bz = 0; bz < n_rows; bz++)
		for (uint32_t by = 0; by < a.ch; by++)
			for (uint32_t bx = 0; bx < tiles; bx++) {
				LwPkTile t;
				if (!lw_pk_tile(a, bx, by, bz, t))
					continue;
				if (mask && by == 0)
					for (uint32_t tid = 0; tid < LW_PK_THREADS; tid++)
						lw_pk_mask(a, t, mask, tid);
				if (!a.vec)
					block<1>(a, t, (const uint32_t *)src, dst, img);
				else if (a.dtype == LW_PK_F32)
					block<4>(a, t, (const uint32_t *)src, dst, img);
				else
					block<8>(a, t, (const uint32_t *)src, dst, img);
			}
	free(img);
	return hipSuccess;
}

static lw_pack_params params(char **v) // F LEFT RIGHT STRIDE EDGE DTYPE
{
	lw_pack_params p{};
	p.F = (uint32_t)strtoul(v[0], nullptr, 10), p.left = (uint32_t)strtoul(v[1], nullptr, 10), p.right = (uint32_t)strtoul(v[2], nullptr, 10);
	p.stride = (uint32_t)strtoul(v[3], nullptr, 10), p.edge = atoi(v[4]), p.dtype = atoi(v[5]);
	return p;
}

int main(int argc, char **argv)
{
	if (argc < 2)
		return 2;
	const std::string mode = argv[1];
	int err = 0;
	if (mode == "create" && argc >= 9) {
		lw_pack_params p = params(argv + 2);
		p.pad = std::string(argv[8]) == "nan" ? NAN : (float)atof(argv[8]);
		lw_pack *pk = lw_pack_create(argc >= 10 ? atoi(argv[9]) : 0, &p, nullptr, nullptr, &err);
		printf("RC %d\n", err);
		if ((pk == nullptr) != (err != 0))
			return 3;
		if (pk && lw_pack_width(pk) != (p.left + p.right + 1) * p.F)
			return 3;
		lw_pack_destroy(pk);
		return 0;
	}
	if (mode == "frames" && argc >= 6) {
		lw_pack_params p{};
		p.F = 3, p.left = (uint32_t)atoi(argv[2]), p.right = (uint32_t)atoi(argv[3]), p.stride = (uint32_t)atoi(argv[4]), p.edge = atoi(argv[5]);
		lw_pack *pk = lw_pack_create(0, &p, nullptr, nullptr, &err);
		if (!pk)
			return 2;
		printf("T_OUT");
		for (uint64_t T = 0; T <= 200; T++)
			printf(" %llu", (unsigned long long)lw_pack_frames(pk, T));
		printf("\n");
		if (lw_pack_frames(nullptr, 5) != 0 || lw_pack_width(nullptr) != 0 || lw_pack_tile_frames(nullptr) != 0 || lw_pack_last_launches(nullptr) != -1)
			return 3;
		lw_pack_destroy(pk);
		return 0;
	}
	if (mode == "plan" && argc >= 6) {
		const uint32_t F = (uint32_t)atoi(argv[2]), W = (uint32_t)atoi(argv[3]) + (uint32_t)atoi(argv[4]) + 1u;
		const LwPackPlan p = lw_pack_plan(F, W, (uint32_t)atoi(argv[5]));
		printf("TILE %u PITCH %u LINES %u LDS %u\n", p.tile, p.pitch, p.lines, p.lds);
		return 0;
	}
	if (mode == "convert" && argc >= 5) {
		lw_pack_params p{};
		p.F = 1, p.stride = 1, p.dtype = atoi(argv[2]);
		lw_pack *pk = lw_pack_create(0, &p, nullptr, nullptr, &err);
		if (!pk)
			return 2;
		const std::vector<float> x = slurp_f32(argv[3]);
		const size_t n = x.size();
		std::vector<uint32_t> y(n);
		for (size_t i = 0; i < n; i++)
			y[i] = lw_pack_convert(pk, x[i]);
		File(argv[4], "wb").put(y.data(), n);
		lw_pack_destroy(pk);
		return 0;
	}
	if (mode == "run" && argc >= 20) {
		lw_pack_params p = params(argv + 2);
		const uint32_t ch = (uint32_t)atoi(argv[8]), D = (p.left + p.right + 1) * p.F, es = p.dtype == LW_PACK_F32 ? 4u : 2u;
		const size_t rows = (size_t)atoll(argv[9]), cap = (size_t)atoll(argv[10]), ocap = (size_t)atoll(argv[11]);
		const bool fill = atoi(argv[12]) != 0, sh = atoi(argv[13]) != 0, sc = atoi(argv[14]) != 0, mk = atoi(argv[15]) != 0;
		const size_t ns = rows * ch * p.F * cap * 4, nd = rows * ch * ocap * D * es, nm = rows * ocap;
		std::vector<uint64_t> cnt(rows + 1), fill_to(rows + 1);
		std::vector<float> shift(D), scale(D);
		const Guarded gs = shifted(ns, (unsigned)atoi(argv[16])), gd = shifted(nd, (unsigned)atoi(argv[17])), gm = shifted(nm, 3);
		{
			File in(argv[18], "rb");
			in.get(cnt.data(), rows), in.get(fill_to.data(), rows), in.get(shift.data(), D), in.get(scale.data(), D), in.get(&p.pad, 1);
			in.get(gs.at, ns);
		}
		lw_pack *pk = lw_pack_create(0, &p, sh ? shift.data() : nullptr, sc ? scale.data() : nullptr, &err);
		if (!pk)
			return 2;
		std::fill(shift.begin(), shift.end(), 0.0f), std::fill(scale.begin(), scale.end(), 0.0f); // copied at creation: the caller's are free
		if (es == 4)
			fill32(gd.at, nd / 4, SENT_DEAD);
		else
			fill16(gd.at, nd / 2, SENT_HALF);
		memset(gm.at, 0xa5, nm);
		const int rc = lw_pack_rows(pk, ch, gs.at, gd.at, rows, cap, ocap, cnt.data(), fill ? fill_to.data() : nullptr, mk ? (uint8_t *)gm.at : nullptr, nullptr);
		printf("RC %d\nLAUNCHES %d\nTILE %u\nVEC %u\n", rc, g_log.launches, lw_pack_tile_frames(pk), g_vec);
		if (rc == LW_OK && lw_pack_last_launches(pk) != g_log.launches)
			return 3;
		{
			File out(argv[19], "wb");
			out.put(gd.at, nd), out.put(gm.at, nm);
		}
		if (!guard_intact(gs) || !guard_intact(gd) || !guard_intact(gm))
			bad("a store in front of a buffer");
		free(gs.base), free(gd.base), free(gm.base);
		lw_pack_destroy(pk);
		return 0;
	}
	// ---- calls on a small fixture: 3 rows of 2 channels, 5 lines, LFR 7/6 into bf16, capacities 300 and 60
	lw_pack_params p{};
	p.F = 5, p.left = 3, p.right = 3, p.stride = 6, p.edge = LW_PACK_EDGE_REPLICATE, p.dtype = LW_PACK_BF16;
	lw_pack *pk = lw_pack_create(0, &p, nullptr, nullptr, &err);
	if (!pk)
		return 2;
	const size_t cap = 300, ocap = 60;
	std::vector<float> src(3 * 2 * 5 * cap, 0.25f);
	std::vector<uint16_t> dst(3 * 2 * ocap * 35, 0);
	std::vector<uint8_t> msk(3 * ocap, 0);
	uint64_t cnt[3] = {300, 0, 4}, fill[3] = {60, 3, 0};
	g_log.run = false;
	if (mode == "two") {
		uint64_t cnt_b[3] = {1, 257, 13};
		int rc = lw_pack_rows(pk, 2, src.data(), dst.data(), 3, cap, ocap, cnt, fill, msk.data(), nullptr);
		printf("RC %d LAST %d\n", rc, lw_pack_last_launches(pk));
		cnt[0] = 1, fill[1] = 7; // the first call has copied its arrays: the caller's are free
		rc = lw_pack_rows(pk, 2, src.data(), dst.data(), 3, cap, ocap, cnt_b, nullptr, nullptr, nullptr);
		printf("RC %d LAST %d\n", rc, lw_pack_last_launches(pk));
		g_log.print([](const LwPackRow &r) { printf(" %llu/%llu/%llu", (unsigned long long)r.n, (unsigned long long)r.n_out, (unsigned long long)r.fill_end); });
	} else if (mode == "refuse" && argc >= 3) {
		const std::string cs = argv[2];
		uint32_t ch = 2;
		const void *s = src.data();
		void *d = dst.data();
		const uint64_t *n = cnt, *fl = fill;
		size_t rows = 3, c = cap, oc = ocap;
		lw_pack *h = pk, *other = nullptr;
		if (cs == "null_pk")
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
		else if (cs == "out_over")
			oc = 49; // row 0 has ceil(300 / 6) = 50 output frames
		else if (cs == "fill_over")
			fill[2] = ocap + 1;
		else if (cs == "ch0")
			ch = 0;
		else if (cs == "ch256")
			ch = 256;
		else if (cs == "src_too_large")
			c = (size_t)1 << 62, fl = nullptr;
		else if (cs == "dst_too_large")
			oc = (size_t)1 << 58; // 3 * 2 * 2^58 * 35 elements
		else if (cs == "too_many_tiles") // the tile of stride 6 is 32 frames: 2^24 tiles to fill, one more than a grid counts
			oc = (size_t)1 << 30, ch = 1, rows = 1, cnt[0] = 0, fill[0] = (uint64_t)32 << 24;
		else if (cs == "ok_most_tiles")
			oc = (size_t)1 << 30, ch = 1, rows = 1, cnt[0] = 0, fill[0] = ((uint64_t)32 << 24) - 32; // 2^24 - 1 tiles: accepted
		else if (cs == "ok_nothing")
			cnt[0] = cnt[2] = 0, fl = nullptr, s = nullptr, d = nullptr; // all rows empty, no fill: accepted, nothing queued
		else if (cs == "ok_no_rows")
			rows = 0, n = nullptr;
		else if (cs == "ok_fill_only")
			cnt[0] = cnt[2] = 0, s = nullptr;
		else if (cs == "ok_valid_too_short") { // VALID with every row shorter than the window reads nothing: no source needed
			p.edge = LW_PACK_EDGE_VALID;
			h = other = lw_pack_create(0, &p, nullptr, nullptr, &err);
			if (!h)
				return 2;
			cnt[0] = 6, s = nullptr, fl = nullptr, d = nullptr;
		} else if (cs != "ok")
			return 2;
		const int rc = lw_pack_rows(h, ch, s, d, rows, c, oc, n, fl, msk.data(), nullptr);
		printf("RC %d\nLAUNCHES %d\nLAST %d\n", rc, g_log.launches, lw_pack_last_launches(other ? other : pk));
		lw_pack_destroy(other);
	} else {
		return 2;
	}
	lw_pack_destroy(pk);
	return 0;
}
