// Inverse spectral frames of rows WITHOUT a GPU: lw_istft.cpp linked against hip_standins.inc (device memory = calloc), and the
// KERNEL source itself, lw_kernels_istft.hip, compiled for the host (LW_ISTFT_HOST: the route with per-lane fmaf chains): the
// stand-in for lw_launch_istft below runs it workgroup by workgroup and lane by lane, phase by phase in the kernel's own order
// (every lane of a phase before the next phase: the barriers), each lane's registers kept in an LwIsLane between the phases,
// with an LDS buffer of exactly the kernel's size, so AddressSanitizer sees every load and store the kernel makes.
// tests/test_host_istft.py drives it.
//   istft_host basis NFFT WIN HOP WINDOW CENTER FILE FILE2   "G bins offset ov m", the table [2 B][WIN] as raw f32 into FILE and
//                                                            w2 [WIN] as raw f64 into FILE2
//   istft_host create NFFT WIN HOP WINDOW CENTER RESERVED    "RC err"
//   istft_host lens NFFT WIN HOP WINDOW CENTER T...          "L T natural" per T
//   istft_host tile NFFT WIN HOP CENTER M TILE T OUTLEN DROW CAP   "S s0 tf0 nf r0 P d_at": lw_is_tile's 64-bit arithmetic far up a row
//   istft_host refuse CASE                                   "RC rc", "LAUNCHES n", "WRITTEN n" (elements that lost the sentinel)
//   istft_host run NFFT WIN HOP WINDOW CENTER M FMT CH ROWS FCAP NDST DCAP IN OUT FRAMES ROWMAP LENS
//        the rows in IN (raw f32 [ROWS][CH][2 B][FCAP], an exact-size buffer) into a sentinel-filled exact-size destination, dumped
//        to OUT; FRAMES / ROWMAP / LENS are comma lists, "-" for NULL; M 0 keeps the object's m: "RC rc", "M m", "LAUNCHES n"
#include "../../include/lewton_amd.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "hip_standins.inc"
#include "kernel_host.hpp"

#define LW_ISTFT_HOST 1
#include "../../lewton_amd/csrc/lw_kernels_istft.hip"

static LaunchLog<LwIstftRow> g_log;

static void run_tile(const LwIstftArgs &a, uint32_t bx, uint32_t by, uint32_t bz)
{
	LwIsTile t;
	if (!lw_is_tile(a, bx, by, bz, t))
		return;
	float *lds = (float *)malloc((size_t)LW_IS_LDS_FLOATS * 4); // exactly the kernel's size: one float beyond it is an ASan report
	for (size_t i = 0; i < LW_IS_LDS_FLOATS; i++)
		lds[i] = NAN; // LDS holds garbage at launch
	std::vector<LwIsLane> st(LW_IS_THREADS);
	const uint32_t N = LW_IS_THREADS;
	for (uint32_t tid = 0; tid < N; tid++)
		lw_is_zero_span(t, tid, lds);
	if (t.nf)
		for (uint32_t pass = a.passes; pass-- > 0u;) {
			for (uint32_t tid = 0; tid < N; tid++)
				lw_is_zero_acc(st[tid]);
			for (uint32_t kt = 0; kt < a.l_pad / LW_IS_KT; kt++) {
				for (uint32_t tid = 0; tid < N; tid++)
					lw_is_stage(a, t, pass, kt, tid, lds);
				for (uint32_t tid = 0; tid < N; tid++)
					lw_is_mma<LW_IS_ROUTE_FMA>(a, pass, tid, lds, st[tid]);
			}
			for (uint32_t tid = 0; tid < N; tid++)
				lw_is_put_y(a, pass, tid, lds, st[tid]);
			for (uint32_t tid = 0; tid < N; tid++)
				lw_is_add(a, t, pass, tid, lds);
		}
	for (uint32_t tid = 0; tid < N; tid++)
		lw_is_finish(a, t, tid, lds);
	free(lds);
}

hipError_t lw_launch_istft(const LwIstftArgs &a, int route, uint32_t tiles, uint32_t ch, uint32_t n_rows, hipStream_t)
{
	g_log.launch();
	if (!a.rows || !a.table || !a.w2 || (route != 0 && route != 1) || ch == 0 || n_rows > 65535u || a.l_pad % LW_IS_KT || tiles > LW_IS_MAX_TILES ||
			a.m == 0 || (uint64_t)a.m * a.hop > LW_IS_SPAN_MAX || a.m + (a.win_length + a.hop - 1u) / a.hop > LW_IS_TF)
		bad("arguments");
	if (!g_log.run)
		return hipSuccess;
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

static lw_istft *make(char **v, int *err, uint32_t reserved = 0)
{
	lw_istft_params p{u32(v[0]), u32(v[1]), u32(v[2]), atoi(v[3]), atoi(v[4]), reserved};
	return lw_istft_create(0, &p, err);
}

static bool list(const char *s, std::vector<uint64_t> &out)
{
	out.clear();
	if (!strcmp(s, "-"))
		return false;
	for (const char *p = s; *p;) {
		char *end;
		out.push_back(strtoull(p, &end, 10));
		p = *end ? end + 1 : end;
	}
	return true;
}

static const uint32_t SENT = SENT_ABC;

int main(int argc, char **argv)
{
	if (argc < 2)
		return 2;
	const std::string mode = argv[1];
	int err = 0;
	if (mode == "create" && argc >= 8) {
		lw_istft *is = make(argv + 2, &err, u32(argv[7]));
		printf("RC %d\n", err);
		if ((is == nullptr) != (err != 0))
			return 3;
		lw_istft_destroy(is);
		return 0;
	}
	if (mode == "basis" && argc >= 9) {
		lw_istft *is = make(argv + 2, &err);
		if (!is)
			return 2;
		const LwIstftPlan p = lw_istft_plan(u32(argv[2]), u32(argv[3]), u32(argv[4]));
		printf("G %u %u %u %u\n", lw_istft_bins(is), p.offset, p.ov, lw_istft_tile_frames(is));
		std::vector<float> g(lw_istft_basis(is, nullptr));
		std::vector<double> w2(lw_istft_window2(is, nullptr));
		if (g.size() != (size_t)p.lines * u32(argv[3]) || w2.size() != u32(argv[3]) || lw_istft_basis(is, g.data()) != g.size() ||
				lw_istft_window2(is, w2.data()) != w2.size())
			return 3;
		File(argv[7], "wb").put(g.data(), g.size());
		File(argv[8], "wb").put(w2.data(), w2.size());
		lw_istft_destroy(is);
		return 0;
	}
	if (mode == "lens" && argc >= 7) {
		lw_istft *is = make(argv + 2, &err);
		if (!is)
			return 2;
		for (int i = 7; i < argc; i++) {
			const uint64_t T = strtoull(argv[i], nullptr, 10);
			printf("L %llu %llu\n", (unsigned long long)T, (unsigned long long)lw_istft_out_len(is, T));
		}
		lw_istft_destroy(is);
		return 0;
	}
	if (mode == "tile" && argc >= 12) {
		const uint32_t n_fft = u32(argv[2]), win = u32(argv[3]), hop = u32(argv[4]), center = u32(argv[5]), m = u32(argv[6]);
		const uint64_t tile = strtoull(argv[7], nullptr, 10);
		LwIstftRow row{strtoull(argv[8], nullptr, 10), strtoull(argv[9], nullptr, 10), strtoull(argv[10], nullptr, 10)};
		const uint64_t cap = strtoull(argv[11], nullptr, 10);
		LwIstftArgs a{};
		a.rows = &row, a.n_fft = n_fft, a.win_length = win, a.hop = hop, a.offset = (n_fft - win) / 2, a.m = m, a.pad = center ? n_fft / 2 : 0;
		a.d = LwIstftLayout{cap * 2, cap, 1};
		a.tile0 = (uint32_t)(tile - tile % 1000u); // (the launch's first tile and the workgroup's index within it)
		LwIsTile t;
		if (!lw_is_tile(a, (uint32_t)(tile % 1000u), 1, 0, t))
			return 3;
		printf("S %llu %llu %u %d %llu %llu\n", (unsigned long long)t.s0, (unsigned long long)t.tf0, t.nf, t.r0, (unsigned long long)t.P,
				(unsigned long long)t.d_at);
		return 0;
	}
	if (mode == "run" && argc >= 19) {
		lw_istft *is = make(argv + 2, &err);
		if (!is)
			return 2;
		const uint32_t m = u32(argv[7]), ch = u32(argv[9]);
		const int fmt = atoi(argv[8]);
		const size_t rows = strtoull(argv[10], nullptr, 10), fcap = strtoull(argv[11], nullptr, 10), ndst = strtoull(argv[12], nullptr, 10),
			     dcap = strtoull(argv[13], nullptr, 10);
		if (m && lw_istft_set_tile_frames(is, m) != LW_OK)
			return 3;
		if (lw_istft_set_route(is, LW_IS_ROUTE_FMA) != LW_OK) // the route this program has
			return 3;
		const size_t sn = rows * ch * 2 * lw_istft_bins(is) * fcap, dn = ndst * ch * dcap;
		float *src = (float *)malloc(sn ? sn * 4 : 4), *dst = (float *)malloc(dn ? dn * 4 : 4); // exact sizes: one element beyond is an ASan report
		File(argv[14], "rb").get(src, sn);
		fill32(dst, dn, SENT);
		std::vector<uint64_t> frames, map64, lens;
		list(argv[16], frames);
		const bool has_map = list(argv[17], map64), has_len = list(argv[18], lens);
		std::vector<uint32_t> map(map64.begin(), map64.end());
		if (frames.size() != rows || (has_map && map.size() != rows) || (has_len && lens.size() != rows))
			return 2;
		const int rc = lw_istft_rows(is, ch, src, rows, fcap, frames.data(), has_map ? map.data() : nullptr, has_len ? lens.data() : nullptr, fmt, dst, ndst,
				dcap, nullptr);
		printf("RC %d\nM %u\nLAUNCHES %d\n", rc, lw_istft_tile_frames(is), g_log.launches);
		if (rc == LW_OK && g_log.launches && lw_istft_last_route(is) != 1)
			return 3;
		File(argv[15], "wb").put(dst, dn);
		free(src), free(dst);
		lw_istft_destroy(is);
		return 0;
	}
	if (mode != "refuse" || argc < 3)
		return 2;
	// ---- refusals on a small fixture: 3 rows of 2 channels, (16, 16, 4) hann centred; T = 9 gives 32 samples
	lw_istft_params prm{16, 16, 4, LW_SPEC_HANN, 1, 0};
	lw_istft *is = lw_istft_create(0, &prm, &err);
	if (!is)
		return 2;
	const size_t fcap = 9, dcap = 40;
	std::vector<float> src(3 * 2 * 18 * fcap, 0.25f), dst(4 * 2 * dcap);
	fill32(dst.data(), dst.size(), SENT);
	uint64_t frames[3] = {9, 0, 5}, lens[3] = {32, 7, 40};
	uint32_t map[3] = {2, 0, 3};
	const std::string cs = argv[2];
	int fmt = LW_FMT_F32_PLANAR;
	uint32_t ch = 2;
	const void *s = src.data();
	void *d = dst.data();
	const uint64_t *fr = frames, *ln = lens;
	const uint32_t *mp = map;
	size_t n_dst = 4, fc = fcap, dc = dcap;
	lw_istft *h = is;
	int rc;
	if (cs == "null_is")
		h = nullptr;
	else if (cs == "null_frames")
		fr = nullptr;
	else if (cs == "null_src")
		s = nullptr;
	else if (cs == "null_dst")
		d = nullptr;
	else if (cs == "i16")
		fmt = LW_FMT_I16_PLANAR;
	else if (cs == "i16_interleaved")
		fmt = LW_FMT_I16_INTERLEAVED;
	else if (cs == "bad_fmt")
		fmt = 17;
	else if (cs == "ch0")
		ch = 0;
	else if (cs == "ch256")
		ch = 256;
	else if (cs == "frames_over")
		frames[2] = fcap + 1; // (the LAST row: every row is checked before anything is queued)
	else if (cs == "len_over")
		lens[2] = dcap + 1;
	else if (cs == "natural_over")
		ln = nullptr, dc = 31; // the natural length of 9 frames is 32
	else if (cs == "row_over")
		map[2] = 4;
	else if (cs == "row_over_identity")
		mp = nullptr, n_dst = 2;
	else if (cs == "row_twice")
		map[2] = 2;
	else if (cs == "row_twice_empty")
		map[1] = 3;
	else if (cs == "bytes_over")
		fc = (size_t)1 << 62, frames[0] = frames[2] = 0;
	else if (cs == "bad_route" || cs == "bad_m" || cs == "bad_m0") {
		rc = cs == "bad_route" ? lw_istft_set_route(is, 2) : lw_istft_set_tile_frames(is, cs == "bad_m" ? lw_istft_tile_frames(is) + 1 : 0);
		printf("RC %d\nLAUNCHES %d\nWRITTEN 0\n", rc, g_log.launches);
		lw_istft_destroy(is);
		return 0;
	} else if (cs != "ok" && cs != "ok_natural")
		return 2;
	if (cs == "ok_natural")
		ln = nullptr;
	rc = lw_istft_rows(h, ch, s, 3, fc, fr, mp, ln, fmt, d, n_dst, dc, nullptr);
	size_t written = 0;
	for (auto &v : dst)
		written += memcmp(&v, &SENT, 4) != 0;
	printf("RC %d\nLAUNCHES %d\nWRITTEN %zu\n", rc, g_log.launches, written);
	lw_istft_destroy(is);
	return 0;
}
