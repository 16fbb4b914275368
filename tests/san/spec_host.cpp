// Spectral frames of rows WITHOUT a GPU: lw_spec.cpp linked against hip_standins.inc (device memory = calloc), and the KERNEL
// source itself, lw_kernels_spec.hip, compiled for the host (LW_SPEC_HOST: the route with per-lane fmaf chains): the stand-in for
// lw_launch_spec below runs it workgroup by workgroup and lane by lane, phase by phase in the kernel's own order (every lane of
// a phase before the next phase: the barriers), each lane's registers kept in an LwSpLane between the phases, with an LDS buffer
// of exactly the kernel's size, so AddressSanitizer sees every load and store the kernel makes.  tests/test_host_spec.py drives it.
//   spec_host basis NFFT WIN HOP WINDOW CENTER FILE      "G bins features offset" and the basis [2][WIN][B] as raw f32 into FILE
//   spec_host frames NFFT WIN HOP WINDOW CENTER LEN...   "L len n_frames" per LEN
//   spec_host index NFFT WIN HOP WINDOW CENTER FRAME...  "I frame index": the input index of sample 0 of FRAME by the kernel's own
//                                                        index functions (lw_sp_tile / lw_sp_index)
//   spec_host create NFFT WIN HOP WINDOW CENTER NMELS FB "RC err" (FB 0: a NULL matrix)
//   spec_host refuse CASE            "RC rc" and "LAUNCHES n": CASE is one of the refusals of lw_spec_rows (main below)
//   spec_host two                    two calls queued back to back: "ROWS len/frames/row..." per launch, read at the end
//   spec_host run NFFT WIN HOP WINDOW CENTER IN OUT      the power spectrum of one row (raw f32 IN) as [B][frames] raw f32 into OUT
//   spec_host kernel SEED CASES      the listed shapes and random ones against a scalar chain, bit for bit: "CASE ..." per case
#include "../../include/lewton_amd.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "hip_standins.inc"
#include "kernel_host.hpp"

#define LW_SPEC_HOST 1
#include "../../lewton_amd/csrc/lw_kernels_spec.hip"

static LaunchLog<LwSpecRow> g_log;
static std::vector<std::pair<uint32_t, uint32_t>> g_tiles; // (tile0, tiles) of each launch

static void run_tile(const LwSpecArgs &a, uint32_t bx, uint32_t by, uint32_t bz)
{
	LwSpTile t;
	if (!lw_sp_tile(a, bx, by, bz, t))
		return;
	float *lds = (float *)malloc((size_t)LW_SP_LDS_FLOATS * 4); // exactly the kernel's size: one float beyond it is an ASan report
	for (size_t i = 0; i < LW_SP_LDS_FLOATS; i++)
		lds[i] = NAN; // LDS holds garbage at launch
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
		if (a.n_mels == 0) {
			for (uint32_t tid = 0; tid < T; tid++)
				lw_sp_store_power(a, t, pass, tid, lds);
			continue;
		}
		for (uint32_t jc = 0; jc < lw_sp_slices(a, pass); jc++) {
			for (uint32_t tid = 0; tid < T; tid++)
				lw_sp_stage_fb(a, pass, jc, tid, lds);
			for (uint32_t tid = 0; tid < T; tid++)
				lw_sp_mel(a, pass, jc, tid, lds, st[tid]);
		}
	}
	if (a.n_mels)
		for (uint32_t tid = 0; tid < T; tid++)
			lw_sp_store_mel(a, t, tid, st[tid]);
	free(lds);
}

hipError_t lw_launch_spec(const LwSpecArgs &a, int route, uint32_t tiles, uint32_t ch, uint32_t n_rows, hipStream_t)
{
	g_log.launch(a.rows + a.row0, n_rows);
	g_tiles.emplace_back(a.tile0, tiles);
	if (!a.rows || !a.basis || (a.n_mels && !a.fb) || (route != 0 && route != 1) || ch == 0 || n_rows > 65535u || a.k_pad % LW_SP_KT || a.mel_pad % 32u ||
			tiles > LW_SP_MAX_TILES)
		bad("arguments");
	if (!g_log.run)
		return hipSuccess;
	for (uint32_t bz = 0; bz < n_rows; bz++)
		for (uint32_t by = 0; by < ch; by++)
			for (uint32_t bx = 0; bx < tiles; bx++)
				run_tile(a, bx, by, bz);
	return hipSuccess;
}

static lw_spec *make(char **v, uint32_t n_mels, const float *fb, int *err)
{
	return lw_spec_create(0, (uint32_t)strtoul(v[0], nullptr, 10), (uint32_t)strtoul(v[1], nullptr, 10), (uint32_t)strtoul(v[2], nullptr, 10), atoi(v[3]),
			atoi(v[4]), n_mels, fb, err);
}

static uint32_t bits(float f) // -0 counts as +0: the sign of a zero is outside the contract
{
	uint32_t u;
	memcpy(&u, &f, 4);
	return u == 0x80000000u ? 0u : u;
}

struct Shape {
	uint32_t n_fft, win, hop;
	int window, center;
	uint32_t n_mels;
};

// the contract, scalar: line q (or bin q without a mel matrix) of frame t of a row of len samples x (stride el)
static void frame_features(const Shape &s, const std::vector<float> &basis, const std::vector<float> &fb, const float *x, uint64_t el, uint64_t len,
		uint64_t t, std::vector<float> &P, std::vector<float> &out)
{
	const uint32_t B = s.n_fft / 2 + 1, o = (s.n_fft - s.win) / 2;
	const int64_t first = (int64_t)(t * s.hop) - (s.center ? (int64_t)(s.n_fft / 2) : 0) + o;
	const float *Cb = basis.data(), *Sb = basis.data() + (size_t)s.win * B;
	P.assign(B, 0.0f);
	for (uint32_t j = 0; j < B; j++) {
		float re = 0.0f, im = 0.0f;
		for (uint32_t k = 0; k < s.win; k++) {
			const int64_t i = first + k;
			const float xv = i >= 0 && (uint64_t)i < len ? x[(uint64_t)i * el] : 0.0f;
			re = fmaf(xv, Cb[(size_t)k * B + j], re);
			im = fmaf(xv, Sb[(size_t)k * B + j], im);
		}
		const float sq = re * re;
		P[j] = fmaf(im, im, sq);
	}
	if (s.n_mels == 0) {
		out = P;
		return;
	}
	out.assign(s.n_mels, 0.0f);
	for (uint32_t q = 0; q < s.n_mels; q++) {
		float acc = 0.0f;
		for (uint32_t j = 0; j < B; j++)
			acc = fmaf(P[j], fb[(size_t)q * B + j], acc);
		out[q] = acc;
	}
}

static const uint32_t SENT = SENT_ABC;

// the shapes every suite lists, then random ones
static const Shape LISTED[] = {{400, 400, 160, 0, 1, 80}, {512, 400, 160, 0, 1, 80}, {16, 16, 4, 1, 0, 0}, {25, 25, 7, 0, 1, 0}, {64, 64, 100, 0, 1, 1},
	{32, 32, 1, 0, 1, 0}, {2048, 2048, 512, 0, 1, 128}, {400, 400, 160, 0, 1, 0}, {400, 400, 160, 0, 0, 1}, {400, 400, 160, 1, 1, 128}};
static const uint64_t LENS_400[] = {0, 1, 159, 160, 199, 200, 399, 400, 401, 1999}, LENS_16[] = {15, 16, 17, 19, 20};

static int kernel_cases(unsigned seed, int cases)
{
	std::mt19937 rng(seed);
	auto rnd = [&](uint32_t lo, uint32_t hi) { return lo + (uint32_t)(rng() % (hi - lo + 1)); };
	const int n_listed = (int)(sizeof(LISTED) / sizeof(LISTED[0]));
	int done = 0;
	for (int c = 0; c < cases; c++) {
		Shape s;
		if (c < n_listed) {
			s = LISTED[c];
		} else {
			s.n_fft = rnd(0, 3) == 0 ? rnd(2, 40) : rnd(2, 640);
			s.win = rnd(0, 1) ? s.n_fft : rnd(1, s.n_fft);
			s.hop = rnd(0, 3) == 0 ? rnd(1, 8) : rnd(1, 300);
			s.window = (int)rnd(0, 1), s.center = (int)rnd(0, 1);
			const uint32_t kind = rnd(0, 4);
			s.n_mels = kind == 0 ? 0 : kind == 1 ? 1 : kind == 2 ? 80 : kind == 3 ? 128 : rnd(1, 256);
		}
		const uint32_t B = s.n_fft / 2 + 1, F = s.n_mels ? s.n_mels : B;
		std::uniform_real_distribution<float> uni(-1.0f, 1.0f);
		std::vector<float> fb((size_t)s.n_mels * B);
		for (auto &v : fb)
			v = rnd(0, 2) == 0 ? 0.0f : std::fabs(uni(rng)) * 0.05f;
		int err = 0;
		lw_spec *sp = lw_spec_create(0, s.n_fft, s.win, s.hop, s.window, s.center, s.n_mels, s.n_mels ? fb.data() : nullptr, &err);
		if (!sp)
			bad("create %d", err);
		if (lw_spec_set_route(sp, LW_SP_ROUTE_FMA) != LW_OK) // the route this program has
			return 3;
		std::vector<float> basis(lw_spec_basis(sp, nullptr));
		if (basis.size() != (size_t)2 * s.win * B || lw_spec_basis(sp, basis.data()) != basis.size() || lw_spec_bins(sp) != B || lw_spec_features(sp) != F)
			return 3;
		const int fmt = (c & 1) ? LW_FMT_F32_INTERLEAVED : LW_FMT_F32_PLANAR;
		const bool itl = fmt == LW_FMT_F32_INTERLEAVED;
		const uint32_t TF = lw_spec_tile_frames(sp);
		std::vector<uint64_t> len;
		uint32_t ch = rnd(1, 3);
		if (c == 0 || c == 7) {
			len.assign(LENS_400, LENS_400 + 10), ch = 2;
		} else if (c == 2) {
			len.assign(LENS_16, LENS_16 + 5);
		} else if (c == 6) {
			len = {700}, ch = 1; // one short row
		} else if (c == 8) {
			len = {(uint64_t)s.n_fft + (TF - 1) * s.hop, (uint64_t)s.n_fft + TF * s.hop}; // exactly a tile of frames, and one more
		} else {
			const uint32_t rows = rnd(1, 3);
			for (uint32_t r = 0; r < rows; r++) {
				const uint32_t kind = rnd(0, 5);
				len.push_back(kind == 0 ? 0 : kind == 1 ? rnd(1, s.n_fft + 1) : kind == 2 ? (uint64_t)s.hop * rnd(TF - 2, TF + 1) + rnd(0, 1) * s.n_fft
						: rnd(0, std::min<uint32_t>(3000, 40 * s.hop + s.n_fft)));
			}
		}
		const uint32_t rows = (uint32_t)len.size(), extra = rnd(0, 2);
		uint64_t longest = 0, most = 0;
		for (auto l : len) {
			longest = std::max(longest, l);
			most = std::max(most, lw_spec_frames(sp, l));
		}
		const size_t scap = (longest + rnd(0, 9)) | 1, fcap = (most + rnd(0, 5)) | 1; // odd capacities
		std::vector<uint32_t> map(rows);
		for (uint32_t r = 0; r < rows; r++)
			map[r] = rows + extra - 1 - r; // reversed, the gap in front
		// exact-size buffers: one element beyond either is an ASan report
		const size_t sn = (size_t)rows * ch * scap, dn = (size_t)(rows + extra) * ch * F * fcap;
		float *src = (float *)malloc(sn * 4), *dst = (float *)malloc(dn * 4), *want = (float *)malloc(dn * 4);
		fill32(src, sn, SENT), fill32(dst, dn, SENT), fill32(want, dn, SENT);
		std::vector<float> P, out;
		for (uint32_t r = 0; r < rows; r++)
			for (uint32_t q = 0; q < ch; q++) {
				float *x = src + (itl ? ((size_t)r * scap) * ch + q : ((size_t)r * ch + q) * scap);
				const uint64_t el = itl ? ch : 1;
				const uint32_t kind = rnd(0, 3);
				for (uint64_t i = 0; i < len[r]; i++) {
					float v = kind == 0 ? (i == len[r] / 2 ? 1.0f : 0.0f) : kind == 1 ? uni(rng) * 1e-20f : uni(rng);
					if (kind == 2 && (i & 7) == 0)
						v = -0.0f;
					x[i * el] = v;
				}
				float *y = want + ((size_t)map[r] * ch + q) * F * fcap;
				const uint64_t frames = lw_spec_frames(sp, len[r]);
				for (uint64_t t = 0; t < frames; t++) {
					frame_features(s, basis, fb, x, el, len[r], t, P, out);
					for (uint32_t l = 0; l < F; l++)
						y[(size_t)l * fcap + t] = out[l];
				}
			}
		const int rc = lw_spec_rows(sp, fmt, ch, src, rows, scap, len.data(), map.data(), dst, rows + extra, fcap, nullptr);
		printf("CASE %d fft%u win%u hop%u w%d c%d mels%u fmt%d ch%u rows%u frames%llu route %d rc %d\n", c, s.n_fft, s.win, s.hop, s.window, s.center,
				s.n_mels, fmt, ch, rows, (unsigned long long)most, lw_spec_last_route(sp), rc);
		if (rc != LW_OK)
			return 3;
		for (size_t i = 0; i < dn; i++)
			if (bits(dst[i]) != bits(want[i]))
				bad("element %zu: %08x, expected %08x", i, bits(dst[i]), bits(want[i]));
		free(src), free(dst), free(want);
		lw_spec_destroy(sp);
		done++;
	}
	printf("OK %d\n", done);
	return 0;
}

int main(int argc, char **argv)
{
	if (argc < 2)
		return 2;
	const std::string mode = argv[1];
	int err = 0;
	if (mode == "create" && argc >= 9) {
		const uint32_t n_mels = (uint32_t)strtoul(argv[7], nullptr, 10);
		std::vector<float> fb((size_t)n_mels * 2048 + 1, 0.5f);
		lw_spec *sp = make(argv + 2, n_mels, atoi(argv[8]) ? fb.data() : nullptr, &err);
		printf("RC %d\n", err);
		if ((sp == nullptr) != (err != 0))
			return 3;
		lw_spec_destroy(sp);
		return 0;
	}
	if ((mode == "basis" && argc >= 8) || (mode == "frames" && argc >= 7) || (mode == "index" && argc >= 7) || (mode == "run" && argc >= 9)) {
		lw_spec *sp = make(argv + 2, 0, nullptr, &err);
		if (!sp)
			return 2;
		const uint32_t n_fft = (uint32_t)strtoul(argv[2], nullptr, 10), win = (uint32_t)strtoul(argv[3], nullptr, 10), hop = (uint32_t)strtoul(argv[4], nullptr, 10);
		const bool center = atoi(argv[6]) != 0;
		const LwSpecPlan p = lw_spec_plan(n_fft, win, 0);
		if (mode == "basis") {
			printf("G %u %u %u\n", lw_spec_bins(sp), lw_spec_features(sp), p.offset);
			std::vector<float> b(lw_spec_basis(sp, nullptr));
			if (b.size() != (size_t)2 * win * p.bins || lw_spec_basis(sp, b.data()) != b.size())
				return 3;
			File(argv[7], "wb").put(b.data(), b.size());
		} else if (mode == "frames") {
			for (int i = 7; i < argc; i++) {
				const uint64_t len = strtoull(argv[i], nullptr, 10);
				printf("L %llu %llu\n", (unsigned long long)len, (unsigned long long)lw_spec_frames(sp, len));
			}
		} else if (mode == "index") {
			LwSpecRow row{UINT64_MAX, UINT64_MAX, 0};
			LwSpecArgs a{};
			a.rows = &row, a.hop = hop, a.s = LwSpecLayout{0, 0, 1};
			a.lead = (int64_t)p.offset - (int64_t)(center ? n_fft / 2 : 0);
			for (int i = 7; i < argc; i++) {
				const uint64_t frame = strtoull(argv[i], nullptr, 10), bx = frame / LW_SP_TF;
				LwSpTile t;
				if (bx > UINT32_MAX || !lw_sp_tile(a, (uint32_t)bx, 0, 0, t))
					return 3;
				printf("I %llu %lld\n", (unsigned long long)frame, (long long)(lw_sp_index(a, t, (uint32_t)(frame % LW_SP_TF), 0) - (int64_t)p.offset));
			}
		} else {
			const std::vector<float> in = slurp_f32(argv[7]);
			const size_t n = in.size();
			float *x = (float *)malloc(n ? n * 4 : 4); // an exact-size source
			std::copy(in.begin(), in.end(), x);
			const uint64_t len = n, frames = lw_spec_frames(sp, len);
			std::vector<float> y((size_t)p.bins * frames + 1, 0.0f);
			const int rc = lw_spec_rows(sp, LW_FMT_F32_PLANAR, 1, x, 1, n, &len, nullptr, y.data(), 1, frames, nullptr);
			printf("RC %d\nF %u %llu\n", rc, p.bins, (unsigned long long)frames);
			File(argv[8], "wb").put(y.data(), (size_t)p.bins * frames);
			free(x);
		}
		lw_spec_destroy(sp);
		return 0;
	}
	if (mode == "kernel" && argc >= 4)
		return kernel_cases((unsigned)atoi(argv[2]), atoi(argv[3]));
	// ---- calls on a small fixture: 3 rows of 2 channels, (400, 400, 160) hann centred, the power spectrum
	lw_spec *sp = lw_spec_create(0, 400, 400, 160, LW_SPEC_HANN, 1, 0, nullptr, &err);
	if (!sp)
		return 2;
	const size_t scap = 1001, fcap = 7; // n_frames(1000) = 7
	std::vector<float> src(3 * 2 * scap, 0.25f), dst(4 * 2 * 201 * fcap, 0.0f);
	uint64_t len[3] = {1000, 0, 441};
	uint32_t map[3] = {2, 0, 3};
	if (mode == "two") {
		g_log.run = false;
		uint64_t len_b[3] = {7, 8, 159};
		int rc = lw_spec_rows(sp, LW_FMT_F32_PLANAR, 2, src.data(), 3, scap, len, map, dst.data(), 4, fcap, nullptr);
		printf("RC %d\n", rc);
		len[0] = 1; // the first call has copied its lengths: the caller's are free
		rc = lw_spec_rows(sp, LW_FMT_F32_INTERLEAVED, 2, src.data(), 3, scap, len_b, nullptr, dst.data(), 4, fcap, nullptr);
		printf("RC %d\n", rc);
		g_log.print([](const LwSpecRow &r) { printf(" %llu/%llu/%llu", (unsigned long long)r.len, (unsigned long long)r.n_frames, (unsigned long long)r.dst_row); });
	} else if (mode == "refuse" && argc >= 3) {
		const std::string cs = argv[2];
		int fmt = LW_FMT_F32_PLANAR;
		uint32_t ch = 2;
		const void *s = src.data();
		void *d = dst.data();
		const uint64_t *l = len;
		const uint32_t *mp = map;
		size_t n_dst = 4, sc = scap, fc = fcap;
		lw_spec *h = sp;
		g_log.run = false;
		if (cs == "null_sp")
			h = nullptr;
		else if (cs == "null_len")
			l = nullptr;
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
		else if (cs == "len_over")
			len[2] = scap + 1; // (the LAST row: every row is checked before anything is queued)
		else if (cs == "frames_over")
			fc = 6;
		else if (cs == "row_over")
			map[2] = 4;
		else if (cs == "row_over_identity")
			mp = nullptr, n_dst = 2;
		else if (cs == "row_twice")
			map[2] = 2;
		else if (cs == "row_twice_empty")
			map[1] = 3; // the row without samples names a row another one has
		else if (cs == "bad_route") {
			printf("RC %d\nLAUNCHES %d\n", lw_spec_set_route(sp, 2), g_log.launches);
			lw_spec_destroy(sp);
			return 0;
		} else if (cs == "ok_many_tiles") {
			// one row of 2^30 + 1 frames: 2^25 + 1 tiles, more than one launch holds (nothing runs here, and no sample is touched)
			len[0] = sc = (size_t)160 << 30, len[1] = len[2] = 0, fc = ((size_t)1 << 30) + 1;
		} else if (cs != "ok" && cs != "ok_exact" && cs != "ok_route1")
			return 2;
		if (cs == "ok_exact")
			sc = 1000;
		if (cs == "ok_route1" && lw_spec_set_route(sp, 1) != LW_OK)
			return 3;
		const int rc = lw_spec_rows(h, fmt, ch, s, 3, sc, l, mp, d, n_dst, fc, nullptr);
		printf("RC %d\nLAUNCHES %d\n", rc, g_log.launches);
		if (cs == "ok_many_tiles")
			for (const auto &g : g_tiles)
				printf("TILES %u %u\n", g.first, g.second);
		if (rc == LW_OK && lw_spec_last_route(sp) != (cs == "ok_route1" ? 1 : 0))
			return 3;
	} else {
		return 2;
	}
	lw_spec_destroy(sp);
	return 0;
}
