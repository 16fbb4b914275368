// The row resampler WITHOUT a GPU: lw_resample.cpp linked against hip_standins.inc (device memory = calloc), and the KERNEL source
// itself, lw_kernels_resample.hip, compiled for the host (LW_RESAMPLE_HOST): the stand-in for lw_launch_resample below runs it
// workgroup by workgroup and lane by lane (stage for every lane, then fold for every lane: the barrier), with an LDS buffer of
// exactly the planned size, so AddressSanitizer sees every load and store the kernel makes.  tests/test_host_resample.py drives it.
//   resample_host taps IN OUT ZEROS ROLLOFF WINDOW BETA FILE   "G orig new W K" and the taps [new][K] as raw f32 into FILE
//   resample_host outlen IN OUT ZEROS ROLLOFF WINDOW BETA LEN...   "L len out_len" per LEN
//   resample_host index IN OUT ZEROS ROLLOFF WINDOW BETA N...   "I n base i route": base(n) and n mod new by the kernel's own index
//                 arithmetic (lw_rs_tile / lw_rs_unit / lw_rs_global_index), for the planned route and for the global-taps one
//   resample_host create IN OUT ZEROS ROLLOFF WINDOW BETA        "RC err"
//   resample_host refuse CASE          "RC rc" and "LAUNCHES n": CASE is one of the refusals of lw_resample_rows (main below)
//   resample_host two                  two calls queued back to back: "ROWS len..." per launch, read at the end
//   resample_host kernel SEED CASES    random cases against a scalar fold, bit for bit: "CASE ..." per case, "OK n" at the end
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

#define LW_RESAMPLE_HOST 1
#include "../../lewton_amd/csrc/lw_kernels_resample.hip"

static LaunchLog<LwResampleRow> g_log;
static std::vector<std::pair<uint32_t, uint32_t>> g_tiles; // (tile0, tiles) of each launch

template <int ROUTE, int J> static void run_tile(const LwResampleArgs &a, const LwResamplePlan &p, uint32_t bx, uint32_t by, uint32_t bz)
{
	LwRsTile t;
	if (!lw_rs_tile(a, p.tile, bx, by, bz, t))
		return;
	float *lds = (float *)malloc((size_t)p.lds_floats * 4); // exactly the planned size: one float beyond it is an ASan report
	for (size_t i = 0; i < p.lds_floats; i++)
		lds[i] = NAN; // LDS holds garbage at launch
	for (uint32_t tid = 0; tid < LW_RS_THREADS; tid++)
		lw_rs_stage<ROUTE>(a, t, p.span, tid, LW_RS_THREADS, lds);
	for (uint32_t tid = 0; tid < LW_RS_THREADS; tid++)
		lw_rs_fold<ROUTE, J>(a, t, p.span, tid, LW_RS_THREADS, lds);
	free(lds);
}

hipError_t lw_launch_resample(const LwResampleArgs &a, const LwResamplePlan &p, uint32_t tiles, uint32_t ch, uint32_t n_rows, hipStream_t)
{
	g_log.launch(a.rows + a.row0, n_rows);
	g_tiles.emplace_back(a.tile0, tiles);
	if (!a.rows || !a.taps || p.lds_floats > LW_RS_LDS_FLOATS || p.blocks != a.blocks || ch == 0 || n_rows > 65535u || tiles > LW_RS_MAX_TILES)
		bad("arguments");
	if (!g_log.run)
		return hipSuccess;
	for (uint32_t bz = 0; bz < n_rows; bz++)
		for (uint32_t by = 0; by < ch; by++)
			for (uint32_t bx = 0; bx < tiles; bx++) {
				LwRsTile t;
				if (p.route == LW_RS_ROUTE_COPY) {
					if (lw_rs_tile(a, p.tile, bx, by, bz, t))
						for (uint32_t tid = 0; tid < LW_RS_THREADS; tid++)
							lw_rs_copy(a, t, tid, LW_RS_THREADS);
				} else if (p.route == LW_RS_ROUTE_GLOBAL) {
					if (lw_rs_tile(a, p.tile, bx, by, bz, t))
						for (uint32_t tid = 0; tid < LW_RS_THREADS; tid++)
							lw_rs_fold_global(a, t, tid);
				} else if (p.route == LW_RS_ROUTE_LDS) {
					p.j == 4 ? run_tile<LW_RS_ROUTE_LDS, 4>(a, p, bx, by, bz) : p.j == 2 ? run_tile<LW_RS_ROUTE_LDS, 2>(a, p, bx, by, bz)
					         : run_tile<LW_RS_ROUTE_LDS, 1>(a, p, bx, by, bz);
				} else {
					p.j == 4 ? run_tile<LW_RS_ROUTE_GLOBAL_TAPS, 4>(a, p, bx, by, bz)
					: p.j == 2 ? run_tile<LW_RS_ROUTE_GLOBAL_TAPS, 2>(a, p, bx, by, bz)
					           : run_tile<LW_RS_ROUTE_GLOBAL_TAPS, 1>(a, p, bx, by, bz);
				}
			}
	return hipSuccess;
}

static lw_resampler *make(char **v, int *err)
{
	return lw_resampler_create(0, (uint32_t)strtoul(v[0], nullptr, 10), (uint32_t)strtoul(v[1], nullptr, 10), (uint32_t)strtoul(v[2], nullptr, 10),
			strtod(v[3], nullptr), atoi(v[4]), strtod(v[5], nullptr), err);
}

static uint32_t bits(float f)
{
	uint32_t u;
	memcpy(&u, &f, 4);
	return u;
}

// the contract, scalar: output n of a row of len samples x (stride el)
static float fold(const std::vector<float> &taps, uint32_t orig, uint32_t new_, uint32_t W, uint32_t K, const float *x, uint64_t el, uint64_t len, uint64_t n)
{
	const unsigned __int128 p = (unsigned __int128)n * orig;
	const int64_t base = (int64_t)(p / new_);
	const uint32_t ph = (uint32_t)(p % new_);
	float acc = 0;
	for (uint32_t k = 0; k < K; k++) {
		const int64_t i = base - (int64_t)W + k;
		const float xv = i >= 0 && (uint64_t)i < len ? x[(uint64_t)i * el] : 0.0f;
		const float t = taps[(size_t)ph * K + k] * xv;
		acc = k == 0 ? t : acc + t;
	}
	return acc;
}

static const uint32_t PAIRS[][2] = {{44100, 16000}, {48000, 16000}, {44100, 48000}, {16000, 44100}, {22050, 44100}, {48000, 44100},
	{2000, 1}, {16000, 16000}}; // the last two: the all-global route and the copy
static const uint32_t SENT = SENT_ABC;

static int kernel_cases(unsigned seed, int cases)
{
	std::mt19937 rng(seed);
	auto rnd = [&](uint32_t lo, uint32_t hi) { return lo + (uint32_t)(rng() % (hi - lo + 1)); };
	int done = 0;
	for (int c = 0; c < cases; c++) {
		const uint32_t *pair = PAIRS[c < 8 ? c : rnd(0, 7)];
		const int window = (c / 8 + c) & 1;
		const bool big = pair[0] == 2000;
		int err = 0;
		lw_resampler *rs = lw_resampler_create(0, pair[0], pair[1], window || big ? (big ? 6 : 16) : 6, 0.99, big ? 0 : window, 14.769656459379492, &err);
		if (!rs)
			bad("create %d", err);
		uint32_t orig, new_, W, K;
		lw_resampler_geometry(rs, &orig, &new_, &W, &K);
		std::vector<float> taps(lw_resampler_taps(rs, nullptr));
		lw_resampler_taps(rs, taps.data());
		const bool force_global_taps = (c & 2) != 0;
		lw_resampler_set_taps_in_lds(rs, !force_global_taps);
		const int fmt = (c & 1) ? LW_FMT_F32_INTERLEAVED : LW_FMT_F32_PLANAR;
		const bool itl = fmt == LW_FMT_F32_INTERLEAVED;
		const uint32_t ch = rnd(1, 6), rows = rnd(1, 3), extra = rnd(0, 2);
		std::vector<uint64_t> len(rows);
		uint64_t longest = 0, longest_out = 0;
		for (auto &l : len) {
			const uint32_t kind = rnd(0, 5);
			l = kind == 0 ? 0 : kind == 1 ? rnd(1, W + 1) : rnd(0, 3000);
			longest = std::max(longest, l);
			longest_out = std::max(longest_out, lw_resampler_out_len(rs, l));
		}
		const size_t scap = (longest + rnd(0, 9)) | 1, dcap = (longest_out + rnd(0, 9)) | 1; // odd capacities
		std::vector<uint32_t> map(rows);
		for (uint32_t r = 0; r < rows; r++)
			map[r] = (r * 2 + 1) % (rows + extra);
		{ // a permuted order where that is one-to-one, the reversed order where not
			std::vector<bool> seen(rows + extra, false);
			bool distinct = true;
			for (uint32_t r = 0; r < rows; r++) {
				distinct = distinct && !seen[map[r]];
				seen[map[r]] = true;
			}
			if (!distinct)
				for (uint32_t r = 0; r < rows; r++)
					map[r] = rows - 1 - r;
		}
		// exact-size buffers: one element beyond either is an ASan report
		const size_t sn = (size_t)rows * ch * scap, dn = (size_t)(rows + extra) * ch * dcap;
		float *src = (float *)malloc(sn * 4), *dst = (float *)malloc(dn * 4), *want = (float *)malloc(dn * 4);
		fill32(src, sn, SENT), fill32(dst, dn, SENT), fill32(want, dn, SENT);
		std::uniform_real_distribution<float> uni(-1.0f, 1.0f);
		for (uint32_t r = 0; r < rows; r++)
			for (uint32_t q = 0; q < ch; q++) {
				const float *x = src + (itl ? ((size_t)r * scap) * ch + q : ((size_t)r * ch + q) * scap);
				const uint64_t el = itl ? ch : 1;
				const uint32_t kind = rnd(0, 3);
				for (uint64_t i = 0; i < len[r]; i++) {
					float v = kind == 0 ? (i == len[r] / 2 ? 1.0f : 0.0f) : kind == 1 ? uni(rng) * 1e-39f : uni(rng);
					if (kind == 2 && (i & 7) == 0)
						v = -0.0f;
					((float *)x)[i * el] = v;
				}
				float *y = want + (itl ? ((size_t)map[r] * dcap) * ch + q : ((size_t)map[r] * ch + q) * dcap);
				const uint64_t out = lw_resampler_out_len(rs, len[r]);
				for (uint64_t n = 0; n < out; n++) {
					const float v = orig == new_ ? x[n * el] : fold(taps, orig, new_, W, K, x, el, len[r], n);
					y[n * el] = v;
				}
			}
		const int rc = lw_resample_rows(rs, fmt, ch, src, rows, scap, len.data(), map.data(), dst, rows + extra, dcap, nullptr);
		const int route = lw_resampler_last_route(rs);
		printf("CASE %d %u->%u w%d fmt%d ch%u rows%u route %d rc %d\n", c, pair[0], pair[1], window, fmt, ch, rows, route, rc);
		if (rc != LW_OK)
			return 3;
		for (size_t i = 0; i < dn; i++)
			if (bits(dst[i]) != bits(want[i]))
				bad("element %zu: %08x, expected %08x", i, bits(dst[i]), bits(want[i]));
		free(src), free(dst), free(want);
		lw_resampler_destroy(rs);
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
	if (mode == "create" && argc >= 8) {
		lw_resampler *rs = make(argv + 2, &err);
		printf("RC %d\n", err);
		if ((rs == nullptr) != (err != 0))
			return 3;
		lw_resampler_destroy(rs);
		return 0;
	}
	if ((mode == "taps" && argc >= 9) || (mode == "outlen" && argc >= 8) || (mode == "index" && argc >= 8)) {
		lw_resampler *rs = make(argv + 2, &err);
		if (!rs)
			return 2;
		uint32_t orig, new_, W, K;
		lw_resampler_geometry(rs, &orig, &new_, &W, &K);
		if (mode == "taps") {
			printf("G %u %u %u %u\n", orig, new_, W, K);
			std::vector<float> taps(lw_resampler_taps(rs, nullptr));
			if (taps.size() != (size_t)new_ * K || lw_resampler_taps(rs, taps.data()) != taps.size())
				return 3;
			File(argv[8], "wb").put(taps.data(), taps.size());
		} else if (mode == "outlen") {
			for (int i = 8; i < argc; i++) {
				const uint64_t len = strtoull(argv[i], nullptr, 10);
				printf("L %llu %llu\n", (unsigned long long)len, (unsigned long long)lw_resampler_out_len(rs, len));
			}
		} else {
			LwResampleRow row{UINT64_MAX, UINT64_MAX, 0};
			for (int pass = 0; pass < 3; pass++) {
				LwResamplePlan p = lw_resample_plan(orig, new_, K, pass == 0);
				if (pass == 2) // the all-global route's index, whatever the plan
					p.route = LW_RS_ROUTE_GLOBAL, p.j = 1, p.blocks = 1, p.tile = LW_RS_THREADS;
				LwResampleArgs a{};
				a.rows = &row, a.orig = orig, a.new_ = new_, a.half_width = W, a.k_taps = K, a.blocks = p.blocks;
				a.s = a.d = LwResampleLayout{0, 0, 1};
				for (int i = 8; i < argc; i++) {
					const uint64_t n = strtoull(argv[i], nullptr, 10);
					int64_t base;
					uint32_t ni;
					if (p.route == LW_RS_ROUTE_GLOBAL) {
						base = lw_rs_global_index(a, n, ni) + W;
					} else if (p.route == LW_RS_ROUTE_COPY) {
						continue;
					} else {
						LwRsTile t;
						const uint64_t bx = n / p.tile, r = n - bx * p.tile;
						const uint32_t units = p.blocks * new_, j = (uint32_t)(r / units);
						uint32_t x_at;
						if (bx > UINT32_MAX || !lw_rs_tile(a, p.tile, (uint32_t)bx, 0, 0, t))
							return 3;
						const uint64_t first = lw_rs_unit(a, t, (uint32_t)(r % units), ni, x_at);
						if (first + (uint64_t)j * units != n || x_at + j * p.blocks * orig + K - 1 >= p.span)
							return 3;
						base = t.x0 + (int64_t)W + x_at + (int64_t)j * p.blocks * orig;
					}
					printf("I %llu %lld %u %d\n", (unsigned long long)n, (long long)base, ni, p.route);
				}
			}
		}
		lw_resampler_destroy(rs);
		return 0;
	}
	if (mode == "kernel" && argc >= 4)
		return kernel_cases((unsigned)atoi(argv[2]), atoi(argv[3]));
	// ---- calls on a small fixture: 3 rows of 2 channels, 44100 -> 16000
	lw_resampler *rs = lw_resampler_create(0, 44100, 16000, 6, 0.99, LW_RESAMPLE_HANN, 0, &err);
	if (!rs)
		return 2;
	const size_t scap = 1001, dcap = 401;
	std::vector<float> src(3 * 2 * scap, 0.25f), dst(4 * 2 * dcap, 0.0f);
	uint64_t len[3] = {1000, 0, 441};
	uint32_t map[3] = {2, 0, 3};
	if (mode == "two") {
		g_log.run = false;
		uint64_t len_b[3] = {7, 8, 9};
		int rc = lw_resample_rows(rs, LW_FMT_F32_PLANAR, 2, src.data(), 3, scap, len, map, dst.data(), 4, dcap, nullptr);
		printf("RC %d\n", rc);
		len[0] = 1; // the first call has copied its lengths: the caller's are free
		rc = lw_resample_rows(rs, LW_FMT_F32_INTERLEAVED, 2, src.data(), 3, scap, len_b, nullptr, dst.data(), 4, dcap, nullptr);
		printf("RC %d\n", rc);
		g_log.print([](const LwResampleRow &r) { printf(" %llu/%llu/%llu", (unsigned long long)r.len, (unsigned long long)r.out_len, (unsigned long long)r.dst_row); });
	} else if (mode == "refuse" && argc >= 3) {
		const std::string cs = argv[2];
		int fmt = LW_FMT_F32_PLANAR;
		uint32_t ch = 2;
		const void *s = src.data();
		void *d = dst.data();
		const uint64_t *l = len;
		const uint32_t *mp = map;
		size_t n_dst = 4, sc = scap, dc = dcap;
		lw_resampler *h = rs;
		if (cs == "null_rs")
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
		else if (cs == "out_over")
			dc = 362; // out_len(1000) = 363
		else if (cs == "row_over")
			map[2] = 4;
		else if (cs == "row_over_identity")
			mp = nullptr, n_dst = 2;
		else if (cs == "row_twice")
			map[2] = 2;
		else if (cs == "row_twice_empty")
			map[1] = 3; // the row without samples names a row another one has
		else if (cs == "ok_many_tiles") {
			// one row of 2^37 outputs: more tiles than one launch holds, whatever the plan's tile (nothing runs here, no sample is touched)
			g_log.run = false;
			dc = (size_t)1 << 37, len[0] = sc = ((size_t)1 << 37) / 160 * 441, len[1] = len[2] = 0;
		} else if (cs != "ok" && cs != "ok_exact")
			return 2;
		if (cs == "ok_exact")
			dc = 363, sc = 1000;
		const int rc = lw_resample_rows(h, fmt, ch, s, 3, sc, l, mp, d, n_dst, dc, nullptr);
		printf("RC %d\nLAUNCHES %d\n", rc, g_log.launches);
		if (cs == "ok_many_tiles") {
			uint32_t orig, new_, hw, k;
			lw_resampler_geometry(rs, &orig, &new_, &hw, &k);
			printf("TILE %u\n", lw_resample_plan(orig, new_, k, 1).tile);
			for (const auto &g : g_tiles)
				printf("TILES %u %u\n", g.first, g.second);
		}
	} else {
		return 2;
	}
	lw_resampler_destroy(rs);
	return 0;
}
