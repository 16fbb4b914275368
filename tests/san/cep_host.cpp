// Cepstra and deltas of feature rows WITHOUT a GPU: lw_cep.cpp linked against hip_standins.inc (device memory = calloc), and the
// KERNEL source itself, lw_kernels_cep.hip, compiled for the host (LW_CEP_HOST): the stand-in for the launcher below runs it
// workgroup by workgroup, the phases of a group in the kernel's own order (every lane of a phase before the next: the barrier),
// each lane's values kept in an array of its own and the LDS image an exact-size allocation, so AddressSanitizer sees every load
// and store the kernel makes.  Built with -fsanitize=address,undefined; tests/test_host_cep.py drives it.
//   cep_host create N_IN N_OUT MATRIX ORDER WIDTH [DEVICE]   "RC err"; MATRIX: "null", or "ones" (the stand-ins have ONE device, 0)
//   cep_host weights N              "W bits..." of lw_cep_delta_weights as hex, and "N n"
//   cep_host refuse CASE            "RC rc", "LAUNCHES n", "LAST n": CASE is one of the refusals of lw_cep_rows (main below)
//   cep_host two                    two calls queued back to back: "ROWS n/fill_end..." per launch, read at the end
//   cep_host run N_IN N_OUT IDENTITY ORDER WIDTH CH ROWS CAP FILL SHIFT_SRC SHIFT_DST IN OUT
//                                   IN: u64 n[ROWS], u64 fill_to[ROWS], f32 matrix[N_OUT][N_IN], f32 x[ROWS][CH][N_IN][CAP];  OUT:
//                                   the destination, sentinel-filled before the call.  The buffers are exact-size, start SHIFT
//                                   elements behind a 16-byte boundary and have a guarded front.  "RC rc", "LAUNCHES n", "TILE n"
#include "../../include/lewton_amd.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "hip_standins.inc"
#include "kernel_host.hpp"

#define LW_CEP_HOST 1
#include "../../lewton_amd/csrc/lw_kernels_cep.hip"

static LaunchLog<LwCepRow> g_log;

// one group of one workgroup, as lw_cp_group runs it on the device
template <int G>
static void group(const LwCepArgs &a, const LwCpTile &t, const float *mt, const float *src, float *dst, float *lds, uint32_t q0, uint32_t g)
{
	std::vector<float> vals((size_t)LW_CP_THREADS * G, 0.0f);
	auto v = [&](uint32_t tid) -> float(&)[G] { return *(float(*)[G])(vals.data() + (size_t)tid * G); };
	if (!t.data) {
		for (uint32_t tid = 0; tid < LW_CP_THREADS; tid++)
			for (uint32_t level = 0; level <= a.order; level++)
				lw_cp_store<G>(a, t, dst, q0, g, level, tid, v(tid));
		return;
	}
	for (uint32_t tid = 0; tid < LW_CP_THREADS; tid++) {
		lw_cp_static<G>(a, t, mt, src, q0, g, lw_cp_frame(t, tid), v(tid));
		lw_cp_store<G>(a, t, dst, q0, g, 0, tid, v(tid));
	}
	float *img = lds;
	for (uint32_t level = 1; level <= a.order; level++, img += a.plan.group * LW_CP_THREADS) {
		for (uint32_t tid = 0; tid < LW_CP_THREADS; tid++)
			lw_cp_put<G>(img, tid, v(tid));
		for (uint32_t tid = 0; tid < LW_CP_THREADS; tid++) // (behind the barrier)
			if (lw_cp_has(a, level, tid)) {
				lw_cp_delta<G>(a, t, img, lw_cp_frame(t, tid), v(tid));
				lw_cp_store<G>(a, t, dst, q0, g, level, tid, v(tid));
			}
	}
}

hipError_t lw_launch_cep(const LwCepArgs &a, const float *mt, const float *src, float *dst, uint32_t tiles, uint32_t n_rows, hipStream_t)
{
	g_log.launch(a.rows + a.row0, n_rows);
	const LwCepPlan p = lw_cep_plan(a.n_out, a.order, a.width);
	if (!a.rows || n_rows == 0 || n_rows > 65535u || tiles == 0 || !dst || (a.identity ? a.n_in != a.n_out : !mt) || p.tile != a.plan.tile ||
			p.halo != a.plan.halo || p.group != a.plan.group || p.lds != a.plan.lds || a.mt_stride < ((a.n_out + 31u) & ~31u))
		bad("arguments");
	if (!g_log.run)
		return hipSuccess;
	float *lds = (float *)malloc(a.plan.lds ? a.plan.lds : 1); // exact size: one float beyond the images is a report
	for (uint32_t bz = 0; bz < n_rows; bz++)
		for (uint32_t by = 0; by < a.ch; by++)
			for (uint32_t bx = 0; bx < tiles; bx++) {
				LwCpTile t;
				if (!lw_cp_tile(a, bx, by, bz, t))
					continue;
				for (uint32_t q0 = 0; q0 < a.n_out; q0 += LW_CP_GROUP) {
					const uint32_t left = a.n_out - q0, g = left < LW_CP_GROUP ? left : LW_CP_GROUP;
					if (g > 24u)
						group<32>(a, t, mt, src, dst, lds, q0, g);
					else if (g > 16u)
						group<24>(a, t, mt, src, dst, lds, q0, g);
					else if (g > 8u)
						group<16>(a, t, mt, src, dst, lds, q0, g);
					else
						group<8>(a, t, mt, src, dst, lds, q0, g);
				}
			}
	free(lds);
	return hipSuccess;
}

static const uint32_t SENT = SENT_DEAD;

int main(int argc, char **argv)
{
	if (argc < 2)
		return 2;
	const std::string mode = argv[1];
	int err = 0;
	if (mode == "create" && argc >= 7) {
		const uint32_t n_in = (uint32_t)strtoul(argv[2], nullptr, 10), n_out = (uint32_t)strtoul(argv[3], nullptr, 10);
		std::vector<float> ones((size_t)(n_in ? n_in : 1) * (n_out ? n_out : 1), 1.0f);
		lw_cep *cp = lw_cep_create(argc >= 8 ? atoi(argv[7]) : 0, n_in, n_out, std::string(argv[4]) == "null" ? nullptr : ones.data(),
				(uint32_t)strtoul(argv[5], nullptr, 10), (uint32_t)strtoul(argv[6], nullptr, 10), &err);
		printf("RC %d\n", err);
		if ((cp == nullptr) != (err != 0))
			return 3;
		if (cp && lw_cep_features(cp) != n_out * (1 + (uint32_t)strtoul(argv[5], nullptr, 10)))
			return 3;
		lw_cep_destroy(cp);
		return 0;
	}
	if (mode == "weights" && argc >= 3) {
		const uint32_t N = (uint32_t)atoi(argv[2]);
		lw_cep *cp = lw_cep_create(0, 4, 4, nullptr, N ? 1 : 0, N, &err);
		if (!cp)
			return 2;
		float w[LW_CEP_MAX_WIDTH + 1];
		for (auto &v : w)
			memcpy(&v, &SENT, 4);
		const uint32_t n = lw_cep_delta_weights(cp, w);
		if (lw_cep_delta_weights(cp, nullptr) != n || lw_cep_delta_weights(nullptr, w) != 0 || memcmp(&w[n], &SENT, 4))
			return 3;
		printf("W");
		for (uint32_t i = 0; i < n; i++) {
			uint32_t b;
			memcpy(&b, &w[i], 4);
			printf(" %08x", b);
		}
		printf("\nN %u\n", n);
		if (lw_cep_matrix(cp, nullptr) != 0 || lw_cep_tile_frames(cp) != 256 - 2 * N || lw_cep_tile_frames(nullptr) != 0 || lw_cep_features(nullptr) != 0)
			return 3;
		lw_cep_destroy(cp);
		return 0;
	}
	if (mode == "run" && argc >= 15) {
		const uint32_t n_in = (uint32_t)atoi(argv[2]), n_out = (uint32_t)atoi(argv[3]);
		const bool identity = atoi(argv[4]) != 0;
		const uint32_t order = (uint32_t)atoi(argv[5]), width = (uint32_t)atoi(argv[6]), ch = (uint32_t)atoi(argv[7]);
		const size_t rows = (size_t)atoll(argv[8]), cap = (size_t)atoll(argv[9]);
		const bool fill = atoi(argv[10]) != 0;
		const size_t ns = rows * ch * n_in * cap, nd = rows * ch * n_out * (1 + order) * cap;
		std::vector<uint64_t> cnt(rows + 1), fill_to(rows + 1);
		std::vector<float> m((size_t)n_out * n_in);
		const Guarded gs = shifted(4 * ns, 4u * (unsigned)atoi(argv[11])), gd = shifted(4 * nd, 4u * (unsigned)atoi(argv[12]));
		{
			File in(argv[13], "rb");
			in.get(cnt.data(), rows), in.get(fill_to.data(), rows), in.get(m.data(), m.size()), in.get(gs.as<float>(), ns);
		}
		lw_cep *cp = lw_cep_create(0, n_in, n_out, identity ? nullptr : m.data(), order, width, &err);
		if (!cp)
			return 2;
		std::fill(m.begin(), m.end(), 0.0f); // the matrix was copied at creation: the caller's is free
		if (!identity) {
			std::vector<float> back((size_t)n_out * n_in + 1);
			memcpy(&back.back(), &SENT, 4);
			if (lw_cep_matrix(cp, nullptr) != m.size() || lw_cep_matrix(cp, back.data()) != m.size() || memcmp(&back.back(), &SENT, 4))
				return 3;
		}
		fill32(gd.at, nd, SENT);
		const int rc = lw_cep_rows(cp, ch, gs.at, gd.at, rows, cap, cnt.data(), fill ? fill_to.data() : nullptr, nullptr);
		printf("RC %d\nLAUNCHES %d\nTILE %u\n", rc, g_log.launches, lw_cep_tile_frames(cp));
		if (rc == LW_OK && lw_cep_last_launches(cp) != g_log.launches)
			return 3;
		File(argv[14], "wb").put(gd.as<float>(), nd);
		if (!guard_intact(gs) || !guard_intact(gd))
			bad("a store in front of a buffer");
		free(gs.base), free(gd.base);
		lw_cep_destroy(cp);
		return 0;
	}
	// ---- calls on a small fixture: 3 rows of 2 channels, 5 lines -> 3 cepstra with deltas and delta-deltas, capacity 300
	std::vector<float> mat(3 * 5, 0.5f);
	lw_cep *cp = lw_cep_create(0, 5, 3, mat.data(), 2, 2, &err);
	if (!cp)
		return 2;
	const size_t cap = 300;
	std::vector<float> src(3 * 2 * 5 * cap, 0.25f), dst(3 * 2 * 9 * cap, 0.0f);
	uint64_t cnt[3] = {300, 0, 4}, fill[3] = {300, 3, 2};
	g_log.run = false;
	if (mode == "two") {
		uint64_t cnt_b[3] = {1, 257, 3};
		int rc = lw_cep_rows(cp, 2, src.data(), dst.data(), 3, cap, cnt, fill, nullptr);
		printf("RC %d LAST %d\n", rc, lw_cep_last_launches(cp));
		cnt[0] = 1, fill[1] = 7; // the first call has copied its arrays: the caller's are free
		rc = lw_cep_rows(cp, 2, src.data(), dst.data(), 3, cap, cnt_b, nullptr, nullptr);
		printf("RC %d LAST %d\n", rc, lw_cep_last_launches(cp));
		g_log.print([](const LwCepRow &r) { printf(" %llu/%llu", (unsigned long long)r.n, (unsigned long long)r.fill_end); });
	} else if (mode == "refuse" && argc >= 3) {
		const std::string cs = argv[2];
		uint32_t ch = 2;
		const void *s = src.data();
		void *d = dst.data();
		const uint64_t *n = cnt, *fl = fill;
		size_t rows = 3, c = cap;
		lw_cep *h = cp, *other = nullptr;
		if (cs == "null_cp")
			h = nullptr;
		else if (cs == "null_n")
			n = nullptr;
		else if (cs == "null_src")
			s = nullptr;
		else if (cs == "null_dst")
			d = nullptr;
		else if (cs == "null_dst_fill_only")
			cnt[0] = cnt[2] = 0, s = nullptr, d = nullptr; // nothing to read, but row 1 is filled to 3
		else if (cs == "n_over")
			cnt[2] = cap + 1; // (the LAST row: every row is checked before anything is queued)
		else if (cs == "fill_over")
			fill[2] = cap + 1;
		else if (cs == "ch0")
			ch = 0;
		else if (cs == "ch256")
			ch = 256;
		else if (cs == "too_large")
			c = (size_t)1 << 62;
		else if (cs == "too_many_tiles")
			c = (size_t)1 << 32, ch = 1, rows = 1, cnt[0] = 0, fill[0] = (uint64_t)248 << 24; // 2^24 tiles to fill, one more than a grid counts
		else if (cs == "ok_most_tiles")
			c = (size_t)1 << 32, ch = 1, rows = 1, cnt[0] = 0, fill[0] = ((uint64_t)248 << 24) - 248; // 2^24 - 1 tiles: accepted
		else if (cs == "ok_nothing")
			cnt[0] = cnt[2] = 0, fl = nullptr, s = nullptr, d = nullptr; // all rows empty, no fill: accepted, nothing queued
		else if (cs == "ok_no_rows")
			rows = 0, n = nullptr;
		else if (cs == "ok_fill_only")
			cnt[0] = cnt[2] = 0, s = nullptr;
		else if (cs == "ok_order0" || cs == "ok_order1") {
			h = other = lw_cep_create(0, 5, 3, mat.data(), cs == "ok_order1" ? 1 : 0, cs == "ok_order1" ? 16 : 0, &err);
			if (!h)
				return 2;
		} else if (cs != "ok")
			return 2;
		const int rc = lw_cep_rows(h, ch, s, d, rows, c, n, fl, nullptr);
		printf("RC %d\nLAUNCHES %d\nLAST %d\n", rc, g_log.launches, lw_cep_last_launches(other ? other : cp));
		lw_cep_destroy(other);
	} else {
		return 2;
	}
	lw_cep_destroy(cp);
	return 0;
}
