// The Kaldi-compatible front end of lw_spec WITHOUT a GPU (lw_spec_create_ex: Kaldi framing, symmetric padding, folded
// pre-emphasis / window / scale, DC removal and energy; include/lewton_amd.h "spectral frames of rows"): lw_spec.cpp linked against
// hip_standins.inc and the kernel source, lw_kernels_spec.hip, compiled for the host (LW_SPEC_HOST: the route with per-lane fmaf
// chains) and run workgroup by workgroup, lane by lane, phase by phase in the kernel's own order, the prologue's four phases
// included, with an LDS buffer of exactly the kernel's size and exact-size source and destination buffers, as
// tests/san/spec_host.cpp does.  A stand-alone program built with -fsanitize=address,undefined; tests/test_host_fbank.py drives it.
//   P = NFFT WIN HOP WINDOW CENTER FRAMING DC ENERGY RESERVED PREEMPH SCALE   (eleven arguments: a lw_spec_params without a matrix)
//   fbank_host create P                 "RC err"
//   fbank_host legacy NFFT WIN HOP WINDOW CENTER   "SAME n": lw_spec_create's table and lw_spec_create_ex's with the defaults, compared
//                                       byte for byte (n floats), and lw_spec_frames of both for len 0 .. 4 NFFT
//   fbank_host basis P FILE             "G bins features pad_mode" and the table [2][WIN][B] as raw f32 into FILE
//   fbank_host frames P LO HI           "L len n_frames first last" for LO <= len <= HI: lw_spec_frames, and the first and last
//                                       input index by the kernel's own lw_sp_tile / lw_sp_index (0 0 without frames)
//   fbank_host accept P LEN             "RC rc", "LAUNCHES n": two rows, the LAST of LEN samples
//   fbank_host padmode P MODE           "RC rc MODE m": lw_spec_set_pad_mode, and the mode afterwards
//   fbank_host run P NMELS FB CH ITL IN OUT LEN...   rows of CH channels, raw f32 IN as [row][CH][cap], cap = the longest LEN + 3 (the
//                                       caller's poison between len and cap), ITL 1: handed over interleaved; FB raw f32
//                                       [NMELS][B] ("-" with NMELS 0); the destination [row + 1][CH][F][fcap], fcap = the most frames
//                                       + 1, sentinel-filled, as raw f32 into OUT.  "RC rc", "F features fcap", "LAUNCHES n"
#include "../../include/lewton_amd.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "hip_standins.inc"
#include "kernel_host.hpp"

#define LW_SPEC_HOST 1
#include "../../lewton_amd/csrc/lw_kernels_spec.hip"

static LaunchLog<LwSpecRow> g_log;

static void run_tile(const LwSpecArgs &a, uint32_t bx, uint32_t by, uint32_t bz)
{
	LwSpTile t;
	if (!lw_sp_tile(a, bx, by, bz, t))
		return;
	float *lds = (float *)malloc((size_t)LW_SP_LDS_FLOATS * 4); // exactly the kernel's size: one float beyond it is an ASan report
	for (size_t i = 0; i < LW_SP_LDS_FLOATS; i++)
		lds[i] = NAN; // LDS holds garbage at launch
	std::vector<LwSpLane> st(LW_SP_THREADS);
	std::vector<float> mu0(LW_SP_THREADS, 0.0f), mu1(LW_SP_THREADS, 0.0f);
	const uint32_t T = LW_SP_THREADS;
	const bool pro = a.remove_dc || a.energy;
	for (uint32_t tid = 0; tid < T; tid++)
		lw_sp_zero_mel(st[tid]);
	if (pro) {
		for (uint32_t tid = 0; tid < T; tid++)
			lw_sp_pro_span(a, t, tid, lds);
		for (uint32_t tid = 0; tid < T; tid++)
			lw_sp_pro_sums(a, t, tid, lds);
		for (uint32_t tid = 0; tid < T; tid++)
			lw_sp_pro_finish(a, t, tid, lds);
		for (uint32_t tid = 0; tid < T; tid++)
			lw_sp_pro_mu(tid, lds, mu0[tid], mu1[tid]);
	}
	for (uint32_t pass = 0; pass < a.passes; pass++) {
		for (uint32_t tid = 0; tid < T; tid++)
			lw_sp_zero_acc(st[tid]);
		for (uint32_t kt = 0; kt < a.k_pad / LW_SP_KT; kt++) {
			for (uint32_t tid = 0; tid < T; tid++) {
				if (pro)
					lw_sp_stage<LW_SP_PAD_ARGS, 1>(a, t, pass, kt, tid, lds, mu0[tid], mu1[tid]);
				else
					lw_sp_stage(a, t, pass, kt, tid, lds);
			}
			for (uint32_t tid = 0; tid < T; tid++)
				lw_sp_mma<LW_SP_ROUTE_FMA>(a, pass, tid, lds, st[tid]);
		}
		for (uint32_t tid = 0; tid < T; tid++)
			lw_sp_power(a, pass, tid, lds, st[tid]);
		if (a.n_mels == 0) {
			for (uint32_t tid = 0; tid < T; tid++) {
				if (pro)
					lw_sp_store_power<1>(a, t, pass, tid, lds);
				else
					lw_sp_store_power(a, t, pass, tid, lds);
			}
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
		for (uint32_t tid = 0; tid < T; tid++) {
			if (pro)
				lw_sp_store_mel<1>(a, t, tid, st[tid]);
			else
				lw_sp_store_mel(a, t, tid, st[tid]);
		}
	free(lds);
}

hipError_t lw_launch_spec(const LwSpecArgs &a, int route, uint32_t tiles, uint32_t ch, uint32_t n_rows, hipStream_t)
{
	g_log.launch();
	if (!a.rows || !a.basis || (a.n_mels && !a.fb) || route != LW_SP_ROUTE_FMA || ch == 0 || n_rows > 65535u || a.k_pad % LW_SP_KT || a.mel_pad % 32u ||
			a.pad_mode > 2u || (a.span && (a.span != (LW_SP_TF - 1u) * a.hop + a.win_length || !lw_spec_span_fits(a.hop, a.win_length))))
		bad("arguments");
	for (uint32_t bz = 0; bz < n_rows; bz++)
		for (uint32_t by = 0; by < ch; by++)
			for (uint32_t bx = 0; bx < tiles; bx++)
				run_tile(a, bx, by, bz);
	return hipSuccess;
}

static lw_spec_params params(char **v)
{
	lw_spec_params p{};
	p.n_fft = (uint32_t)strtoul(v[0], nullptr, 10), p.win_length = (uint32_t)strtoul(v[1], nullptr, 10), p.hop = (uint32_t)strtoul(v[2], nullptr, 10);
	p.window = atoi(v[3]), p.center = atoi(v[4]), p.framing = atoi(v[5]), p.remove_dc = atoi(v[6]), p.energy = atoi(v[7]);
	p.reserved = (uint32_t)strtoul(v[8], nullptr, 10);
	p.preemphasis = strtod(v[9], nullptr), p.scale = strtod(v[10], nullptr); // ("nan" and "inf" are read as such)
	return p;
}

int main(int argc, char **argv)
{
	if (argc < 2)
		return 2;
	const std::string mode = argv[1];
	int err = 0;
	if (mode == "legacy" && argc >= 7) {
		const uint32_t n_fft = (uint32_t)strtoul(argv[2], nullptr, 10), win = (uint32_t)strtoul(argv[3], nullptr, 10), hop = (uint32_t)strtoul(argv[4], nullptr, 10);
		lw_spec_params p{};
		p.n_fft = n_fft, p.win_length = win, p.hop = hop, p.window = atoi(argv[5]), p.center = atoi(argv[6]), p.scale = 1.0;
		lw_spec *a = lw_spec_create(0, n_fft, win, hop, p.window, p.center, 0, nullptr, &err), *b = lw_spec_create_ex(0, &p, &err);
		if (!a || !b)
			return 3;
		std::vector<float> ta(lw_spec_basis(a, nullptr)), tb(lw_spec_basis(b, nullptr));
		if (ta.size() != tb.size() || ta.size() != (size_t)2 * win * (n_fft / 2 + 1) || lw_spec_basis(a, ta.data()) != ta.size() || lw_spec_basis(b, tb.data()) != tb.size() ||
				memcmp(ta.data(), tb.data(), ta.size() * 4) || lw_spec_features(a) != lw_spec_features(b) || lw_spec_pad_mode(b) != LW_SPEC_PAD_ZERO)
			return 3;
		for (uint64_t len = 0; len <= 4ull * n_fft; len++)
			if (lw_spec_frames(a, len) != lw_spec_frames(b, len))
				return 3;
		printf("SAME %zu\n", ta.size());
		lw_spec_destroy(a), lw_spec_destroy(b);
		return 0;
	}
	if (argc < 13)
		return 2;
	lw_spec_params p = params(argv + 2);
	char **rest = argv + 13;
	const int n_rest = argc - 13;
	if (mode == "create") {
		lw_spec *sp = lw_spec_create_ex(0, &p, &err);
		printf("RC %d\n", err);
		if ((sp == nullptr) != (err != 0))
			return 3;
		lw_spec_destroy(sp);
		if (lw_spec_create_ex(0, nullptr, &err) || err != LW_ERR_NULL_ARG)
			return 3;
		return 0;
	}
	if (mode == "run" && n_rest >= 7) {
		p.n_mels = (uint32_t)strtoul(rest[0], nullptr, 10);
		std::vector<float> fb;
		if (p.n_mels) {
			fb = slurp_f32(rest[1]);
			if (fb.size() != (size_t)p.n_mels * (p.n_fft / 2 + 1))
				return 2;
			p.fb = fb.data();
		}
		lw_spec *sp = lw_spec_create_ex(0, &p, &err);
		if (!sp || lw_spec_set_route(sp, LW_SP_ROUTE_FMA) != LW_OK)
			return 3;
		const uint32_t ch = (uint32_t)strtoul(rest[2], nullptr, 10);
		const bool itl = atoi(rest[3]) != 0;
		std::vector<uint64_t> len;
		for (int i = 6; i < n_rest; i++)
			len.push_back(strtoull(rest[i], nullptr, 10));
		const size_t rows = len.size(), cap = (size_t)*std::max_element(len.begin(), len.end()) + 3;
		const std::vector<float> in = slurp_f32(rest[4]);
		if (in.size() != rows * ch * cap)
			return 2;
		float *src = (float *)malloc(in.size() * 4); // exact size: an index beyond the buffer is an ASan report
		for (size_t r = 0; r < rows; r++)
			for (size_t c = 0; c < ch; c++)
				for (size_t i = 0; i < cap; i++)
					src[itl ? (r * cap + i) * ch + c : (r * ch + c) * cap + i] = in[(r * ch + c) * cap + i];
		uint64_t most = 0;
		for (auto l : len)
			most = std::max(most, lw_spec_frames(sp, l));
		const size_t F = lw_spec_features(sp), fcap = (size_t)most + 1, dn = (rows + 1) * ch * F * fcap;
		float *dst = (float *)malloc(dn * 4);
		fill32(dst, dn, SENT_DEAD);
		const int rc = lw_spec_rows(sp, itl ? LW_FMT_F32_INTERLEAVED : LW_FMT_F32_PLANAR, ch, src, rows, cap, len.data(), nullptr, dst, rows + 1, fcap, nullptr);
		printf("RC %d\nF %zu %zu\nLAUNCHES %d\n", rc, F, fcap, g_log.launches);
		File(rest[5], "wb").put(dst, dn);
		free(src), free(dst);
		lw_spec_destroy(sp);
		return 0;
	}
	lw_spec *sp = lw_spec_create_ex(0, &p, &err);
	if (!sp)
		return 3;
	if (mode == "basis" && n_rest >= 1) {
		printf("G %u %u %d\n", lw_spec_bins(sp), lw_spec_features(sp), lw_spec_pad_mode(sp));
		std::vector<float> b(lw_spec_basis(sp, nullptr));
		if (b.size() != (size_t)2 * p.win_length * lw_spec_bins(sp) || lw_spec_basis(sp, b.data()) != b.size())
			return 3;
		File(rest[0], "wb").put(b.data(), b.size());
	} else if (mode == "frames" && n_rest >= 2) {
		const bool snip = p.framing == LW_SPEC_FRAMES_KALDI_SNIP;
		for (uint64_t len = strtoull(rest[0], nullptr, 10); len <= strtoull(rest[1], nullptr, 10); len++) {
			const uint64_t T = lw_spec_frames(sp, len);
			long long first = 0, last = 0;
			if (T) {
				LwSpecRow row{len, T, 0};
				LwSpecArgs a{};
				a.rows = &row, a.hop = p.hop, a.s = LwSpecLayout{0, 0, 1}, a.lead = lw_spec_kaldi_lead(p.win_length, p.hop, snip);
				LwSpTile t0, t1;
				if (!lw_sp_tile(a, 0, 0, 0, t0) || !lw_sp_tile(a, (uint32_t)((T - 1) / LW_SP_TF), 0, 0, t1))
					return 3;
				first = lw_sp_index(a, t0, 0, 0), last = lw_sp_index(a, t1, (uint32_t)((T - 1) % LW_SP_TF), p.win_length - 1);
			}
			printf("L %llu %llu %lld %lld\n", (unsigned long long)len, (unsigned long long)T, first, last);
		}
	} else if (mode == "accept" && n_rest >= 1) {
		if (lw_spec_set_route(sp, LW_SP_ROUTE_FMA) != LW_OK)
			return 3;
		const uint64_t len[2] = {(uint64_t)p.win_length * 4, strtoull(rest[0], nullptr, 10)}; // (the LAST row is the short one)
		const size_t cap = (size_t)std::max(len[0], len[1]), fcap = (size_t)std::max(lw_spec_frames(sp, len[0]), lw_spec_frames(sp, len[1])), F = lw_spec_features(sp);
		std::vector<float> x(2 * cap, 0.5f), y(2 * F * fcap + 1, 0.0f);
		const int rc = lw_spec_rows(sp, LW_FMT_F32_PLANAR, 1, x.data(), 2, cap, len, nullptr, y.data(), 2, fcap, nullptr);
		printf("RC %d\nLAUNCHES %d\n", rc, g_log.launches);
	} else if (mode == "padmode" && n_rest >= 1) {
		const int rc = lw_spec_set_pad_mode(sp, atoi(rest[0]));
		printf("RC %d MODE %d\n", rc, lw_spec_pad_mode(sp));
	} else {
		return 2;
	}
	lw_spec_destroy(sp);
	return 0;
}
