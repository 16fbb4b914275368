// lw_rows_synth_mix WITHOUT a GPU: the product sources + lw_rows.cpp + lw_rows_mix.cpp linked against hip_standins.inc (sample
// values are zero, everything the host decides is real), like rows_host.cpp.  The stand-in for lw_launch_rows_mix below prints the
// matrix and the piece list it was handed and checks every piece against the sizes of the source and the destination;
// tests/test_host_rows_mix.py recomputes the expected position mapping from the printed lw_batch_results and the places it chose.
//   usage: rows_mix_host packets.bin FMT results
//          rows_mix_host packets.bin FMT synth places.txt N_ROWS ROW_CAPACITY CASE MATRIX [MATRIX_B]
//   packets.bin: [u32 length][bytes] of the three header packets, then of the audio packets of one stream (one batch, one
//   PreviousWindowRight: the first packet yields no samples)
//   places.txt: one line "row skip keep t0" per audio packet
//   MATRIX: a text file "out_ch in_ch" and then out_ch * in_ch coefficients (out_ch / in_ch are passed on as they stand)
//   CASE: ok | twice | two (MATRIX, then MATRIX_B without synchronising) | plain_between (mix, lw_rows_synth, mix) | refuse |
//         fail (the k_rows_mix launch of the first of two calls fails) |
//         null_mix | null_coef | null_rows | null_place | null_batch | null_r | other_fmt | n_short
//   output: "R status n_samples out_offset" per packet; per k_rows_mix launch "M out_ch in_ch cap itl coefficient bits..." and
//   "P src stride count dst" per piece; "K n" per k_rows launch; "RC rc" per call; "A coefficient bits..." per k_rows_mix launch:
//   what its matrix pointer holds after all calls; "LAUNCHES k_rows_mix k_rows synth" (synth: 1
//   when a synthesis launcher ran in a CASE that is expected to be refused); "N segments copied_elems"
#include "../../include/lewton_amd.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "hip_standins.inc"
#define KERNEL_HOST_NO_HIP_OK 1 // (lw_runtime.cpp is linked)
#include "kernel_host.hpp"

static uint64_t g_src_elems = 0, g_rows = 0;
static int g_mix_launches = 0, g_rows_launches = 0;
static bool g_fail_mix_launch = false; // the next k_rows_mix launch fails, once
static std::vector<std::pair<const float *, uint32_t>> g_coef; // what each k_rows_mix launch was given, looked at again at the end

hipError_t lw_launch_rows(const void *, void *, const LwRowSeg *, uint32_t n_segs, int, hipStream_t)
{
	g_rows_launches++;
	printf("K %u\n", n_segs);
	return hipSuccess;
}

hipError_t lw_launch_rows_mix(const void *d_src, void *d_dst, const LwRowMixPiece *d_pieces, uint32_t n_pieces, const float *d_coef, uint32_t in_ch,
		uint32_t out_ch, uint64_t row_capacity, int elem_size, bool interleaved, hipStream_t)
{
	g_mix_launches++;
	if (g_fail_mix_launch) {
		g_fail_mix_launch = false;
		return hipErrorLaunchFailure;
	}
	if (!d_src || !d_dst || !d_pieces || !d_coef || (elem_size != 2 && elem_size != 4) || out_ch == 0 || out_ch > LW_ROWS_MIX_MAX_OUT || in_ch == 0)
		bad("arguments");
	printf("M %u %u %llu %d", out_ch, in_ch, (unsigned long long)row_capacity, interleaved ? 1 : 0);
	for (uint32_t k = 0; k < out_ch * in_ch; k++) { // (device memory = calloc here, filled by the hipMemcpyAsync stand-in)
		uint32_t bits;
		memcpy(&bits, d_coef + k, 4);
		printf(" %u", bits);
	}
	printf("\n");
	g_coef.emplace_back(d_coef, out_ch * in_ch);
	const uint64_t dst_elems = g_rows * out_ch * row_capacity;
	for (uint32_t i = 0; i < n_pieces; i++) {
		const LwRowMixPiece &p = d_pieces[i];
		printf("P %u %u %u %llu\n", p.src_elem, p.src_stride, p.count, (unsigned long long)p.dst_elem);
		// the last element the wave reads and the last it writes
		const uint64_t n = p.count;
		const uint64_t src_end = interleaved ? p.src_elem + n * in_ch : p.src_elem + (uint64_t)(in_ch - 1) * p.src_stride + n;
		const uint64_t dst_end = interleaved ? p.dst_elem + n * out_ch : p.dst_elem + (uint64_t)(out_ch - 1) * row_capacity + n;
		if (n == 0 || n > LW_ROWS_MIX_PIECE || src_end > g_src_elems || dst_end > dst_elems || dst_end < p.dst_elem ||
				(interleaved ? p.src_stride != 1 : p.src_stride < n))
			bad("piece %u", i);
	}
	return hipSuccess;
}

static std::vector<std::vector<uint8_t>> split_packets(const std::vector<uint8_t> &d)
{
	std::vector<std::vector<uint8_t>> out;
	for (size_t o = 0; o + 4 <= d.size();) {
		uint32_t n;
		memcpy(&n, d.data() + o, 4);
		o += 4;
		if (o + n > d.size())
			break;
		out.emplace_back(d.begin() + o, d.begin() + o + n);
		o += n;
	}
	return out;
}

struct Matrix {
	lw_row_mix mix{};
	std::vector<float> coef;
};

static bool read_matrix(const char *path, Matrix &m)
{
	FILE *f = fopen(path, "r");
	if (!f)
		return false;
	unsigned o = 0, c = 0;
	bool ok = fscanf(f, "%u %u", &o, &c) == 2;
	m.coef.assign(ok ? (size_t)o * c + 1 : 1, 0.0f); // (+ 1: never an empty vector's NULL data())
	for (size_t k = 0; ok && k < (size_t)o * c; k++)
		ok = fscanf(f, "%a", &m.coef[k]) == 1;
	fclose(f);
	m.mix.out_ch = o, m.mix.in_ch = c, m.mix.coef = m.coef.data();
	return ok;
}

int main(int argc, char **argv)
{
	if (argc < 4)
		return 2;
	const auto pk = split_packets(slurp(argv[1]));
	if (pk.size() < 4)
		return 2;
	const int fmt = atoi(argv[2]);
	const std::string mode = argv[3];
	int err = 0;
	lw_ident *id = lw_read_header_ident(pk[0].data(), pk[0].size(), &err);
	lw_ident_info info;
	lw_ident_get_info(id, &info);
	lw_setup *setup = lw_read_header_setup(pk[2].data(), pk[2].size(), info.audio_channels, info.blocksize_0, info.blocksize_1, &err);
	lw_decoder *d = lw_decoder_create(id, setup, 0, &err);
	const size_t n = pk.size() - 3;
	lw_batch *b = lw_batch_create(d, n, fmt, &err);
	lw_pwr *pw = lw_pwr_new(d);
	std::vector<lw_packet> in(n);
	for (size_t i = 0; i < n; i++)
		in[i] = lw_packet{pk[3 + i].data(), pk[3 + i].size(), pw};
	if (lw_batch_entropy(b, in.data(), n, 2) != LW_OK || lw_batch_upload(b, nullptr) != LW_OK)
		return 2;
	const lw_packet_result *res = lw_batch_results(b);
	for (size_t i = 0; i < n; i++)
		printf("R %d %u %llu\n", res[i].status, res[i].n_samples, (unsigned long long)res[i].out_offset);
	if (mode == "synth" && argc >= 9) {
		std::vector<lw_row_place> place;
		if (FILE *f = fopen(argv[4], "r")) {
			unsigned long long row, skip, keep, t0;
			while (fscanf(f, "%llu %llu %llu %llu", &row, &skip, &keep, &t0) == 4)
				place.push_back(lw_row_place{(uint32_t)row, (uint32_t)skip, (uint32_t)keep, 0, (uint64_t)t0});
			fclose(f);
		}
		if (place.size() != n)
			return 2;
		const size_t n_rows = (size_t)strtoull(argv[5], nullptr, 10), cap = (size_t)strtoull(argv[6], nullptr, 10);
		const std::string cs = argv[7];
		Matrix ma, mb;
		if (!read_matrix(argv[8], ma) || (argc > 9 && !read_matrix(argv[9], mb)))
			return 2;
		lw_rows *r = lw_rows_create(d, n, fmt, &err);
		if (!r)
			return 2;
		g_src_elems = lw_batch_out_elems(b);
		g_rows = n_rows;
		void *rows = (void *)(uintptr_t)0x1000; // never dereferenced: the stand-ins launch nothing
		lw_batch *bx = b;
		if (cs == "other_fmt") {
			bx = lw_batch_create(d, n, fmt ^ 1, &err);
			lw_pwr *p2 = lw_pwr_new(d);
			for (size_t i = 0; i < n; i++)
				in[i].pwr = p2;
			if (lw_batch_entropy(bx, in.data(), n, 2) != LW_OK || lw_batch_upload(bx, nullptr) != LW_OK)
				return 2;
			lw_pwr_free(p2);
		}
		// every CASE but these is expected to be refused: armed, the first synthesis launcher that runs takes this to 0
		const bool armed = cs != "ok" && cs != "twice" && cs != "two" && cs != "plain_between" && cs != "fail";
		g_fail_mix_launch = cs == "fail";
		lw_standin_fail_launch.store(armed ? 1 : 0);
		int rc;
		if (cs == "null_mix")
			rc = lw_rows_synth_mix(r, b, place.data(), n, nullptr, rows, n_rows, cap, nullptr);
		else if (cs == "null_coef") {
			lw_row_mix m = ma.mix;
			m.coef = nullptr;
			rc = lw_rows_synth_mix(r, b, place.data(), n, &m, rows, n_rows, cap, nullptr);
		} else if (cs == "null_rows")
			rc = lw_rows_synth_mix(r, b, place.data(), n, &ma.mix, nullptr, n_rows, cap, nullptr);
		else if (cs == "null_place")
			rc = lw_rows_synth_mix(r, b, nullptr, n, &ma.mix, rows, n_rows, cap, nullptr);
		else if (cs == "null_batch")
			rc = lw_rows_synth_mix(r, nullptr, place.data(), n, &ma.mix, rows, n_rows, cap, nullptr);
		else if (cs == "null_r")
			rc = lw_rows_synth_mix(nullptr, b, place.data(), n, &ma.mix, rows, n_rows, cap, nullptr);
		else if (cs == "n_short")
			rc = lw_rows_synth_mix(r, b, place.data(), n - 1, &ma.mix, rows, n_rows, cap, nullptr);
		else {
			rc = lw_rows_synth_mix(r, bx, place.data(), n, &ma.mix, rows, n_rows, cap, nullptr); // (refuse: what the test made unacceptable)
			if ((rc == LW_OK && (cs == "twice" || cs == "two" || cs == "plain_between")) || (rc == LW_ERR_DEVICE && cs == "fail")) {
				printf("RC %d\n", rc);
				Matrix again;
				if ((cs == "twice" || cs == "fail") && !read_matrix(argv[8], again))
					return 2;
				std::fill(ma.coef.begin(), ma.coef.end(), -123.0f); // the first call has copied its matrix: the caller's is free
				if (cs == "plain_between") {
					rc = lw_rows_synth(r, b, place.data(), n, rows, n_rows, cap, nullptr);
					printf("RC %d\n", rc);
				}
				if (rc == LW_OK || cs == "fail") // (fail: the object takes the next call)
					rc = lw_rows_synth_mix(r, b, place.data(), n, cs == "two" || cs == "plain_between" ? &mb.mix : &again.mix, rows, n_rows, cap, nullptr);
			}
		}
		printf("RC %d\n", rc);
		for (const auto &c : g_coef) { // queued work reads its matrix later: it must still be there after the calls behind it
			printf("A");
			for (uint32_t k = 0; k < c.second; k++) {
				uint32_t bits;
				memcpy(&bits, c.first + k, 4);
				printf(" %u", bits);
			}
			printf("\n");
		}
		printf("LAUNCHES %d %d %d\n", g_mix_launches, g_rows_launches, armed && lw_standin_fail_launch.load() != 1 ? 1 : 0);
		printf("N %zu %llu\n", lw_rows_last_segments(r), (unsigned long long)lw_rows_last_copied_elems(r));
		lw_standin_fail_launch.store(0);
		lw_rows_destroy(r);
		if (bx != b)
			lw_batch_destroy(bx);
	}
	lw_pwr_free(pw);
	lw_batch_destroy(b);
	lw_decoder_destroy(d);
	lw_setup_free(setup);
	lw_ident_free(id);
	return 0;
}
