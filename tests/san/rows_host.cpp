// lw_rows_synth WITHOUT a GPU: the product sources + lw_rows.cpp linked against hip_standins.inc (sample values are zero,
// everything the host decides is real), like fmt_host.cpp.  The stand-in for lw_launch_rows below prints the piece list it was
// given and checks every piece against the sizes of the source and the destination; tests/test_host_rows.py recomputes the
// expected element mapping from the printed lw_batch_results and the places it chose.
//   usage: rows_host packets.bin FMT results
//          rows_host packets.bin FMT synth places.txt N_ROWS ROW_CAPACITY [CASE]
//   packets.bin: [u32 length][bytes] of the three header packets, then of the audio packets of one stream (one batch, one
//   PreviousWindowRight: the first packet yields no samples)
//   places.txt: one line "row skip keep t0" per audio packet
//   CASE: ok (default) | twice | fail (the k_rows launch of the first of two calls fails) | refuse | null_rows | null_place | null_batch | null_r | other_fmt | other_decoder | n_short | small_max
//   output: "R status n_samples out_offset" per packet, "S src count dst" per piece of each k_rows launch, "RC rc",
//   "LAUNCHES k_rows synth" (synth: 1 when a synthesis launcher ran), "N segments copied_elems"
#include "../../include/lewton_amd.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "hip_standins.inc"
#define KERNEL_HOST_NO_HIP_OK 1 // (lw_runtime.cpp is linked)
#include "kernel_host.hpp"

static uint64_t g_src_elems = 0, g_dst_elems = 0;
static int g_rows_launches = 0;
static bool g_fail_rows_launch = false; // the next k_rows launch fails, once

hipError_t lw_launch_rows(const void *d_src, void *d_dst, const LwRowSeg *d_segs, uint32_t n_segs, int elem_size, hipStream_t)
{
	g_rows_launches++;
	if (g_fail_rows_launch) {
		g_fail_rows_launch = false;
		return hipErrorLaunchFailure;
	}
	if (!d_src || !d_dst || (elem_size != 2 && elem_size != 4))
		bad("arguments");
	for (uint32_t i = 0; i < n_segs; i++) {
		const LwRowSeg &s = d_segs[i]; // (device memory = calloc here, filled by the hipMemcpyAsync stand-in)
		printf("S %u %u %llu\n", s.src_elem, s.count, (unsigned long long)s.dst_elem);
		if (s.count == 0 || (uint64_t)s.src_elem + s.count > g_src_elems || s.dst_elem + s.count > g_dst_elems || s.dst_elem + s.count < s.dst_elem)
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
	const size_t n = pk.size() - 3, ch = info.audio_channels;
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
	if (mode == "synth" && argc >= 7) {
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
		const std::string cs = argc > 7 ? argv[7] : "ok";
		lw_rows *r = lw_rows_create(d, cs == "small_max" ? n - 1 : n, fmt, &err);
		if (!r)
			return 2;
		g_src_elems = lw_batch_out_elems(b);
		g_dst_elems = (uint64_t)n_rows * ch * cap;
		void *rows = (void *)(uintptr_t)0x1000; // never dereferenced: the stand-ins launch nothing
		lw_batch *bx = b;
		lw_decoder *d2 = nullptr;
		if (cs == "other_fmt")
			bx = lw_batch_create(d, n, fmt ^ 1, &err);
		if (cs == "other_decoder") {
			d2 = lw_decoder_create(id, setup, 0, &err);
			bx = lw_batch_create(d2, n, fmt, &err);
		}
		if (bx != b) {
			lw_pwr *p2 = lw_pwr_new(d2 ? d2 : d);
			for (size_t i = 0; i < n; i++)
				in[i].pwr = p2;
			if (lw_batch_entropy(bx, in.data(), n, 2) != LW_OK || lw_batch_upload(bx, nullptr) != LW_OK)
				return 2;
			lw_pwr_free(p2);
		}
		// every CASE but ok / twice is expected to be refused: armed, the first synthesis launcher that runs takes this to 0
		const bool armed = cs != "ok" && cs != "twice" && cs != "fail";
		g_fail_rows_launch = cs == "fail";
		lw_standin_fail_launch.store(armed ? 1 : 0);
		int rc;
		if (cs == "null_rows")
			rc = lw_rows_synth(r, b, place.data(), n, nullptr, n_rows, cap, nullptr);
		else if (cs == "null_place")
			rc = lw_rows_synth(r, b, nullptr, n, rows, n_rows, cap, nullptr);
		else if (cs == "null_batch")
			rc = lw_rows_synth(r, nullptr, place.data(), n, rows, n_rows, cap, nullptr);
		else if (cs == "null_r")
			rc = lw_rows_synth(nullptr, b, place.data(), n, rows, n_rows, cap, nullptr);
		else if (cs == "n_short")
			rc = lw_rows_synth(r, b, place.data(), n - 1, rows, n_rows, cap, nullptr);
		else {
			rc = lw_rows_synth(r, bx, place.data(), n, rows, n_rows, cap, nullptr); // (refuse: places the test made unacceptable)
			if ((rc == LW_OK && cs == "twice") || (rc == LW_ERR_DEVICE && cs == "fail")) { // (fail: the object takes the next call)
				printf("RC %d\n", rc);
				rc = lw_rows_synth(r, bx, place.data(), n, rows, n_rows, cap, nullptr);
			}
		}
		printf("RC %d\n", rc);
		printf("LAUNCHES %d %d\n", g_rows_launches, armed && lw_standin_fail_launch.load() != 1 ? 1 : 0);
		printf("N %zu %llu\n", lw_rows_last_segments(r), (unsigned long long)lw_rows_last_copied_elems(r));
		lw_standin_fail_launch.store(0);
		lw_rows_destroy(r);
		if (bx != b)
			lw_batch_destroy(bx);
		if (d2)
			lw_decoder_destroy(d2);
	}
	lw_pwr_free(pw);
	lw_batch_destroy(b);
	lw_decoder_destroy(d);
	lw_setup_free(setup);
	lw_ident_free(id);
	return 0;
}
