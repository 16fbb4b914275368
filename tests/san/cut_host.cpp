// Cutting rows into segment rows WITHOUT a GPU: lw_cut.cpp linked against hip_standins.inc (device memory = calloc), and the KERNEL
// source itself, lw_kernels_cut.hip, compiled for the host (LW_CUT_HOST): the stand-in for the launcher below runs it workgroup by
// workgroup over exact-size buffers, so AddressSanitizer sees every load and store the kernel makes.  In "run" the whole source is
// poisoned and only the elements [start, end) of the jobs' lines are opened again (to ASan's granule of 8 bytes), so a load outside a
// job's part of a line is a report as well.  Built with -fsanitize=address,undefined; tests/test_host_cut.py drives it.
//   cut_host refuse CASE               "RC rc", "LAUNCHES n", "LAST n", "OUT u": whether the destination still holds its fill;
//                                      CASE is one of the calls of main below
//   cut_host two                       two calls queued back to back: "ROWS at/len/fill_end..." per launch, read at the end
//   cut_host run ELEM CH F ROWS CAP NOUT OUTCAP FILL OFF_SRC OFF_DST IN OUT
//                                      IN: u64 n[ROWS], u64 jobs[NOUT][3], u64 fill_to[NOUT], the source [ROWS][CH][F][CAP] of ELEM
//                                      bytes an element; OUT: the destination [NOUT][CH][F][OUTCAP], sentinel-filled before the
//                                      call.  FILL: 0 = the array is NULL.  The buffers are exact-size, start OFF_* BYTES (a
//                                      multiple of ELEM) behind a 16-byte boundary and have a guarded front.  "RC rc", "LAUNCHES n"
//   cut_host far ELEM BASE KEEP START END OUTCAP IN OUT
//                                      ONE row, channel and line of BASE + KEEP elements of which only [BASE, BASE + KEEP) exist
//                                      (BASE past 2^32): IN holds them; the source pointer is moved BASE elements in front of
//                                      the data; one job (0, BASE + START, BASE + END).  OUT: the destination [OUTCAP]
#include "../../include/lewton_amd.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "hip_standins.inc"
#include "kernel_host.hpp"

#define LW_CUT_HOST 1
#include "../../lewton_amd/csrc/lw_kernels_cut.hip"

static LaunchLog<LwCutJob> g_log;

hipError_t lw_launch_cut(const LwCutArgs &a, uint32_t n_jobs, hipStream_t)
{
	g_log.launch(a.jobs + a.job0, n_jobs);
	if (!a.jobs || n_jobs == 0 || n_jobs > 65535u || a.ch == 0 || a.F == 0 || !a.dst || (a.elem != 2u && a.elem != 4u) || a.tiles == 0 ||
			(uint64_t)a.tiles * a.F > LW_CT_MAX_TILES)
		bad("arguments");
	if (!g_log.run)
		return hipSuccess;
	for (uint32_t bz = 0; bz < n_jobs; bz++)
		for (uint32_t by = 0; by < a.ch; by++)
			for (uint32_t bx = 0; bx < a.tiles * a.F; bx++)
				for (uint32_t tid = 0; tid < LW_CT_THREADS; tid++)
					lw_ct_workgroup_lane(a, bx, by, bz, tid);
	return hipSuccess;
}

int main(int argc, char **argv)
{
	if (argc < 2)
		return 2;
	const std::string mode = argv[1];
	int err = 0;
	if (mode == "run" && argc >= 14) {
		const uint32_t elem = (uint32_t)atoi(argv[2]), ch = (uint32_t)atoi(argv[3]), F = (uint32_t)atoi(argv[4]);
		const size_t rows = (size_t)atoll(argv[5]), cap = (size_t)atoll(argv[6]), n_out = (size_t)atoll(argv[7]), outcap = (size_t)atoll(argv[8]);
		const bool fill = atoi(argv[9]) != 0;
		const size_t nb = rows * ch * F * cap * elem, ob = n_out * ch * F * outcap * elem;
		std::vector<uint64_t> n(rows + 1), jobs(3 * n_out + 1), fill_to(n_out + 1);
		const Guarded gs = shifted(nb, (unsigned)atoi(argv[10])), gd = shifted(ob, (unsigned)atoi(argv[11]));
		{
			File in(argv[12], "rb");
			in.get(n.data(), rows), in.get(jobs.data(), 3 * n_out), in.get(fill_to.data(), n_out), in.get(gs.at, nb);
		}
		if (elem == 4)
			fill32(gd.at, ob / 4, SENT_DEAD);
		else
			fill16(gd.at, ob / 2, 0x7eadu);
		// only the jobs' parts of their lines may be read (checked here too: the call refuses what does not fit)
		ASAN_POISON_MEMORY_REGION(gs.at, nb);
		for (size_t i = 0; i < n_out; i++)
			for (size_t line = 0; line < (size_t)ch * F && jobs[3 * i] < rows && jobs[3 * i + 1] <= jobs[3 * i + 2] && jobs[3 * i + 2] <= cap; line++)
				ASAN_UNPOISON_MEMORY_REGION(gs.at + ((jobs[3 * i] * ch * F + line) * cap + jobs[3 * i + 1]) * elem, (jobs[3 * i + 2] - jobs[3 * i + 1]) * elem);
		lw_cut *c = lw_cut_create(0, &err);
		if (!c || lw_cut_last_launches(c) != -1)
			return 2;
		const int rc = lw_cut_rows(c, ch, F, elem, gs.at, rows, cap, n.data(), jobs.data(), n_out, gd.at, outcap, fill ? fill_to.data() : nullptr, nullptr);
		printf("RC %d\nLAUNCHES %d\n", rc, g_log.launches);
		if (rc == LW_OK && lw_cut_last_launches(c) != g_log.launches)
			return 3;
		{
			File out(argv[13], "wb");
			out.put(gd.at, ob);
		}
		ASAN_UNPOISON_MEMORY_REGION(gs.at, nb);
		if (!guard_intact(gs) || !guard_intact(gd))
			bad("a store in front of a buffer");
		free(gs.base), free(gd.base);
		lw_cut_destroy(c);
		return 0;
	}
	if (mode == "far" && argc >= 10) {
		const uint32_t elem = (uint32_t)atoi(argv[2]);
		const uint64_t base = strtoull(argv[3], nullptr, 10), keep = strtoull(argv[4], nullptr, 10), T = base + keep;
		const uint64_t job[3] = {0, base + strtoull(argv[5], nullptr, 10), base + strtoull(argv[6], nullptr, 10)};
		const size_t outcap = (size_t)atoll(argv[7]);
		std::vector<uint8_t> x((size_t)keep * elem), y(outcap * elem, 0x7e);
		{
			File in(argv[8], "rb");
			in.get(x.data(), x.size());
		}
		lw_cut *c = lw_cut_create(0, &err);
		if (!c)
			return 2;
		const uintptr_t s = (uintptr_t)x.data() - (uintptr_t)base * elem;
		const int rc = lw_cut_rows(c, 1, 1, elem, (const void *)s, 1, (size_t)T, &T, job, 1, y.data(), outcap, nullptr, nullptr);
		printf("RC %d\nLAUNCHES %d\n", rc, g_log.launches);
		{
			File out(argv[9], "wb");
			out.put(y.data(), y.size());
		}
		lw_cut_destroy(c);
		return 0;
	}
	// ---- calls on a small fixture: 2 rows of 2 channels and 3 lines of 100 floats, 3 jobs into rows of 64
	std::vector<float> src(2 * 2 * 3 * 100, 0.25f), dst(3 * 2 * 3 * 64, 77.0f);
	uint64_t cnt[2] = {100, 40}, jobs[9] = {0, 10, 50, 1, 0, 40, 0, 90, 100}, fill[3] = {64, 0, 11};
	g_log.run = false;
	if (mode == "two") {
		lw_cut *c = lw_cut_create(0, &err);
		if (!c)
			return 2;
		uint64_t jobs_b[3] = {1, 5, 6};
		int rc = lw_cut_rows(c, 2, 3, 4, src.data(), 2, 100, cnt, jobs, 3, dst.data(), 64, fill, nullptr);
		printf("RC %d LAST %d\n", rc, lw_cut_last_launches(c));
		jobs[0] = 1, fill[1] = 7, cnt[0] = 1; // the first call has copied its arrays: the caller's are free
		rc = lw_cut_rows(c, 2, 3, 4, src.data(), 2, 100, cnt, jobs_b, 1, dst.data(), 64, nullptr, nullptr);
		printf("RC %d LAST %d\n", rc, lw_cut_last_launches(c));
		g_log.print([](const LwCutJob &j) { printf(" %llu/%llu/%llu", (unsigned long long)j.src_at, (unsigned long long)j.len, (unsigned long long)j.fill_end); });
		lw_cut_destroy(c);
		return 0;
	}
	if (mode != "refuse" || argc < 3)
		return 2;
	const std::string cs = argv[2];
	uint32_t ch = 2, F = 3, elem = 4;
	const void *s = src.data();
	void *d = dst.data();
	const uint64_t *n = cnt, *jb = jobs, *fl = fill;
	size_t rows = 2, cap = 100, n_out = 3, outcap = 64;
	bool null_c = false;
	std::vector<uint64_t> many;
	if (cs == "null_c")
		null_c = true;
	else if (cs == "null_n")
		n = nullptr;
	else if (cs == "null_jobs")
		jb = nullptr;
	else if (cs == "null_src")
		s = nullptr;
	else if (cs == "null_dst")
		d = nullptr;
	else if (cs == "null_dst_fill_only")
		jobs[1] = jobs[2] = 0, jobs[5] = 0, jobs[7] = 100, s = nullptr, d = nullptr; // nothing to read, but jobs 0 and 2 are filled
	else if (cs == "elem3")
		elem = 3;
	else if (cs == "elem8")
		elem = 8;
	else if (cs == "elem1")
		elem = 1;
	else if (cs == "row_over")
		jobs[6] = 2; // (the LAST job: every job is checked before anything is queued)
	else if (cs == "start_after_end")
		jobs[7] = 100, jobs[8] = 99;
	else if (cs == "end_over")
		jobs[5] = 41; // beyond the row's length, inside its capacity
	else if (cs == "len_over")
		jobs[7] = 35; // 65 elements into rows of 64
	else if (cs == "fill_over")
		fill[2] = 65;
	else if (cs == "n_over")
		cnt[0] = 101;
	else if (cs == "ch0")
		ch = 0;
	else if (cs == "ch256")
		ch = 256;
	else if (cs == "f0")
		F = 0;
	else if (cs == "f65536")
		F = 65536;
	else if (cs == "too_large")
		cap = (size_t)1 << 62;
	else if (cs == "too_large_out")
		outcap = (size_t)1 << 62;
	else if (cs == "too_many_tiles") // 257 tiles of 16384 bytes in each of 65535 lines, more than a grid counts
		F = 65535, outcap = (size_t)1 << 21, fill[0] = 256 * 4096 + 1;
	else if (cs == "ok_most_tiles")
		F = 65535, outcap = (size_t)1 << 21, fill[0] = 256 * 4096; // (nothing runs here: the buffers are only looked at)
	else if (cs == "ok_i16")
		elem = 2;
	else if (cs == "ok_no_jobs")
		n_out = 0, jb = nullptr, fl = nullptr;
	else if (cs == "ok_no_rows_no_jobs")
		rows = 0, n = nullptr, n_out = 0, jb = nullptr, fl = nullptr;
	else if (cs == "ok_empty_jobs")
		jobs[1] = jobs[2] = 7, jobs[5] = 0, jobs[7] = 100, fl = nullptr, s = nullptr, d = nullptr; // nothing to write: no launch
	else if (cs == "ok_fill_only")
		jobs[1] = jobs[2] = 0, jobs[5] = 0, jobs[7] = 100, s = nullptr;
	else if (cs == "ok_jobs65536") { // two launches
		n_out = 65536, many.assign(3 * n_out, 0), jb = many.data(), fl = nullptr, ch = 1, F = 1, outcap = 1;
		many[3 * 65535 + 2] = 1;
		dst.assign(n_out, 77.0f), d = dst.data();
	} else if (cs != "ok")
		return 2;
	lw_cut *c = lw_cut_create(0, &err);
	if (!c)
		return 2;
	if (lw_cut_last_launches(nullptr) != -1 || lw_cut_create(1, &err) != nullptr || err != LW_ERR_DEVICE)
		return 3;
	const int rc = lw_cut_rows(null_c ? nullptr : c, ch, F, elem, s, rows, cap, n, jb, n_out, d, outcap, fl, nullptr);
	printf("RC %d\nLAUNCHES %d\nLAST %d\n", rc, g_log.launches, lw_cut_last_launches(c));
	bool untouched = true;
	for (float v : dst)
		untouched = untouched && v == 77.0f;
	printf("OUT %d\n", (int)untouched);
	lw_cut_destroy(c);
	lw_cut_destroy(nullptr);
	return 0;
}
