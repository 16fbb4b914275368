// The shared lane-level helpers WITHOUT a GPU: lewton_amd/csrc/lw_lanes.hpp compiled for the host (LW_KERNEL_HOST) and held against
// the plainest restatement of what each helper promises, at the places it can go wrong.  Every buffer is of its exact size, so a
// read or a store beyond it is AddressSanitizer's to report.  Built with -fsanitize=address,undefined; tests/test_host_lanes.py
// drives it.  No HIP code, no GPU.
//   lanes_host bits     count / first / last over every [lo, hi) of three 192-bit lists, both index types, both inv   "OK bits n"
//   lanes_host levels   lists of 1 .. 4097 doubles folded level by level, against the contract's recurrence            "OK levels n"
//   lanes_host mask     the mask writer over spans whose start and end sit 0 .. 3 bytes behind a 4-byte boundary        "OK mask n"
//   lanes_host runs     lw_run_plan and lw_run_group: every element of every line in exactly one group                  "OK runs n"
#define KERNEL_HOST_NO_HIP_OK 1
#define LW_KERNEL_HOST 1
#include "../../lewton_amd/csrc/lw_lanes.hpp"

#include "kernel_host.hpp"

#include <string>

template <class T>
static T *exact(size_t n) // n elements and not one more
{
	T *p = (T *)malloc(n * sizeof(T));
	if (!p)
		exit(2);
	return p;
}

static uint64_t bits_of(double d)
{
	uint64_t u;
	memcpy(&u, &d, 8);
	return u;
}

// ---- bit lists
static bool bit(const uint64_t *b, int j)
{
	return (b[j / 64] >> (j % 64)) & 1u;
}

template <class I>
static long bits_one(const uint64_t *b, const char *name)
{
	long n = 0;
	for (int inv = 0; inv < 2; inv++)
		for (int lo = 0; lo < 192; lo++)
			for (int hi = lo + 1; hi <= 192; hi++) {
				int count = 0, first = -1, last = -1;
				for (int j = lo; j < hi; j++)
					if (bit(b, j) != (inv != 0)) {
						count++, last = j;
						if (first < 0)
							first = j;
					}
				const uint64_t v = inv ? ~(uint64_t)0 : 0u;
				const int c = (int)lw_bits_count<I>(b, (I)lo, (I)hi, v), f = lw_bits_first<I>(b, (I)lo, (I)hi, v), l = lw_bits_last<I>(b, (I)lo, (I)hi, v);
				if (c != count || f != first || l != last)
					bad("bits %s inv %d [%d, %d): count %d first %d last %d, a loop over single bits has %d %d %d", name, inv, lo, hi, c, f, l, count,
							first, last);
				n++;
			}
	return n;
}

static long bits_all()
{
	long n = 0;
	uint64_t x = 0x9e3779b97f4a7c15ull;
	for (int list = 0; list < 3; list++) {
		uint64_t *b = exact<uint64_t>(3); // (word 3 does not exist)
		for (int w = 0; w < 3; w++) {
			x ^= x << 13, x ^= x >> 7, x ^= x << 17;
			b[w] = list == 0 ? x : list == 1 ? ~(uint64_t)0 : 0u;
		}
		n += bits_one<uint32_t>(b, "uint32_t") + bits_one<int32_t>(b, "int32_t");
		if (lw_bits_first<int32_t>(b, 7, 7, 0u) != -1 || lw_bits_last<int32_t>(b, 9, 7, 0u) != -1)
			bad("bits: an empty range has a member");
		for (int j = 0; j < 192; j++)
			if (lw_bits_bit(b, j) != bit(b, j))
				bad("bits: bit %d", j);
		free(b);
	}
	return n;
}

// ---- levels
static double recurrence(const std::vector<double> &list) // the contract: 64 entries at a time, t[j] = t[2j] + t[2j + 1], padded with +0.0
{
	std::vector<double> cur = list;
	while (cur.size() > 1) {
		std::vector<double> pad = cur, next;
		pad.resize((cur.size() + 63) / 64 * 64, 0.0);
		for (size_t g = 0; g < pad.size(); g += 64) {
			double t[64];
			for (int j = 0; j < 64; j++)
				t[j] = pad[g + j];
			for (int n = 32; n; n >>= 1)
				for (int j = 0; j < n; j++)
					t[j] = t[2 * j] + t[2 * j + 1];
			next.push_back(t[0]);
		}
		cur = next;
	}
	return cur[0];
}

static long levels_all()
{
	const size_t lens[] = {1, 2, 64, 65, 4096, 4097};
	long n = 0;
	for (size_t len : lens) {
		std::vector<double> list(len);
		double plain = 0.0;
		for (size_t i = 0; i < len; i++) {
			list[i] = i % 4 == 0 ? 1e16 : i % 4 == 1 ? 1.0 + (double)(i % 7) : i % 4 == 2 ? -1e16 : 3.0;
			plain += list[i];
		}
		const double want = recurrence(list);
		if (len > 2 && bits_of(plain) == bits_of(want))
			bad("levels %zu: a left-to-right sum has the tree's bits, the case shows nothing", len);
		LwSumPlan p;
		if (!lw_sum_plan((uint64_t)len * LW_SUM_CHUNK, 1u, 1u, 2048u, p) || p.chunks != len || p.longest != len ||
				p.fold_scratch != (len + 63) / 64 + (len + 4095) / 4096)
			bad("levels %zu: the plan", len);
		double *in = exact<double>(len), *scratch = exact<double>((size_t)p.fold_scratch);
		memcpy(in, list.data(), len * 8);
		LwLevels<double> v;
		lw_levels(v, (const double *)in, (uint64_t)len, scratch, p.longest);
		while (v.len > 1) {
			for (uint32_t wave = 0; wave < LW_LANES_WAVES; wave++)
				lw_level_wave(v, wave, 0u);
			lw_level_next(v);
		}
		if (v.len != 1 || bits_of(v.in[0]) != bits_of(want))
			bad("levels %zu: %a, the recurrence has %a", len, v.in[0], want);
		// ... and ONE tree of a list of at most 64, as the fused forms fold it
		if (len <= 64) {
			const double one = lw_wave_tree<double>(0u, [&](uint32_t l) { return l < len ? in[l] : 0.0; });
			if (len > 1 && bits_of(one) != bits_of(want))
				bad("levels %zu: one tree", len);
		}
		free(in), free(scratch);
		n++;
	}
	return n;
}

// ---- the mask writer
static long mask_all()
{
	const unsigned char SENT = 0xa5;
	const uint64_t starts[] = {0, 1021}, lens[] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 1023, 1024, 1025, 1026, 1027};
	long n = 0;
	for (unsigned off = 0; off < 4; off++)
		for (uint64_t t0 : starts)
			for (uint64_t len : lens)
				for (int which = 0; which < 3; which++) {
					const uint64_t end = t0 + len, frames = which == 0 ? 0u : which == 1 ? t0 + len / 2 : end; // n == 0, n < fill_end, n == fill_end
					const Guarded g = shifted((size_t)end, off);
					uint8_t *m = g.as<uint8_t>();
					memset(m, SENT, (size_t)end);
					std::vector<int> asked((size_t)end + 8, 0);
					const auto value = [&](uint64_t f) { return f < frames ? (uint32_t)((f * 7u + 3u) >> 1 & 1u) : 0u; };
					for (uint32_t tid = 0; tid < LW_LANES_WAVES * 64u; tid++)
						lw_mask_write(m, t0, end, tid, [&](uint64_t f) {
							if (f >= end)
								bad("mask: byte %llu of a span that ends at %llu", (unsigned long long)f, (unsigned long long)end);
							asked[(size_t)f]++;
							return value(f);
						});
					for (uint64_t f = 0; f < end; f++) {
						const bool in = f >= t0;
						if (asked[(size_t)f] != (in ? 1 : 0) || m[f] != (in ? value(f) : SENT))
							bad("mask off %u t0 %llu len %llu n %llu: byte %llu is %u, written %d times", off, (unsigned long long)t0,
									(unsigned long long)len, (unsigned long long)frames, (unsigned long long)f, m[f], asked[(size_t)f]);
					}
					if (!guard_intact(g))
						bad("mask: a store in front of the line");
					free(g.base);
					n++;
				}
	return n;
}

// ---- runs of four: the plan and the groups
static long runs_all()
{
	const uint64_t spans[] = {0, 1, 3, 4, 255, 256, 257, 1021, 4099};
	long n = 0;
	for (uint32_t F = 1; F <= 3; F += 2)
		for (uint64_t span : spans)
			for (unsigned off_d = 0; off_d < 16; off_d += 4)
				for (unsigned off_s = 0; off_s < 8; off_s += 4) {
					LwRunPlan p;
					if (!lw_run_plan(2u, F, span, 8u, p) || p.runs_per_line < 1 || p.runs != F * p.runs_per_line || !p.per_wave ||
							(uint64_t)p.tiles * p.per_wave * LW_LANES_WAVES < p.runs || (uint64_t)(p.tiles - 1) * p.per_wave * LW_LANES_WAVES >= p.runs)
						bad("runs F %u span %llu: the plan", F, (unsigned long long)span);
					const uint64_t line_el = span + 1, ch_at = 5;
					const float *dst = (const float *)(uintptr_t)(0x10000u + off_d), *src = (const float *)(uintptr_t)(0x20000u + off_s); // (never dereferenced)
					std::vector<int> seen((size_t)(F * line_el), 0);
					for (uint32_t bx = 0; bx < p.tiles; bx++)
						for (uint32_t tid = 0; tid < LW_LANES_WAVES * 64u; tid++)
							for (uint32_t i = 0; i < p.per_wave; i++) {
								const uint64_t run = (uint64_t)bx * (LW_LANES_WAVES * (uint64_t)p.per_wave) + (uint64_t)i * LW_LANES_WAVES + (tid >> 6);
								if (run >= p.runs)
									continue;
								const LwRunGroup g = lw_run_group(p.runs_per_line, src, dst, ch_at, line_el, (uint32_t)run, tid & 63u);
								if (g.line >= F || g.at != ch_at + g.line * line_el || (((uintptr_t)dst + 4u * (uint64_t)((int64_t)g.at + g.t0)) & 15u) ||
										g.same != ((((uintptr_t)src >> 2) + g.at) % 4u == (((uintptr_t)dst >> 2) + g.at) % 4u))
									bad("runs F %u span %llu: the group of run %llu, lane %u", F, (unsigned long long)span, (unsigned long long)run, tid & 63u);
								for (int j = 0; j < 4; j++)
									if (g.t0 + j >= 0 && (uint64_t)(g.t0 + j) < span)
										seen[(size_t)(g.line * line_el + (uint64_t)(g.t0 + j))]++;
							}
					for (uint32_t line = 0; line < F; line++)
						for (uint64_t e = 0; e < line_el; e++)
							if (seen[(size_t)(line * line_el + e)] != (e < span ? 1 : 0))
								bad("runs F %u span %llu: element %llu of line %u lies in %d groups", F, (unsigned long long)span, (unsigned long long)e, line,
										seen[(size_t)(line * line_el + e)]);
					n++;
				}
	return n;
}

int main(int argc, char **argv)
{
	if (argc < 2)
		return 2;
	const std::string mode = argv[1];
	if (mode == "bits")
		printf("OK bits %ld\n", bits_all());
	else if (mode == "levels")
		printf("OK levels %ld\n", levels_all());
	else if (mode == "mask")
		printf("OK mask %ld\n", mask_all());
	else if (mode == "runs")
		printf("OK runs %ld\n", runs_all());
	else
		return 2;
	return 0;
}
