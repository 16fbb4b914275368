// The lane-level building blocks of the rows kernels (lw_kernels_<op>.hip and their lw_<op>.hpp): the host/device switch, the
// ordered double sum of include/lewton_amd.h ("normalising rows") -- its tree, its levels and its plan --, lists of ballot words,
// the writer of a byte mask, and the plan and the groups of the runs of four floats.  Device and host in one: a program of
// tests/san/ defines LW_KERNEL_HOST before it includes a kernel source and runs it a wave (lane is 0) or a lane at a time.
// Nothing here knows an operator's argument struct; a workgroup is LW_LANES_WAVES waves of 64 lanes.  The ORDER of lw_wave_tree
// and of the levels below IS the order of "normalising rows": an operator that sums takes it from here.
// What a caller keeps in a struct of its own and the loops read again and again (n, t0) arrives by reference: the compiler then
// reads it where the kernels always did and emits the code it emitted when each kernel file had these loops to itself.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

// ---- the switch.  LW_KERNEL_HOST, or the name a kernel file's own programs of tests/san/ have always given it.  LW_LANES_FN: a
// function of a kernel source; LW_LANES_RESTRICT: on its pointer parameters; LW_LANES_HD: a rule of an lw_<op>.hpp that the host
// side and the kernels share
#if defined(LW_CEP_HOST) || defined(LW_CUT_HOST) || defined(LW_FEAT_HOST) || defined(LW_ISTFT_HOST) || defined(LW_NORM_HOST) || defined(LW_PACK_HOST) || \
	defined(LW_RESAMPLE_HOST) || defined(LW_SEGMENT_HOST) || defined(LW_SELECT_HOST) || defined(LW_SLIDE_HOST) || defined(LW_SPEC_HOST) || defined(LW_VAD_HOST)
#define LW_KERNEL_HOST 1
#endif
#ifdef LW_KERNEL_HOST
#define LW_LANES_FN static inline
#define LW_LANES_RESTRICT
#else
#define LW_LANES_FN __device__ __forceinline__
#define LW_LANES_RESTRICT __restrict__
#endif
#if defined(__HIPCC__) || defined(__HIP__)
#define LW_LANES_HD __host__ __device__ static inline
#else
#define LW_LANES_HD static inline
#endif

// C/D layout of the 32x32 matrix instructions: register r of lane l holds row (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31
#define LW_MFMA32_ROW(r, lane) (((r) & 3u) + 8u * ((r) >> 2) + 4u * ((lane) >> 5))

#define LW_LANES_WAVES 4u // waves of a workgroup: the plans and the round-robin loops below count on it
#define LW_SUM_CHUNK 256u // elements per chunk of a sum
#define LW_SUM_GROUP 64u  // list entries one tree folds
#define LW_RUN_EL 256u    // elements per run: 64 groups of four

// ---- plans, for the host side.  The sum: the chunk slots of a row are numbered line-major over the call's largest chunk count,
// slot = line * chunks + chunk; a wave takes per_wave consecutive slots, a workgroup four waves' worth, `aim` workgroups per row
// where that is enough.  Which slot a wave takes decides nothing about the bits.  fold_scratch: what a workgroup that folds a list
// of list_lines * chunks entries level by level keeps of its own, ceil(longest / 64) + ceil(longest / 4096) entries.
// false: chunks or slots that 32 bits cannot count
struct LwSumPlan {
	uint32_t chunks, per_wave, tiles;
	uint64_t longest, fold_scratch;
};

static inline bool lw_sum_plan(uint64_t most, uint64_t lines, uint64_t list_lines, uint32_t aim, LwSumPlan &p)
{
	const uint64_t chunks = (most + LW_SUM_CHUNK - 1u) / LW_SUM_CHUNK, slots = lines * chunks;
	if (chunks > UINT32_MAX || slots > UINT32_MAX)
		return false;
	const uint64_t units = (slots + LW_LANES_WAVES - 1u) / LW_LANES_WAVES;
	p.chunks = (uint32_t)chunks;
	p.per_wave = (uint32_t)((units + aim - 1u) / aim);
	p.tiles = p.per_wave ? (uint32_t)((units + p.per_wave - 1u) / p.per_wave) : 0u;
	p.longest = list_lines * chunks;
	p.fold_scratch = (p.longest + 63u) / 64u + (p.longest + 4095u) / 4096u;
	return true;
}

// Runs of four.  A RUN is 64 groups of four consecutive elements of one line, a group aligned to 16 bytes in the destination (so a
// line whose address is not a multiple of 16 has a partial group at its head and one at its tail: the scalar head and tail); lane
// i of a wave takes group i of a run.  A channel's runs are numbered line-major, run = line * runs_per_line + index.  A workgroup
// is a TILE: 4 * per_wave consecutive runs of one (row, channel), wave w taking runs w, w + 4, ... of them; the plan aims at
// max_tiles tiles per row (a channel has at least one).  false: more runs in a channel than 32 bits count
struct LwRunPlan {
	uint32_t runs_per_line; // ceil((span + 3) / 256), span = the call's largest fill_end; at least 1
	uint32_t runs;          // per channel: F * runs_per_line
	uint32_t per_wave;      // runs a wave takes
	uint32_t tiles;         // per channel: ceil(runs / (4 * per_wave))
};

static inline bool lw_run_plan(uint32_t ch, uint32_t F, uint64_t span, uint32_t max_tiles, LwRunPlan &p)
{
	const uint64_t rpl = (span + 3u + LW_RUN_EL - 1u) / LW_RUN_EL, runs = rpl * F;
	if (runs > UINT32_MAX)
		return false;
	const uint32_t aim = max_tiles / ch ? max_tiles / ch : 1u;                   // tiles per channel
	const uint64_t units = (runs + LW_LANES_WAVES - 1u) / LW_LANES_WAVES; // a unit: one run for each wave
	p.runs_per_line = (uint32_t)rpl, p.runs = (uint32_t)runs;
	p.per_wave = (uint32_t)((units + aim - 1u) / aim);
	p.tiles = (uint32_t)((units + p.per_wave - 1u) / p.per_wave);
	return true;
}

// ---- what follows is for kernel sources alone
#if defined(LW_KERNEL_HOST) || defined(__HIPCC__) || defined(__HIP__)

struct alignas(16) LwF4 {
	float v[4];
};
typedef float LwV4 __attribute__((vector_size(16)));

// ---- the tree.  On the device every lane brings its entry and leaves with the wave's: the xor butterfly 1, 2, .. 32, the
// adjacent-pair tree, the same bits in every lane since the additions commute.  The host build runs a wave at a time (lane is 0)
// and folds the 64 entries as the contract writes it, t[j] = t[2j] + t[2j + 1].  A type other than double brings its own
// lw_wave_add and (device) lw_wave_xor
LW_LANES_FN double lw_wave_add(double a, double b)
{
	return a + b;
}
#ifndef LW_KERNEL_HOST
LW_LANES_FN double lw_wave_xor(double t, int o)
{
	return __shfl_xor(t, o, 64);
}
#endif

template <class T, class E>
LW_LANES_FN T lw_wave_tree(uint32_t lane, E entry)
{
#ifdef LW_KERNEL_HOST
	T t[LW_SUM_GROUP];
	for (uint32_t l = 0; l < LW_SUM_GROUP; l++)
		t[l] = entry(l);
	for (uint32_t n = LW_SUM_GROUP / 2; n; n >>= 1)
		for (uint32_t j = 0; j < n; j++)
			t[j] = lw_wave_add(t[2 * j], t[2 * j + 1]);
	(void)lane;
	return t[0];
#else
	T t = entry(lane);
#pragma unroll
	for (int o = 1; o < 64; o <<= 1)
		t = lw_wave_add(t, lw_wave_xor(t, o));
	return t;
#endif
}

// ... and the wave's ballot: bit l is lane l's decision
template <class P>
LW_LANES_FN uint64_t lw_wave_ballot(uint32_t lane, P decision)
{
#ifdef LW_KERNEL_HOST
	uint64_t w = 0;
	for (uint32_t l = 0; l < 64u; l++)
		w |= (uint64_t)(decision(l) ? 1u : 0u) << l;
	(void)lane;
	return w;
#else
	return __ballot(decision(lane));
#endif
}

// ---- a list folded 64 entries at a time, level by level, by a workgroup.  The lists of the levels: the caller's, then in turn
// the two halves of a scratch of its own, ceil(longest / 64) and ceil(longest / 4096) entries (level 3's list is no longer than
// level 1's, level 4's than level 2's).  while (v.len > 1) { lw_level_wave for every wave; barrier; lw_level_next; }
template <class T>
struct LwLevels {
	const T *in;
	T *out, *other;
	uint64_t len;
};

template <class T>
LW_LANES_FN void lw_levels(LwLevels<T> &v, const T *list, uint64_t len, T *scratch, uint64_t longest)
{
	v.in = list, v.len = len;
	v.out = scratch;
	v.other = scratch + (longest + 63u) / 64u;
}

// one wave's groups of one level: group j of the list, padded with zeros -> entry j of the next
template <class T>
LW_LANES_FN void lw_level_wave(const LwLevels<T> &v, uint32_t wave, uint32_t lane)
{
	const uint64_t groups = (v.len + LW_SUM_GROUP - 1u) / LW_SUM_GROUP;
	for (uint64_t j = wave; j < groups; j += LW_LANES_WAVES) {
		const T t = lw_wave_tree<T>(lane, [&](uint32_t l) {
			const uint64_t e = j * LW_SUM_GROUP + l;
			return e < v.len ? v.in[e] : T{};
		});
		if (lane == 0)
			v.out[j] = t;
	}
}

// ... and behind the level's barrier
template <class T>
LW_LANES_FN void lw_level_next(LwLevels<T> &v)
{
	T *was = v.out;
	v.len = (v.len + LW_SUM_GROUP - 1u) / LW_SUM_GROUP;
	v.in = was, v.out = v.other, v.other = was;
}

// ---- lists of ballot words: bit j is word j >> 6, bit j & 63.  lo and hi are bit numbers, I their type (the caller's own index
// arithmetic: uint32_t or int32_t); inv is ~0 to look for unset bits
LW_LANES_FN bool lw_bits_bit(const uint64_t *b, int32_t j)
{
	return (b[j >> 6] >> (j & 63)) & 1u;
}

// word w of [lo, hi), lo < hi, masked to it
template <class I>
LW_LANES_FN uint64_t lw_bits_word(const uint64_t *b, I w, I lo, I hi, uint64_t inv)
{
	uint64_t m = b[w] ^ inv;
	if (w == lo >> 6)
		m &= ~(uint64_t)0 << (lo & 63);
	if (w == (hi - 1) >> 6 && (hi & 63))
		m &= ((uint64_t)1 << (hi & 63)) - 1u;
	return m;
}

template <class I>
LW_LANES_FN uint32_t lw_bits_count(const uint64_t *b, I lo, I hi, uint64_t inv) // the set bits of [lo, hi), lo < hi
{
	uint32_t c = 0;
	for (I w = lo >> 6; w <= (hi - 1) >> 6; w++)
		c += (uint32_t)__builtin_popcountll(lw_bits_word(b, w, lo, hi, inv));
	return c;
}

template <class I>
LW_LANES_FN int32_t lw_bits_last(const uint64_t *b, I lo, I hi, uint64_t inv) // the largest in [lo, hi), or -1
{
	if (lo >= hi)
		return -1;
	for (int32_t w = (int32_t)((hi - 1) >> 6); w >= (int32_t)(lo >> 6); w--) { // (a signed word number: it runs to -1)
		const uint64_t m = lw_bits_word<I>(b, (I)w, lo, hi, inv);
		if (m)
			return w * 64 + 63 - (int32_t)__builtin_clzll(m);
	}
	return -1;
}

template <class I>
LW_LANES_FN int32_t lw_bits_first(const uint64_t *b, I lo, I hi, uint64_t inv) // the smallest in [lo, hi), or -1
{
	if (lo >= hi)
		return -1;
	for (I w = lo >> 6; w <= (hi - 1) >> 6; w++) {
		const uint64_t m = lw_bits_word(b, w, lo, hi, inv);
		if (m)
			return (int32_t)(w * 64) + (int32_t)__builtin_ctzll(m);
	}
	return -1;
}

// one wave's words of a list of `span` bits in `words` = ceil(span / 64) words, a wave per word, round robin: bit j is frame
// first + j and is decision(j, frame), 0 outside [0, n) of the line
// (n by reference: the caller's struct field, read in the loop where the kernels always read it -- by value the compiler reorders
// k_vad's compares; profiles/rows_lanes_device_diff.txt is the check that it still does as said)
template <class P>
LW_LANES_FN void lw_bits_fill(uint64_t *out, uint32_t span, uint32_t words, int64_t first, const uint64_t &n, uint32_t wave, uint32_t lane, const P &decision)
{
	for (uint32_t w = wave; w < words; w += LW_LANES_WAVES) {
		const uint64_t word = lw_wave_ballot(lane, [&](uint32_t i) {
			const uint32_t j = w * 64u + i;
			const int64_t f = first + (int64_t)j;
			return j < span && f >= 0 && (uint64_t)f < n && decision(j, (uint64_t)f);
		});
		if (lane == 0)
			out[w] = word;
	}
}

// ---- the mask writer: lane tid's groups of four bytes of [t0, end) of the mask line m, byte(f) each -- four at a 4-byte boundary
// of the ADDRESS as one dword, byte by byte where t0 or end cuts a group.  Nothing outside [t0, end) is written
// (t0 by reference, for the same reason as lw_bits_fill's n)
template <class B>
LW_LANES_FN void lw_mask_write(uint8_t *m, const uint64_t &t0, uint64_t end, uint32_t tid, const B &byte)
{
	if (t0 >= end)
		return;
	const uint32_t head = (uint32_t)((uintptr_t)(m + t0) & 3u);
	const uint32_t groups = (uint32_t)((end - t0 + head + 3u) / 4u);
	for (uint32_t g = tid; g < groups; g += LW_LANES_WAVES * 64u) {
		const int64_t f0 = (int64_t)t0 - (int64_t)head + (int64_t)g * 4;
		if (f0 >= (int64_t)t0 && (uint64_t)f0 + 4u <= end) { // all four are the span's: ONE dword
			uint32_t v = 0;
#pragma unroll
			for (uint32_t k = 0; k < 4u; k++)
				v |= byte((uint64_t)f0 + k) << (8u * k);
			*(uint32_t *)(m + f0) = v;
			continue;
		}
		for (int64_t f = f0; f < f0 + 4; f++) // the ragged head and tail of the span
			if (f >= (int64_t)t0 && (uint64_t)f < end)
				m[f] = (uint8_t)byte((uint64_t)f);
	}
}

// ---- runs of four (LwRunPlan above).  The lane's group of run `run` of the channel whose line 0 is at element ch_at: its line,
// the line's element offset, the group's first element (-3 .. at the head of a line that starts off a 16-byte boundary), whether
// the source line sits like the destination line (src may be NULL)
struct LwRunGroup {
	uint32_t line;
	uint64_t at;
	int64_t t0;
	bool same;
};

LW_LANES_FN LwRunGroup lw_run_group(uint32_t runs_per_line, const float *src, const float *dst, uint64_t ch_at, uint64_t line_el, uint32_t run, uint32_t lane)
{
	LwRunGroup g;
	const uint32_t idx = run % runs_per_line;
	g.line = run / runs_per_line;
	g.at = ch_at + (uint64_t)g.line * line_el;
	const uint32_t sd = (uint32_t)(((uintptr_t)dst >> 2) + g.at) & 3u, ss = (uint32_t)(((uintptr_t)src >> 2) + g.at) & 3u;
	g.same = sd == ss;
	g.t0 = (int64_t)(((uint64_t)idx * (LW_RUN_EL / 4u) + lane) * 4u) - (int64_t)sd;
	return g;
}

#endif // kernel sources
