// Energy voice-activity decisions (product code, gfx950): k_vad, k_vad_sum, k_vad_fold, k_vad_decide and k_vad_fill, the kernels
// of lw_vad_rows.  A pass of its own from ONE line of f32 [row][ch][F][frame_capacity] rows (the log energy) to a uint8 mask
// [row][ch][frame_capacity] by the rule of include/lewton_amd.h ("energy voice-activity decisions of feature rows"): Kaldi's
// compute-vad-energy, bit for bit.  The line's sum is DOUBLE and its ORDER is the contract (that of "normalising rows": chunks of
// 256 from frame 0, the adjacent-pair tree, the chunk list folded 64 at a time); the threshold and the window rule are single f32
// operations from lw_vad.hpp.  Two forms that give the same bits:
//   FUSED (every row's span <= 16384 frames = 64 chunks), ONE launch:
//     k_vad         a workgroup of 256 lanes takes one tile of one row and channel.  It recomputes the line's sum itself: its four
//                   waves take the chunks round robin (lane i holds frames 4i .. 4i + 3 of the chunk, adds them in double, the 64
//                   lanes fold by the xor butterfly 1, 2, .. 32 -- the adjacent-pair tree), the chunk sums go into 64 doubles of
//                   LDS, and behind a barrier every wave folds those 64 by the same tree (the same bits in every wave, so no wave
//                   waits for another to broadcast them).  Then thr by lw_vad_threshold_value, then the decide phase below.  The
//                   workgroup of tile 0 stores thr into d_thr.
//   SPLIT (longer rows), THREE launches:
//     k_vad_sum     a wave takes chunks of the energy line and stores each sum into the row's chunk list: ONE plain store.
//     k_vad_fold    a workgroup per row and channel folds the list 64 entries at a time, level by level (the levels' lists in
//                   scratch of its own, __syncthreads() between levels), to S, then thr into scratch and d_thr.
//     k_vad_decide  thr from scratch, then the decide phase.
//   Without a mean (energy_mean_scale == 0) thr is energy_threshold: k_vad_decide alone, whose tile 0 stores d_thr.
//   DECIDE  the raw decisions e[t] > thr of the tile and of frames_context frames either side, frames outside [0, T) as 0, are
//           __ballot words in LDS (a wave per word, round robin); behind a barrier a lane takes four consecutive mask bytes at a
//           4-byte boundary of the mask's ADDRESS: num is the popcount of the masked words of [lo, hi), voiced by
//           lw_vad_voiced_value, the four bytes leave as ONE dword; a group that the tile's start or end cuts goes byte by byte.
// Every byte of [0, fill_end) of a row and channel is written once, nothing else is.  No atomics, no wait of a workgroup on
// another, offsets in 64 bits.  Nothing at or beyond T of the energy line is read, and nothing of any other line.
// tests/san/vad_host.cpp compiles this file for the host (LW_VAD_HOST) and runs it workgroup by workgroup, the phases in the
// kernels' order.
#include "lw_vad.hpp"

#ifdef LW_VAD_HOST
#define LW_VD_FN static inline
#define LW_VD_RESTRICT
#else
#include "lw_kernels.hpp"
#define LW_VD_FN __device__ __forceinline__
#define LW_VD_RESTRICT __restrict__
#endif

typedef float LwVdV4 __attribute__((vector_size(16)));

struct LwVdLds { // the LDS of a workgroup
	double sum[LW_VD_GROUP];    // the line's chunk sums (k_vad)
	uint64_t bits[LW_VD_WORDS]; // raw decisions: bit j of the list is frame t0 - ctx + j
};
static_assert(sizeof(LwVdLds) == LW_VD_LDS, "LW_VD_LDS is the structure's size");

struct LwVdTile { // what a workgroup works on; the same for all its lanes
	uint64_t n, fill_end;
	uint64_t t0;      // first frame of the tile
	uint32_t tile_i;  // the tile's number in its row
	uint32_t chunks;  // of the row
	uint64_t src_at;  // element of frame 0 of the row and channel's energy line in the source
	uint64_t mask_at; // byte of frame 0 of the row and channel in the mask
	uint64_t list_at; // the row and channel's chunk sums in a.part
	uint64_t thr_at;  // entry of the row and channel in d_thr and a.thr
};

LW_VD_FN void lw_vd_tile(const LwVadArgs &a, uint32_t tile_i, uint32_t by, uint32_t bz, LwVdTile &t)
{
	const uint64_t row = (uint64_t)a.row0 + bz;
	const LwVadRow r = a.rows[row];
	t.n = r.n, t.fill_end = r.fill_end, t.tile_i = tile_i, t.chunks = r.chunks;
	t.t0 = (uint64_t)tile_i * a.tile;
	t.src_at = ((row * a.ch + by) * a.F + a.line) * a.line_el;
	t.mask_at = (row * a.ch + by) * a.line_el;
	t.list_at = r.list_at + (uint64_t)by * r.chunks;
	t.thr_at = row * a.ch + by;
}

// ---- the tree.  On the device every lane brings its entry and leaves with the wave's; the host build runs a wave at a time
// (lane is 0) and folds the 64 entries as the contract writes it, t[j] = t[2j] + t[2j + 1]
template <class E>
LW_VD_FN double lw_vd_wave_tree(uint32_t lane, E entry)
{
#ifdef LW_VAD_HOST
	double t[LW_VD_GROUP];
	for (uint32_t l = 0; l < LW_VD_GROUP; l++)
		t[l] = entry(l);
	for (uint32_t n = LW_VD_GROUP / 2; n; n >>= 1)
		for (uint32_t j = 0; j < n; j++)
			t[j] = t[2 * j] + t[2 * j + 1];
	(void)lane;
	return t[0];
#else
	double t = entry(lane);
#pragma unroll
	for (int o = 1; o < 64; o <<= 1)
		t = t + __shfl_xor(t, o, 64);
	return t;
#endif
}

// ... and the wave's ballot: bit l is lane l's decision
template <class P>
LW_VD_FN uint64_t lw_vd_wave_ballot(uint32_t lane, P decision)
{
#ifdef LW_VAD_HOST
	uint64_t w = 0;
	for (uint32_t l = 0; l < 64u; l++)
		w |= (uint64_t)(decision(l) ? 1u : 0u) << l;
	(void)lane;
	return w;
#else
	return __ballot(decision(lane));
#endif
}

// ---- the chunk sum ("normalising rows", step 1, the sum alone): lane `lane`'s share of chunk c of the line at element `at` --
// frames 4 lane .. 4 lane + 3 of the chunk, those at or beyond n as +0.0
LW_VD_FN double lw_vd_chunk_lane(const float *LW_VD_RESTRICT src, uint64_t at, uint64_t n, uint32_t c, uint32_t lane)
{
	const uint64_t e0 = (uint64_t)c * LW_VD_CHUNK + lane * 4u;
	float x0 = 0.0f, x1 = 0.0f, x2 = 0.0f, x3 = 0.0f;
	if (e0 + 4u <= n) {
		const float *s = src + at + e0;
		if ((((uintptr_t)src >> 2) + at + e0) & 3u)
			x0 = s[0], x1 = s[1], x2 = s[2], x3 = s[3];
		else { // ONE 16-byte load
			const LwVdV4 q = *(const LwVdV4 *)s;
			x0 = q[0], x1 = q[1], x2 = q[2], x3 = q[3];
		}
	} else {
		if (e0 < n)
			x0 = src[at + e0];
		if (e0 + 1u < n)
			x1 = src[at + e0 + 1u];
		if (e0 + 2u < n)
			x2 = src[at + e0 + 2u];
	}
	return (((double)x0 + (double)x1) + (double)x2) + (double)x3;
}

LW_VD_FN double lw_vd_chunk(const float *LW_VD_RESTRICT src, uint64_t at, uint64_t n, uint32_t c, uint32_t lane)
{
	return lw_vd_wave_tree(lane, [&](uint32_t l) { return lw_vd_chunk_lane(src, at, n, c, l); });
}

// ---- k_vad: one wave's chunks of the line into the workgroup's list
LW_VD_FN void lw_vd_sum_lds(const LwVadArgs &a, const LwVdTile &t, LwVdLds &l, uint32_t wave, uint32_t lane)
{
	for (uint32_t c = wave; c < t.chunks && c < LW_VD_GROUP; c += LW_VD_WAVES) { // (the host admits rows of at most 64 chunks here)
		const double s = lw_vd_chunk(a.src, t.src_at, t.n, c, lane);
		if (lane == 0)
			l.sum[c] = s;
	}
}

// (behind a barrier) S of a list of at most 64 entries: the entry itself, or ONE tree padded with +0.0
LW_VD_FN double lw_vd_fold_lds(const LwVdLds &l, uint32_t chunks, uint32_t lane)
{
	if (chunks == 1u)
		return l.sum[0];
	return lw_vd_wave_tree(lane, [&](uint32_t i) { return i < chunks ? l.sum[i] : 0.0; });
}

// ---- k_vad_sum: one wave's chunks of workgroup bx of a row and channel into the row's chunk list
LW_VD_FN void lw_vd_sum_wave(const LwVadArgs &a, uint32_t bx, uint32_t by, uint32_t bz, uint32_t wave, uint32_t lane)
{
	LwVdTile t;
	lw_vd_tile(a, 0u, by, bz, t);
	uint64_t c = ((uint64_t)bx * LW_VD_WAVES + wave) * a.sum_per_wave;
	for (uint32_t i = 0; i < a.sum_per_wave && c < t.chunks; i++, c++) {
		const double s = lw_vd_chunk(a.src, t.src_at, t.n, (uint32_t)c, lane);
		if (lane == 0)
			a.part[t.list_at + c] = s;
	}
}

// ---- k_vad_fold: a workgroup per row and channel.  The lists of the levels: the row and channel's part of a.part, then in turn
// the two halves of its scratch, ceil(longest / 64) and ceil(longest / 4096) doubles
struct LwVdLevels {
	const double *in;
	double *out, *other;
	uint64_t len, n, thr_at;
};

LW_VD_FN void lw_vd_levels(const LwVadArgs &a, uint32_t by, uint32_t bz, LwVdLevels &v)
{
	LwVdTile t;
	lw_vd_tile(a, 0u, by, bz, t);
	v.len = t.chunks, v.n = t.n, v.thr_at = t.thr_at;
	v.in = v.len ? a.part + t.list_at : nullptr;
	v.out = a.scratch + t.thr_at * a.fold_scratch;
	v.other = v.out + ((uint64_t)a.sum_chunks + 63u) / 64u;
}

// one wave's groups of one level: group j of the list -> entry j of the next
LW_VD_FN void lw_vd_level_wave(const LwVdLevels &v, uint32_t wave, uint32_t lane)
{
	const uint64_t groups = (v.len + LW_VD_GROUP - 1u) / LW_VD_GROUP;
	for (uint64_t j = wave; j < groups; j += LW_VD_WAVES) {
		const double s = lw_vd_wave_tree(lane, [&](uint32_t i) {
			const uint64_t e = j * LW_VD_GROUP + i;
			return e < v.len ? v.in[e] : 0.0;
		});
		if (lane == 0)
			v.out[j] = s;
	}
}

// ... and behind the level's barrier
LW_VD_FN void lw_vd_level_next(LwVdLevels &v)
{
	double *was = v.out;
	v.len = (v.len + LW_VD_GROUP - 1u) / LW_VD_GROUP;
	v.in = was, v.out = v.other, v.other = was;
}

// the threshold into its two places (one lane)
LW_VD_FN void lw_vd_levels_out(const LwVadArgs &a, const LwVdLevels &v)
{
	const float thr = lw_vad_threshold_value(a.energy_threshold, a.energy_mean_scale, v.len ? v.in[0] : 0.0, v.n);
	a.thr[v.thr_at] = thr;
	if (a.d_thr)
		a.d_thr[v.thr_at] = thr;
}

// ---- the decide phase.  One wave's words of the raw decisions: bit j of the list is frame t0 - ctx + j, 0 outside [0, T)
LW_VD_FN void lw_vd_stage_wave(const LwVadArgs &a, const LwVdTile &t, float thr, LwVdLds &l, uint32_t wave, uint32_t lane)
{
	const uint32_t span = a.tile + 2u * a.ctx, words = (span + 63u) / 64u;
	const int64_t base = (int64_t)t.t0 - (int64_t)a.ctx;
	for (uint32_t w = wave; w < words; w += LW_VD_WAVES) {
		const uint64_t word = lw_vd_wave_ballot(lane, [&](uint32_t i) {
			const uint32_t j = w * 64u + i;
			const int64_t f = base + (int64_t)j;
			return j < span && f >= 0 && (uint64_t)f < t.n && a.src[t.src_at + (uint64_t)f] > thr;
		});
		if (lane == 0)
			l.bits[w] = word;
	}
}

// the decisions set among bits [lo, hi) of the list, lo < hi
LW_VD_FN uint32_t lw_vd_count(const LwVdLds &l, uint32_t lo, uint32_t hi)
{
	const uint32_t w0 = lo >> 6, w1 = (hi - 1u) >> 6;
	uint32_t c = 0;
	for (uint32_t w = w0; w <= w1; w++) {
		uint64_t m = l.bits[w];
		if (w == w0)
			m &= ~(uint64_t)0 << (lo & 63u);
		if (w == w1 && (hi & 63u))
			m &= ((uint64_t)1 << (hi & 63u)) - 1u;
		c += (uint32_t)__builtin_popcountll(m);
	}
	return c;
}

// rules 3 and 4 for one frame of the tile: the mask's byte
LW_VD_FN uint32_t lw_vd_byte(const LwVadArgs &a, const LwVdTile &t, const LwVdLds &l, uint64_t f)
{
	if (f >= t.n)
		return 0u;
	const int64_t base = (int64_t)t.t0 - (int64_t)a.ctx;
	const int64_t lo = (int64_t)f - (int64_t)a.ctx < 0 ? 0 : (int64_t)f - (int64_t)a.ctx;
	const int64_t hi = (int64_t)f + (int64_t)a.ctx + 1 > (int64_t)t.n ? (int64_t)t.n : (int64_t)f + (int64_t)a.ctx + 1;
	const uint32_t num = lw_vd_count(l, (uint32_t)(lo - base), (uint32_t)(hi - base));
	return lw_vad_voiced_value(num, (uint64_t)(hi - lo), a.proportion_threshold) ? 1u : 0u;
}

// (behind a barrier) the lane's groups of four mask bytes of the tile's share of [0, fill_end)
LW_VD_FN void lw_vd_write(const LwVadArgs &a, const LwVdTile &t, const LwVdLds &l, uint32_t tid)
{
	const uint64_t end = t.t0 + a.tile < t.fill_end ? t.t0 + a.tile : t.fill_end;
	if (t.t0 >= end)
		return;
	uint8_t *m = a.mask + t.mask_at;
	const uint32_t head = (uint32_t)((uintptr_t)(m + t.t0) & 3u);
	const uint32_t groups = (uint32_t)((end - t.t0 + head + 3u) / 4u);
	for (uint32_t g = tid; g < groups; g += LW_VD_THREADS) {
		const int64_t f0 = (int64_t)t.t0 - (int64_t)head + (int64_t)g * 4;
		if (f0 >= (int64_t)t.t0 && (uint64_t)f0 + 4u <= end) { // all four are the tile's: ONE dword
			uint32_t v = 0;
#pragma unroll
			for (uint32_t k = 0; k < 4u; k++)
				v |= lw_vd_byte(a, t, l, (uint64_t)f0 + k) << (8u * k);
			*(uint32_t *)(m + f0) = v;
			continue;
		}
		for (int64_t f = f0; f < f0 + 4; f++) // the ragged head and tail of the span
			if (f >= (int64_t)t.t0 && (uint64_t)f < end)
				m[f] = (uint8_t)lw_vd_byte(a, t, l, (uint64_t)f);
	}
}

// what a decide workgroup does, in this order (k_vad and k_vad_decide below; tests/san/vad_host.cpp on the host)
//   skip    a tile beyond fill_end has nothing to do, unless it is tile 0 and owes d_thr
//   thr     sums (k_vad): lw_vd_sum_lds, barrier, lw_vd_fold_lds, lw_vad_threshold_value -- only where a frame of the tile is
//           decided or d_thr is owed, and the row has a frame; otherwise a.thr's entry, or energy_threshold
//   stage   where the tile holds a frame: lw_vd_stage_wave, barrier
//   write   lw_vd_write
LW_VD_FN bool lw_vd_owes_thr(const LwVadArgs &a, const LwVdTile &t)
{
	return a.thr_out && a.d_thr && t.tile_i == 0;
}

#ifndef LW_VAD_HOST

template <bool SUMS>
LW_VD_FN void lw_vd_workgroup(const LwVadArgs &a, LwVdLds &l)
{
	LwVdTile t;
	lw_vd_tile(a, blockIdx.x, blockIdx.y, blockIdx.z, t);
	const bool owes = lw_vd_owes_thr(a, t), frames = t.t0 < t.n;
	if (t.t0 >= t.fill_end && !owes)
		return;
	const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
	float thr = a.energy_threshold;
	if (frames || owes) { // (the same in every lane)
		if (SUMS) {
			if (t.n && a.energy_mean_scale != 0.0f) {
				lw_vd_sum_lds(a, t, l, wave, lane);
				__syncthreads();
				thr = lw_vad_threshold_value(a.energy_threshold, a.energy_mean_scale, lw_vd_fold_lds(l, t.chunks, lane), t.n);
			}
		} else if (a.thr) {
			thr = a.thr[t.thr_at];
		}
	}
	if (owes && threadIdx.x == 0)
		a.d_thr[t.thr_at] = thr;
	if (frames) {
		lw_vd_stage_wave(a, t, thr, l, wave, lane);
		__syncthreads();
	}
	lw_vd_write(a, t, l, threadIdx.x);
}

__global__ void __launch_bounds__(LW_VD_THREADS) k_vad(LwVadArgs a)
{
	__shared__ LwVdLds l;
	lw_vd_workgroup<true>(a, l);
}

__global__ void __launch_bounds__(LW_VD_THREADS) k_vad_decide(LwVadArgs a)
{
	__shared__ LwVdLds l;
	lw_vd_workgroup<false>(a, l);
}

__global__ void __launch_bounds__(LW_VD_THREADS) k_vad_sum(LwVadArgs a)
{
	lw_vd_sum_wave(a, blockIdx.x, blockIdx.y, blockIdx.z, threadIdx.x >> 6, threadIdx.x & 63u);
}

__global__ void __launch_bounds__(LW_VD_THREADS) k_vad_fold(LwVadArgs a)
{
	LwVdLevels v;
	lw_vd_levels(a, blockIdx.x, blockIdx.z, v);
	while (v.len > 1) { // (the same count in every lane)
		lw_vd_level_wave(v, threadIdx.x >> 6, threadIdx.x & 63u);
		__syncthreads(); // the level's list is complete, and visible to the workgroup, before anyone reads it
		lw_vd_level_next(v);
	}
	if (threadIdx.x == 0)
		lw_vd_levels_out(a, v);
}

__global__ void __launch_bounds__(LW_VD_THREADS) k_vad_fill(float *d_thr, uint64_t n, float value)
{
	for (uint64_t i = threadIdx.x; i < n; i += LW_VD_THREADS)
		d_thr[i] = value;
}

static bool lw_vd_args_ok(const LwVadArgs &a, uint32_t n_rows)
{
	return n_rows != 0 && n_rows <= 65535u && a.ch != 0 && a.ch <= 65535u && a.F != 0 && a.line < a.F && a.rows && lw_vad_tile_ok(a.tile) &&
		a.ctx <= LW_VD_MAX_CONTEXT;
}

static bool lw_vd_decide_ok(const LwVadArgs &a, uint32_t n_rows)
{
	return lw_vd_args_ok(a, n_rows) && a.tiles != 0 && a.tiles <= LW_VD_MAX_TILES;
}

hipError_t lw_launch_vad(const LwVadArgs &a, uint32_t n_rows, hipStream_t st)
{
	if (!lw_vd_decide_ok(a, n_rows) || (uint64_t)a.tiles * a.tile > LW_VD_FUSED_MAX + LW_VD_MAX_TILE - 1u)
		return hipErrorInvalidValue;
	return lw_launch_k(k_vad, dim3(a.tiles, a.ch, n_rows), dim3(LW_VD_THREADS), 0, st, a);
}

hipError_t lw_launch_vad_decide(const LwVadArgs &a, uint32_t n_rows, hipStream_t st)
{
	if (!lw_vd_decide_ok(a, n_rows))
		return hipErrorInvalidValue;
	return lw_launch_k(k_vad_decide, dim3(a.tiles, a.ch, n_rows), dim3(LW_VD_THREADS), 0, st, a);
}

hipError_t lw_launch_vad_sum(const LwVadArgs &a, uint32_t n_rows, hipStream_t st)
{
	if (!lw_vd_args_ok(a, n_rows) || !a.src || !a.part || !a.sum_chunks || !a.sum_per_wave || !a.sum_tiles ||
			(uint64_t)a.sum_tiles * a.sum_per_wave * LW_VD_WAVES < a.sum_chunks)
		return hipErrorInvalidValue;
	return lw_launch_k(k_vad_sum, dim3(a.sum_tiles, a.ch, n_rows), dim3(LW_VD_THREADS), 0, st, a);
}

hipError_t lw_launch_vad_fold(const LwVadArgs &a, uint32_t n_rows, hipStream_t st)
{
	if (!lw_vd_args_ok(a, n_rows) || !a.thr || !a.scratch || !a.fold_scratch || (a.sum_chunks && !a.part))
		return hipErrorInvalidValue;
	return lw_launch_k(k_vad_fold, dim3(a.ch, 1, n_rows), dim3(LW_VD_THREADS), 0, st, a);
}

hipError_t lw_launch_vad_fill(float *d_thr, uint64_t n, float value, hipStream_t st)
{
	if (!d_thr || !n)
		return hipErrorInvalidValue;
	return lw_launch_k(k_vad_fill, dim3(1), dim3(LW_VD_THREADS), 0, st, d_thr, n, value);
}

#endif // LW_VAD_HOST
