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

#ifndef LW_KERNEL_HOST
#include "lw_kernels.hpp"
#endif

static_assert(LW_VD_WAVES == LW_LANES_WAVES && LW_VD_THREADS == LW_LANES_WAVES * 64u, "lw_lanes.hpp's plans and loops count four waves to a workgroup");

struct LwVdLds { // the LDS of a workgroup
	double sum[LW_SUM_GROUP];    // the line's chunk sums (k_vad)
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

LW_LANES_FN void lw_vd_tile(const LwVadArgs &a, uint32_t tile_i, uint32_t by, uint32_t bz, LwVdTile &t)
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

// ---- the chunk sum ("normalising rows", step 1, the sum alone): lane `lane`'s share of chunk c of the line at element `at` --
// frames 4 lane .. 4 lane + 3 of the chunk, those at or beyond n as +0.0.  (This load and lw_kernels_norm.hip's stay two: one
// function for both, which hands the four floats on, changed either kernel's code.)
LW_LANES_FN double lw_vd_chunk_lane(const float *LW_LANES_RESTRICT src, uint64_t at, uint64_t n, uint32_t c, uint32_t lane)
{
	const uint64_t e0 = (uint64_t)c * LW_SUM_CHUNK + lane * 4u;
	float x0 = 0.0f, x1 = 0.0f, x2 = 0.0f, x3 = 0.0f;
	if (e0 + 4u <= n) {
		const float *s = src + at + e0;
		if ((((uintptr_t)src >> 2) + at + e0) & 3u)
			x0 = s[0], x1 = s[1], x2 = s[2], x3 = s[3];
		else { // ONE 16-byte load
			const LwV4 q = *(const LwV4 *)s;
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

LW_LANES_FN double lw_vd_chunk(const float *LW_LANES_RESTRICT src, uint64_t at, uint64_t n, uint32_t c, uint32_t lane)
{
	return lw_wave_tree<double>(lane, [&](uint32_t l) { return lw_vd_chunk_lane(src, at, n, c, l); });
}

// ---- k_vad: one wave's chunks of the line into the workgroup's list
LW_LANES_FN void lw_vd_sum_lds(const LwVadArgs &a, const LwVdTile &t, LwVdLds &l, uint32_t wave, uint32_t lane)
{
	for (uint32_t c = wave; c < t.chunks && c < LW_SUM_GROUP; c += LW_VD_WAVES) { // (the host admits rows of at most 64 chunks here)
		const double s = lw_vd_chunk(a.src, t.src_at, t.n, c, lane);
		if (lane == 0)
			l.sum[c] = s;
	}
}

// (behind a barrier) S of a list of at most 64 entries: the entry itself, or ONE tree padded with +0.0
LW_LANES_FN double lw_vd_fold_lds(const LwVdLds &l, uint32_t chunks, uint32_t lane)
{
	if (chunks == 1u)
		return l.sum[0];
	return lw_wave_tree<double>(lane, [&](uint32_t i) { return i < chunks ? l.sum[i] : 0.0; });
}

// ---- k_vad_sum: one wave's chunks of workgroup bx of a row and channel into the row's chunk list
LW_LANES_FN void lw_vd_sum_wave(const LwVadArgs &a, uint32_t bx, uint32_t by, uint32_t bz, uint32_t wave, uint32_t lane)
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

// ---- k_vad_fold: a workgroup per row and channel: the levels of lw_lanes.hpp over the row and channel's part of a.part and
// fold_scratch doubles of its own
struct LwVdLevels : LwLevels<double> {
	uint64_t n, thr_at;
};

LW_LANES_FN void lw_vd_levels(const LwVadArgs &a, uint32_t by, uint32_t bz, LwVdLevels &v)
{
	LwVdTile t;
	lw_vd_tile(a, 0u, by, bz, t);
	lw_levels(v, t.chunks ? a.part + t.list_at : (const double *)nullptr, (uint64_t)t.chunks, a.scratch + t.thr_at * a.fold_scratch, (uint64_t)a.sum_chunks);
	v.n = t.n, v.thr_at = t.thr_at;
}

LW_LANES_FN void lw_vd_level_wave(const LwVdLevels &v, uint32_t wave, uint32_t lane) // one wave's groups of one level
{
	lw_level_wave(v, wave, lane);
}

LW_LANES_FN void lw_vd_level_next(LwVdLevels &v) // ... and behind the level's barrier
{
	lw_level_next(v);
}

// the threshold into its two places (one lane)
LW_LANES_FN void lw_vd_levels_out(const LwVadArgs &a, const LwVdLevels &v)
{
	const float thr = lw_vad_threshold_value(a.energy_threshold, a.energy_mean_scale, v.len ? v.in[0] : 0.0, v.n);
	a.thr[v.thr_at] = thr;
	if (a.d_thr)
		a.d_thr[v.thr_at] = thr;
}

// ---- the decide phase.  One wave's words of the raw decisions: bit j of the list is frame t0 - ctx + j, 0 outside [0, T)
LW_LANES_FN void lw_vd_stage_wave(const LwVadArgs &a, const LwVdTile &t, float thr, LwVdLds &l, uint32_t wave, uint32_t lane)
{
	const uint32_t span = a.tile + 2u * a.ctx, words = (span + 63u) / 64u;
	lw_bits_fill(l.bits, span, words, (int64_t)t.t0 - (int64_t)a.ctx, t.n, wave, lane, [&](uint32_t, uint64_t f) { return a.src[t.src_at + f] > thr; });
}

// rules 3 and 4 for one frame of the tile: the mask's byte
LW_LANES_FN uint32_t lw_vd_byte(const LwVadArgs &a, const LwVdTile &t, const LwVdLds &l, uint64_t f)
{
	if (f >= t.n)
		return 0u;
	const int64_t base = (int64_t)t.t0 - (int64_t)a.ctx;
	const int64_t lo = (int64_t)f - (int64_t)a.ctx < 0 ? 0 : (int64_t)f - (int64_t)a.ctx;
	const int64_t hi = (int64_t)f + (int64_t)a.ctx + 1 > (int64_t)t.n ? (int64_t)t.n : (int64_t)f + (int64_t)a.ctx + 1;
	const uint32_t num = lw_bits_count<uint32_t>(l.bits, (uint32_t)(lo - base), (uint32_t)(hi - base), 0u); // (lo < hi: f is in it)
	return lw_vad_voiced_value(num, (uint64_t)(hi - lo), a.proportion_threshold) ? 1u : 0u;
}

// (behind a barrier) the lane's groups of four mask bytes of the tile's share of [0, fill_end)
LW_LANES_FN void lw_vd_write(const LwVadArgs &a, const LwVdTile &t, const LwVdLds &l, uint32_t tid)
{
	const uint64_t end = t.t0 + a.tile < t.fill_end ? t.t0 + a.tile : t.fill_end;
	lw_mask_write(a.mask + t.mask_at, t.t0, end, tid, [&](uint64_t f) { return lw_vd_byte(a, t, l, f); });
}

// what a decide workgroup does, in this order (k_vad and k_vad_decide below; tests/san/vad_host.cpp on the host)
//   skip    a tile beyond fill_end has nothing to do, unless it is tile 0 and owes d_thr
//   thr     sums (k_vad): lw_vd_sum_lds, barrier, lw_vd_fold_lds, lw_vad_threshold_value -- only where a frame of the tile is
//           decided or d_thr is owed, and the row has a frame; otherwise a.thr's entry, or energy_threshold
//   stage   where the tile holds a frame: lw_vd_stage_wave, barrier
//   write   lw_vd_write
LW_LANES_FN bool lw_vd_owes_thr(const LwVadArgs &a, const LwVdTile &t)
{
	return a.thr_out && a.d_thr && t.tile_i == 0;
}

#ifndef LW_KERNEL_HOST

template <bool SUMS>
LW_LANES_FN void lw_vd_workgroup(const LwVadArgs &a, LwVdLds &l)
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

#endif // LW_KERNEL_HOST
