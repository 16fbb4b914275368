// Normalising rows (product code, gfx950): k_norm_sum, k_norm_fold and k_norm_apply, the kernels of lw_norm_rows.  A pass of its
// own over f32 [row][ch][F][capacity] rows (a planar waveform is F = 1) by the rule of include/lewton_amd.h ("normalising rows"),
// bit for bit.  The sums are DOUBLE and their ORDER is the contract: there is no atomic anywhere, and neither the grid nor the
// plan's per_wave figures decide which values meet in an addition.  Three launches on one stream:
//   k_norm_sum    a wave takes chunks of 256 consecutive elements of one line, cut by index from the line's element 0.  Lane i
//                 holds elements 4i .. 4i + 3 (one 16-byte load where the chunk's address allows, four 4-byte loads otherwise,
//                 element by element where n cuts the group), adds them and their squares in double in the contract's order,
//                 the 64 lanes fold by the xor butterfly 1, 2, .. 32 (__shfl_xor on doubles) -- the adjacent-pair tree, the
//                 same bits in every lane since double addition commutes -- and lane 0 stores the chunk's triple (sum, sum of
//                 squares, largest |x| as a bit pattern) into the row's chunk list: ONE plain store, line-major, so every
//                 scope's list is contiguous.
//   k_norm_fold   folds a scope's list 64 entries at a time by the same tree, level by level, to (S1, S2, P), then the scalars
//                 (m, g) by lw_norm_scalars_value, for k_norm_apply and into d_stats.  A wave per scope while every list of the
//                 call has at most 64 entries (utterance CMVN: thousands of scopes of a dozen chunks); otherwise a workgroup per
//                 scope, whose four waves share a level's groups and keep the levels' lists in scratch of the scope's own,
//                 __syncthreads() between levels.  No workgroup waits for another.  The fold stayed a launch of its own.
//   k_norm_apply  z = (float)(((double)x - m) * g) and the fill with +0.0, streamed as k_feat_fin streams: lane i of a wave takes
//                 group i of a run, a group = four consecutive elements at a 16-byte boundary of the destination line; a group
//                 that the line's start, n or fill_end cuts goes element by element (the scalar head and tail).  A source line
//                 that sits differently against the boundaries is loaded with four 4-byte loads.  Offsets are 64-bit.
// center = 0 without a scale has m = +0.0, g = 1.0 whatever the data: k_norm_apply alone (a.plain), and k_norm_fold before it
// only where d_stats is owed.  Nothing at or beyond n of a source line is read, nothing outside [0, fill_end) of a destination
// line written.  tests/san/norm_host.cpp compiles this file for the host (LW_NORM_HOST) and runs it workgroup by workgroup.
#include "lw_norm.hpp"

#ifndef LW_KERNEL_HOST
#include "lw_kernels.hpp"
#endif

static_assert(LW_NM_WAVES == LW_LANES_WAVES, "lw_lanes.hpp's plans and loops count four waves to a workgroup");

// ---- a triple's way through lw_wave_tree (lw_wave_add: lw_norm.hpp)
#ifndef LW_KERNEL_HOST
LW_LANES_FN LwNormTriple lw_wave_xor(const LwNormTriple &t, int o)
{
	LwNormTriple u;
	u.s1 = __shfl_xor(t.s1, o, 64), u.s2 = __shfl_xor(t.s2, o, 64), u.pk = (uint32_t)__shfl_xor((int)t.pk, o, 64), u.pad_ = 0;
	return u;
}
#endif

// ---- k_norm_sum: lane `lane`'s share of chunk c of the line at element `at`: elements 4 lane .. 4 lane + 3 of the chunk.  (This
// load and lw_kernels_vad.hip's stay two: the triple needs the floats again, and one function for both changed either kernel.)
LW_LANES_FN LwNormTriple lw_nm_chunk_lane(const LwNormArgs &a, uint64_t at, uint64_t n, uint32_t c, uint32_t lane)
{
	const uint64_t e0 = (uint64_t)c * LW_SUM_CHUNK + lane * 4u;
	LwF4 x = {{0.0f, 0.0f, 0.0f, 0.0f}};
	if (e0 + 4u <= n) {
		const float *s = a.src + at + e0;
		if ((((uintptr_t)a.src >> 2) + at + e0) & 3u)
			x.v[0] = s[0], x.v[1] = s[1], x.v[2] = s[2], x.v[3] = s[3];
		else { // ONE 16-byte load (as a vector: four float members the compiler merges with the branch above into 4-byte loads)
			const LwV4 q = *(const LwV4 *)s;
			x.v[0] = q[0], x.v[1] = q[1], x.v[2] = q[2], x.v[3] = q[3];
		}
	} else {
		for (int j = 0; j < 4; j++)
			if (e0 + j < n)
				x.v[j] = a.src[at + e0 + j];
	}
	const double d0 = (double)x.v[0], d1 = (double)x.v[1], d2 = (double)x.v[2], d3 = (double)x.v[3];
	LwNormTriple t;
	t.s1 = ((d0 + d1) + d2) + d3;
	t.s2 = ((d0 * d0 + d1 * d1) + d2 * d2) + d3 * d3;
	t.pk = 0, t.pad_ = 0;
#pragma unroll
	for (int j = 0; j < 4; j++) { // (an element at or beyond n is +0.0 here: the bit pattern 0, below every other)
		const uint32_t b = __builtin_bit_cast(uint32_t, x.v[j]) & 0x7fffffffu;
		t.pk = b > t.pk ? b : t.pk;
	}
	return t;
}

// one wave's slots of workgroup bx of row bz
LW_LANES_FN void lw_nm_sum_wave(const LwNormArgs &a, uint32_t bx, uint32_t bz, uint32_t wave, uint32_t lane)
{
	const uint64_t row = (uint64_t)a.row0 + bz, lines = (uint64_t)a.ch * a.F, slots = lines * a.plan.sum_chunks;
	const LwNormRow r = a.rows[row];
	uint64_t slot = ((uint64_t)bx * LW_NM_WAVES + wave) * a.plan.sum_per_wave;
	for (uint32_t i = 0; i < a.plan.sum_per_wave && slot < slots; i++, slot++) {
		const uint64_t line = (uint32_t)slot / a.plan.sum_chunks; // (slots: 32 bits count them)
		const uint32_t c = (uint32_t)slot % a.plan.sum_chunks;
		if (c >= r.chunks)
			continue;
		const uint64_t at = (row * lines + line) * a.line_el;
		const LwNormTriple t = lw_wave_tree<LwNormTriple>(lane, [&](uint32_t l) { return lw_nm_chunk_lane(a, at, r.n, c, l); });
		if (lane == 0)
			a.part[r.part_at + line * r.chunks + c] = t;
	}
}

// ---- k_norm_fold
LW_LANES_FN LwNormTriple lw_nm_entry(const LwNormTriple *list, uint64_t len, uint64_t i)
{
	return i < len ? list[i] : LwNormTriple{0.0, 0.0, 0u, 0u};
}

// the scope's scalars from its triple, into their two places (one lane)
LW_LANES_FN void lw_nm_scope_out(const LwNormArgs &a, uint64_t row, uint32_t scope, uint64_t n, const LwNormTriple &t)
{
	double m, g;
	lw_norm_scalars_value(a.center, a.scale, a.eps, a.target, t.s1, t.s2, __builtin_bit_cast(float, t.pk), (uint64_t)a.plan.scope_lines * n, m, g);
	const uint64_t at = (row * a.plan.scopes + scope) * 2u;
	a.sc[at] = m, a.sc[at + 1] = g;
	if (a.d_stats)
		a.d_stats[at] = m, a.d_stats[at + 1] = g;
}

// the scope's list, or nothing to fold: plain, or an empty row (lw_norm_scalars_value makes m = +0.0, g = 1.0 of N = 0)
LW_LANES_FN const LwNormTriple *lw_nm_scope_list(const LwNormArgs &a, const LwNormRow &r, uint32_t scope, uint64_t &len)
{
	len = a.plain ? 0u : (uint64_t)a.plan.scope_lines * r.chunks;
	return len ? a.part + r.part_at + scope * len : nullptr;
}

// a wave per scope: every list has at most 64 entries
LW_LANES_FN void lw_nm_fold_wave(const LwNormArgs &a, uint32_t bx, uint32_t bz, uint32_t wave, uint32_t lane)
{
	const uint64_t row = (uint64_t)a.row0 + bz;
	const uint32_t scope = bx * LW_NM_WAVES + wave;
	if (scope >= a.plan.scopes)
		return;
	const LwNormRow r = a.rows[row];
	uint64_t len;
	const LwNormTriple *list = lw_nm_scope_list(a, r, scope, len);
	LwNormTriple t{0.0, 0.0, 0u, 0u};
	if (len == 1)
		t = list[0];
	else if (len > 1)
		t = lw_wave_tree<LwNormTriple>(lane, [&](uint32_t l) { return lw_nm_entry(list, len, l); });
	if (lane == 0)
		lw_nm_scope_out(a, row, scope, len ? r.n : 0u, t);
}

// a workgroup per scope: the levels of lw_lanes.hpp over the scope's part of a.part and fold_scratch triples of its own
struct LwNmLevels : LwLevels<LwNormTriple> {
	uint64_t n;
};

LW_LANES_FN void lw_nm_levels(const LwNormArgs &a, uint32_t bx, uint32_t bz, LwNmLevels &v)
{
	const uint64_t row = (uint64_t)a.row0 + bz;
	const LwNormRow r = a.rows[row];
	uint64_t len;
	const LwNormTriple *list = lw_nm_scope_list(a, r, bx, len);
	lw_levels(v, list, len, a.scratch + (row * a.plan.scopes + bx) * a.plan.fold_scratch, (uint64_t)a.plan.scope_lines * a.plan.sum_chunks);
	v.n = len ? r.n : 0u;
}

LW_LANES_FN void lw_nm_level_wave(const LwNmLevels &v, uint32_t wave, uint32_t lane) // one wave's groups of one level
{
	lw_level_wave(v, wave, lane);
}

LW_LANES_FN void lw_nm_level_next(LwNmLevels &v) // ... and behind the level's barrier
{
	lw_level_next(v);
}

LW_LANES_FN void lw_nm_levels_out(const LwNormArgs &a, uint32_t bx, uint32_t bz, const LwNmLevels &v)
{
	lw_nm_scope_out(a, (uint64_t)a.row0 + bz, bx, v.n, v.len ? v.in[0] : LwNormTriple{0.0, 0.0, 0u, 0u});
}

// ---- k_norm_apply
struct LwNmTile { // what a workgroup works on; the same for all its lanes
	uint64_t n, end; // the row's n and fill_end
	uint64_t ch_at;  // element of line 0, element 0 of the row and channel (the same in src and dst)
	uint64_t sc_at;  // the row's first scope in a.sc
	uint64_t run0;   // first run of the tile
};

LW_LANES_FN void lw_nm_tile(const LwNormArgs &a, uint32_t bx, uint32_t by, uint32_t bz, LwNmTile &t)
{
	const uint64_t row = (uint64_t)a.row0 + bz;
	const LwNormRow r = a.rows[row];
	t.n = r.n, t.end = r.fill_end;
	t.ch_at = (row * a.ch + by) * a.F * a.line_el;
	t.sc_at = row * a.plan.scopes * 2u;
	t.run0 = (uint64_t)bx * (LW_NM_WAVES * (uint64_t)a.plan.per_wave);
}

// one run for one lane
LW_LANES_FN void lw_nm_run(const LwNormArgs &a, const LwNmTile &t, uint32_t by, uint32_t run, uint32_t lane)
{
	const LwRunGroup gr = lw_run_group(a.plan.runs_per_line, a.src, a.dst, t.ch_at, a.line_el, run, lane);
	const uint64_t at = gr.at;
	const int64_t t0 = gr.t0;
	if (t0 >= (int64_t)t.end)
		return;
	double m = 0.0, g = 1.0;
	if (!a.plain) {
		const uint64_t scope = a.scope == 0 ? 0u : a.scope == 1 ? by : (uint64_t)by * a.F + gr.line;
		m = a.sc[t.sc_at + scope * 2u], g = a.sc[t.sc_at + scope * 2u + 1u];
	}
	if (t0 >= 0 && (uint64_t)t0 + 4u <= t.n) { // all four are data
		const float *s = a.src + at + t0;
		LwF4 x;
		if (gr.same)
			x = *(const LwF4 *)s;
		else
			x.v[0] = s[0], x.v[1] = s[1], x.v[2] = s[2], x.v[3] = s[3];
#pragma unroll
		for (int j = 0; j < 4; j++)
			x.v[j] = lw_norm_apply_value(x.v[j], m, g);
		*(LwF4 *)(a.dst + at + t0) = x;
		return;
	}
	if (t0 >= 0 && (uint64_t)t0 >= t.n && (uint64_t)t0 + 4u <= t.end) { // all four are fill
		*(LwF4 *)(a.dst + at + t0) = LwF4{{0.0f, 0.0f, 0.0f, 0.0f}};
		return;
	}
	for (int j = 0; j < 4; j++) { // the line's head, the tail of the data, the tail of the fill
		const int64_t f = t0 + j;
		if (f < 0 || (uint64_t)f >= t.end)
			continue;
		a.dst[at + f] = (uint64_t)f < t.n ? lw_norm_apply_value(a.src[at + f], m, g) : 0.0f;
	}
}

// the lane's runs of the tile
LW_LANES_FN void lw_nm_tile_apply(const LwNormArgs &a, const LwNmTile &t, uint32_t by, uint32_t tid)
{
	const uint32_t lane = tid & 63u, wave = tid >> 6;
	for (uint32_t i = 0; i < a.plan.per_wave; i++) {
		const uint64_t run = t.run0 + (uint64_t)i * LW_NM_WAVES + wave;
		if (run < a.plan.runs)
			lw_nm_run(a, t, by, (uint32_t)run, lane);
	}
}

#ifndef LW_KERNEL_HOST

__global__ void __launch_bounds__(LW_NM_THREADS) k_norm_sum(LwNormArgs a)
{
	lw_nm_sum_wave(a, blockIdx.x, blockIdx.z, threadIdx.x >> 6, threadIdx.x & 63u);
}

__global__ void __launch_bounds__(LW_NM_THREADS) k_norm_fold(LwNormArgs a)
{
	if (a.plan.fold_wave) { // (the whole grid takes this way, or none of it)
		lw_nm_fold_wave(a, blockIdx.x, blockIdx.z, threadIdx.x >> 6, threadIdx.x & 63u);
		return;
	}
	LwNmLevels v;
	lw_nm_levels(a, blockIdx.x, blockIdx.z, v);
	while (v.len > 1) { // (the same count in every lane)
		lw_nm_level_wave(v, threadIdx.x >> 6, threadIdx.x & 63u);
		__syncthreads(); // the level's list is complete, and visible to the workgroup, before anyone reads it
		lw_nm_level_next(v);
	}
	if (threadIdx.x == 0)
		lw_nm_levels_out(a, blockIdx.x, blockIdx.z, v);
}

__global__ void __launch_bounds__(LW_NM_THREADS) k_norm_apply(LwNormArgs a)
{
	LwNmTile t;
	lw_nm_tile(a, blockIdx.x, blockIdx.y, blockIdx.z, t);
	lw_nm_tile_apply(a, t, blockIdx.y, threadIdx.x);
}

static bool lw_nm_args_ok(const LwNormArgs &a, uint32_t n_rows)
{
	return n_rows != 0 && n_rows <= 65535u && a.ch != 0 && a.ch <= 65535u && a.F != 0 && a.rows && a.plan.scopes != 0 && a.plan.scope_lines != 0 &&
		(uint64_t)a.plan.scopes * a.plan.scope_lines == (uint64_t)a.ch * a.F;
}

hipError_t lw_launch_norm_sum(const LwNormArgs &a, uint32_t n_rows, hipStream_t st)
{
	if (!lw_nm_args_ok(a, n_rows) || a.plain || !a.src || !a.part || !a.plan.sum_chunks || !a.plan.sum_per_wave || !a.plan.sum_tiles ||
			(uint64_t)a.plan.sum_tiles * a.plan.sum_per_wave * LW_NM_WAVES < (uint64_t)a.ch * a.F * a.plan.sum_chunks)
		return hipErrorInvalidValue;
	return lw_launch_k(k_norm_sum, dim3(a.plan.sum_tiles, 1, n_rows), dim3(LW_NM_THREADS), 0, st, a);
}

hipError_t lw_launch_norm_fold(const LwNormArgs &a, uint32_t n_rows, hipStream_t st)
{
	if (!lw_nm_args_ok(a, n_rows) || !a.sc || (!a.plain && a.plan.sum_chunks && !a.part) || (!a.plan.fold_wave && (!a.scratch || !a.plan.fold_scratch)))
		return hipErrorInvalidValue;
	const uint32_t grid = a.plan.fold_wave ? (a.plan.scopes + LW_NM_WAVES - 1u) / LW_NM_WAVES : a.plan.scopes;
	return lw_launch_k(k_norm_fold, dim3(grid, 1, n_rows), dim3(LW_NM_THREADS), 0, st, a);
}

hipError_t lw_launch_norm_apply(const LwNormArgs &a, uint32_t n_rows, hipStream_t st)
{
	if (!lw_nm_args_ok(a, n_rows) || (!a.plain && !a.sc) || !a.plan.tiles || !a.plan.per_wave || !a.plan.runs_per_line ||
			(uint64_t)a.plan.runs_per_line * a.F != a.plan.runs || (uint64_t)a.plan.tiles * a.plan.per_wave * LW_NM_WAVES < a.plan.runs)
		return hipErrorInvalidValue;
	return lw_launch_k(k_norm_apply, dim3(a.plan.tiles, a.ch, n_rows), dim3(LW_NM_THREADS), 0, st, a);
}

#endif // LW_KERNEL_HOST
