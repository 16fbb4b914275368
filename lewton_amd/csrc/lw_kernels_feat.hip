// Finishing feature rows (product code, gfx950): k_feat_log and k_feat_fin, the kernels of lw_feat_rows.  A pass of its own over
// finished feature rows, f32 [row][ch][F][frame_capacity], by the rule of include/lewton_amd.h ("finishing feature rows"), bit
// for bit:
//   v = x > floor ? x : floor;  l = LOG(v) (lw_feat_log_value, double arithmetic);  M = max of l over the scope;
//   tt = M - top (-inf for top = +inf);  y = l > tt ? l : tt;  z = (y + add) * mul;  [n_frames, fill_end) as if x = floor.
// Two launches on one stream:
//   k_feat_log  reads x, stores l in its place in dst, and leaves each tile's maximum of l in a small device array: the lanes'
//               maxima through __shfl_xor within the wave, through LDS across the workgroup's four waves, then ONE plain vector
//               store per tile.  No workgroup waits for another.
//   k_feat_fin  every workgroup folds the maxima of its scope's tiles (at most about a thousand floats, from L2) into M, then
//               re-reads the l of its own tile from dst, stores z, and fills.  The scope's first workgroup stores M into d_max.
// top = +inf without d_max needs no M: k_feat_log alone then stores z and fills (a.final).
// Work (lw_feat.hpp): lane i of a wave takes group i of a run, a group = four consecutive frames at a 16-byte boundary of the
// destination line -- one 16-byte load and store where the whole group is data (or fill); a group that the line's start, n_frames
// or fill_end cuts goes element by element, which is the scalar head and tail.  A source line that sits differently against the
// 16-byte boundaries than its destination line is loaded with four 4-byte loads.  Offsets are 64-bit down to the address.
// Nothing beyond n_frames of a source line is read, nothing outside [0, fill_end) of a destination line written.
// tests/san/feat_host.cpp compiles this file for the host (LW_FEAT_HOST) and runs it workgroup by workgroup, lane by lane.
#include "lw_feat.hpp"

#ifndef LW_KERNEL_HOST
#include "lw_kernels.hpp"
#endif

static_assert(LW_FT_WAVES == LW_LANES_WAVES, "lw_lanes.hpp's plans count four waves to a workgroup");

struct LwFtTile { // what a workgroup works on; the same for all its lanes
	uint64_t n, end;  // the row's n_frames and fill_end
	uint64_t ch_at;   // element of line 0, frame 0 of the row and channel (the same in src and dst)
	uint64_t part_at; // element of the channel's first tile in a.part
	uint64_t run0;    // first run of the tile (64-bit: a tile's last runs may lie behind the channel's, which 32 bits count)
};

LW_LANES_FN void lw_ft_tile(const LwFeatArgs &a, uint32_t bx, uint32_t by, uint32_t bz, LwFtTile &t)
{
	const uint64_t row = (uint64_t)a.row0 + bz;
	const LwFeatRow r = a.rows[row];
	t.n = r.n_frames, t.end = r.fill_end;
	t.ch_at = (row * a.ch + by) * a.F * a.line_el;
	t.part_at = (row * a.ch + by) * a.plan.tiles;
	t.run0 = (uint64_t)bx * (LW_FT_WAVES * (uint64_t)a.plan.per_wave);
}

// steps 1 and 2, and steps 4 and 5
LW_LANES_FN float lw_ft_log(const LwFeatArgs &a, float x)
{
	const float v = x > a.floor ? x : a.floor;
	return lw_feat_log_value(a.log, v);
}

LW_LANES_FN float lw_ft_finish(const LwFeatArgs &a, float l, float tt)
{
	const float y = l > tt ? l : tt;
	const float s = y + a.add;
	return s * a.mul;
}

LW_LANES_FN float lw_ft_tt(const LwFeatArgs &a, float M)
{
	return a.top == __builtin_inff() ? -__builtin_inff() : M - a.top;
}

// the lane's group of run `run` of the tile's channel (lw_run_group).  false: no such group below lim
LW_LANES_FN bool lw_ft_group(const LwFeatArgs &a, const LwFtTile &t, uint32_t run, uint32_t lane, uint64_t lim, uint64_t &at, int64_t &t0, bool &same)
{
	const LwRunGroup g = lw_run_group(a.plan.runs_per_line, a.src, a.dst, t.ch_at, a.line_el, run, lane);
	at = g.at, t0 = g.t0, same = g.same;
	return t0 < (int64_t)lim;
}

// ---- first launch: one run for one lane.  key: the lane's running maximum of l (lw_ft_key)
LW_LANES_FN void lw_ft_run_log(const LwFeatArgs &a, const LwFtTile &t, uint32_t run, uint32_t lane, int32_t &key)
{
	const uint64_t lim = a.final ? t.end : t.n;
	const float ninf = -__builtin_inff(), fillz = lw_ft_finish(a, a.l0, ninf);
	uint64_t at;
	int64_t t0;
	bool same;
	if (!lw_ft_group(a, t, run, lane, lim, at, t0, same))
		return;
	if (t0 >= 0 && (uint64_t)t0 + 4u <= t.n) { // all four are data
		const float *s = a.src + at + t0;
		LwF4 x;
		if (same)
			x = *(const LwF4 *)s;
		else
			x.v[0] = s[0], x.v[1] = s[1], x.v[2] = s[2], x.v[3] = s[3];
#pragma unroll
		for (int j = 0; j < 4; j++) {
			const float l = lw_ft_log(a, x.v[j]);
			const int32_t k = lw_ft_key(l);
			key = k > key ? k : key;
			x.v[j] = a.final ? lw_ft_finish(a, l, ninf) : l;
		}
		*(LwF4 *)(a.dst + at + t0) = x;
		return;
	}
	if (t0 >= 0 && (uint64_t)t0 >= t.n && (uint64_t)t0 + 4u <= t.end) { // all four are fill (only when final: t0 < lim)
		*(LwF4 *)(a.dst + at + t0) = LwF4{{fillz, fillz, fillz, fillz}};
		return;
	}
	for (int j = 0; j < 4; j++) { // the line's head, the tail of the data, the tail of the fill
		const int64_t f = t0 + j;
		if (f < 0 || (uint64_t)f >= lim)
			continue;
		if ((uint64_t)f < t.n) {
			const float l = lw_ft_log(a, a.src[at + f]);
			const int32_t k = lw_ft_key(l);
			key = k > key ? k : key;
			a.dst[at + f] = a.final ? lw_ft_finish(a, l, ninf) : l;
		} else {
			a.dst[at + f] = fillz;
		}
	}
}

// ---- second launch: one run for one lane; l comes from dst
LW_LANES_FN void lw_ft_run_fin(const LwFeatArgs &a, const LwFtTile &t, uint32_t run, uint32_t lane, float tt, float fillz)
{
	uint64_t at;
	int64_t t0;
	bool same;
	if (!lw_ft_group(a, t, run, lane, t.end, at, t0, same))
		return;
	if (t0 >= 0 && (uint64_t)t0 + 4u <= t.n) {
		LwF4 x = *(const LwF4 *)(a.dst + at + t0);
#pragma unroll
		for (int j = 0; j < 4; j++)
			x.v[j] = lw_ft_finish(a, x.v[j], tt);
		*(LwF4 *)(a.dst + at + t0) = x;
		return;
	}
	if (t0 >= 0 && (uint64_t)t0 >= t.n && (uint64_t)t0 + 4u <= t.end) {
		*(LwF4 *)(a.dst + at + t0) = LwF4{{fillz, fillz, fillz, fillz}};
		return;
	}
	for (int j = 0; j < 4; j++) {
		const int64_t f = t0 + j;
		if (f < 0 || (uint64_t)f >= t.end)
			continue;
		a.dst[at + f] = (uint64_t)f < t.n ? lw_ft_finish(a, a.dst[at + f], tt) : fillz;
	}
}

// ---- the phases of a workgroup, per lane; between them the workgroup's maximum of the lanes' keys
// first launch: the lane's runs of the tile
LW_LANES_FN int32_t lw_ft_tile_log(const LwFeatArgs &a, const LwFtTile &t, uint32_t tid)
{
	const uint32_t lane = tid & 63u, wave = tid >> 6;
	int32_t key = LW_FT_KEY_LOWEST;
	for (uint32_t i = 0; i < a.plan.per_wave; i++) {
		const uint64_t run = t.run0 + (uint64_t)i * LW_FT_WAVES + wave;
		if (run < a.plan.runs)
			lw_ft_run_log(a, t, (uint32_t)run, lane, key);
	}
	return key;
}

// ... and the tile's maximum into its place (one lane)
LW_LANES_FN void lw_ft_tile_part(const LwFeatArgs &a, const LwFtTile &t, uint32_t bx, int32_t key)
{
	a.part[t.part_at + bx] = lw_ft_unkey(key);
}

// second launch: the lane's share of the maxima of the scope's tiles
LW_LANES_FN int32_t lw_ft_scope_key(const LwFeatArgs &a, const LwFtTile &t, uint32_t by, uint32_t tid)
{
	const bool row = a.scope == 0; // LW_FEAT_SCOPE_ROW: the channels' tiles lie side by side
	const float *p = a.part + (row ? t.part_at - (uint64_t)by * a.plan.tiles : t.part_at);
	const uint32_t n = row ? a.ch * a.plan.tiles : a.plan.tiles;
	int32_t key = LW_FT_KEY_LOWEST;
	for (uint32_t i = tid; i < n; i += LW_FT_THREADS) {
		const int32_t k = lw_ft_key(p[i]);
		key = k > key ? k : key;
	}
	return key;
}

// ... and with the scope's maximum: M (to d_max by the scope's first lane), the clamp, the tile's runs
LW_LANES_FN void lw_ft_tile_fin(const LwFeatArgs &a, const LwFtTile &t, uint32_t bx, uint32_t by, uint32_t bz, uint32_t tid, int32_t key)
{
	const float M = t.n ? lw_ft_unkey(key) : a.l0; // (an empty scope's tiles all hold -inf)
	const float tt = lw_ft_tt(a, M), fillz = lw_ft_finish(a, a.l0, tt);
	const bool row = a.scope == 0;
	if (a.d_max && tid == 0 && bx == 0 && (!row || by == 0)) {
		const uint64_t r = (uint64_t)a.row0 + bz;
		a.d_max[row ? r : r * a.ch + by] = M;
	}
	const uint32_t lane = tid & 63u, wave = tid >> 6;
	for (uint32_t i = 0; i < a.plan.per_wave; i++) {
		const uint64_t run = t.run0 + (uint64_t)i * LW_FT_WAVES + wave;
		if (run < a.plan.runs)
			lw_ft_run_fin(a, t, (uint32_t)run, lane, tt, fillz);
	}
}

#ifndef LW_KERNEL_HOST

// the workgroup's maximum of its lanes' keys, in every lane: butterfly within the wave, then LDS across the waves
__device__ __forceinline__ int32_t lw_ft_wg_max(int32_t key, int32_t *lds, uint32_t tid)
{
#pragma unroll
	for (int o = 32; o; o >>= 1) {
		const int32_t other = __shfl_xor(key, o, 64);
		key = other > key ? other : key;
	}
	if ((tid & 63u) == 0)
		lds[tid >> 6] = key;
	__syncthreads();
#pragma unroll
	for (uint32_t w = 0; w < LW_FT_WAVES; w++)
		key = lds[w] > key ? lds[w] : key;
	return key;
}

__global__ void __launch_bounds__(LW_FT_THREADS) k_feat_log(LwFeatArgs a)
{
	__shared__ int32_t lds[LW_FT_WAVES];
	LwFtTile t;
	lw_ft_tile(a, blockIdx.x, blockIdx.y, blockIdx.z, t);
	int32_t key = lw_ft_tile_log(a, t, threadIdx.x);
	if (a.final)
		return;
	key = lw_ft_wg_max(key, lds, threadIdx.x);
	if (threadIdx.x == 0)
		lw_ft_tile_part(a, t, blockIdx.x, key);
}

__global__ void __launch_bounds__(LW_FT_THREADS) k_feat_fin(LwFeatArgs a)
{
	__shared__ int32_t lds[LW_FT_WAVES];
	LwFtTile t;
	lw_ft_tile(a, blockIdx.x, blockIdx.y, blockIdx.z, t);
	const int32_t key = lw_ft_wg_max(lw_ft_scope_key(a, t, blockIdx.y, threadIdx.x), lds, threadIdx.x);
	lw_ft_tile_fin(a, t, blockIdx.x, blockIdx.y, blockIdx.z, threadIdx.x, key);
}

static bool lw_ft_args_ok(const LwFeatArgs &a, uint32_t n_rows)
{
	return n_rows != 0 && n_rows <= 65535u && a.ch != 0 && a.ch <= 65535u && a.F != 0 && a.rows && a.plan.tiles != 0 && a.plan.per_wave != 0 &&
		a.plan.runs_per_line != 0 && (uint64_t)a.plan.runs_per_line * a.F == a.plan.runs &&
		(uint64_t)a.plan.tiles * a.plan.per_wave * LW_FT_WAVES >= a.plan.runs && (a.final || a.part);
}

hipError_t lw_launch_feat_log(const LwFeatArgs &a, uint32_t n_rows, hipStream_t st)
{
	if (!lw_ft_args_ok(a, n_rows))
		return hipErrorInvalidValue;
	return lw_launch_k(k_feat_log, dim3(a.plan.tiles, a.ch, n_rows), dim3(LW_FT_THREADS), 0, st, a);
}

hipError_t lw_launch_feat_fin(const LwFeatArgs &a, uint32_t n_rows, hipStream_t st)
{
	if (!lw_ft_args_ok(a, n_rows) || a.final)
		return hipErrorInvalidValue;
	return lw_launch_k(k_feat_fin, dim3(a.plan.tiles, a.ch, n_rows), dim3(LW_FT_THREADS), 0, st, a);
}

#endif // LW_KERNEL_HOST
