// Frame selection (product code, gfx950): k_select_count and k_select, the kernels of lw_select_rows.  A pass of its own from f32
// [row][ch][F][frame_capacity] rows and a uint8 mask [row][ch][frame_capacity] to rows of the same shape that hold the kept frames
// of every line, in order, from position 0, by the rule of include/lewton_amd.h ("frame decisions and frame selection").  Integer
// arithmetic and bit copies only.  TWO launches:
//   k_select_count  a workgroup of 256 lanes takes one tile of one row and channel: a lane counts the kept frames among its
//                   tile / 256 consecutive frames, the workgroup's total goes to the scratch list tile_counts.
//   k_select        a workgroup takes one tile and up to 16 feature lines.
//     base    the lanes add up the list's entries in front of the tile (base) and all of them (K), 256 partial sums folded in LDS;
//             the workgroup of tile 0 and line group 0 stores K into d_counts.
//     places  the lanes count as above; an exclusive prefix sum over the 256 counts in two steps of 16 (within groups of 16 lanes,
//             then over the 16 group totals); every lane writes the places of its kept frames into the compacted list in LDS.
//     copy    lane j copies src[t0 + place[j]] to dst[base + j] for every line of the group: the writes are coalesced, the reads a
//             monotone gather.  Values travel as bit patterns.
//     tail    +0.0 into the tile's share of positions [K, fill_end).
// Every position below fill_end is written once, nothing else is.  No atomics, no wait of a workgroup on another, offsets in 64
// bits.  Nothing at or beyond n of the mask or of a source line is read.  tests/san/select_host.cpp compiles this file for the
// host (LW_SELECT_HOST) and runs it workgroup by workgroup, the phases in the kernels' order.
#include "lw_select.hpp"

#include "lw_lanes.hpp"
#ifndef LW_KERNEL_HOST
#include "lw_kernels.hpp"
#endif

struct LwSeLds { // the LDS of a workgroup
	uint32_t cnt[LW_SE_THREADS];      // kept frames of every lane; then its exclusive prefix within its group of 16
	uint32_t tot[16];                 // kept frames of every group of 16 lanes
	uint64_t part[2 * LW_SE_THREADS]; // partial sums of the tile counts: in front of the tile, all
	uint16_t place[LW_SE_MAX_TILE];   // the tile's kept frames, compacted: their offsets from t0
};
static_assert(sizeof(LwSeLds) == LW_SE_LDS, "LW_SE_LDS is the structure's size");

struct LwSeTile { // what a workgroup works on; the same for all its lanes
	uint64_t n, fill_end;
	uint64_t t0;      // first frame of the tile
	uint32_t nt;      // frames of the tile below T
	uint32_t tile_i;  // the tile's number in its row
	uint32_t n_tiles; // tiles of the row that hold frames: ceil(T / tile)
	uint32_t G, grp;  // lines of this group, the group's number
	uint64_t mask_at; // element of frame 0 of the row and channel in the mask
	uint64_t at;      // element of frame 0 of the group's first line in source and destination
	uint64_t list_at; // entry of tile 0 of the row and channel in tile_counts
	uint64_t cnt_at;  // entry of the row and channel in d_counts
};

LW_LANES_FN void lw_se_tile(const LwSelectArgs &a, uint32_t tile_i, uint32_t grp, uint32_t by, uint32_t bz, LwSeTile &t)
{
	const uint64_t row = (uint64_t)a.row0 + bz;
	const LwSelectRow r = a.rows[row];
	const uint32_t f0 = grp * LW_SE_LINES;
	t.n = r.n, t.fill_end = r.fill_end, t.tile_i = tile_i, t.grp = grp;
	t.t0 = (uint64_t)tile_i * a.tile;
	const uint64_t end = t.t0 + a.tile;
	t.nt = t.t0 < r.n ? (uint32_t)((end < r.n ? end : r.n) - t.t0) : 0u;
	t.n_tiles = (uint32_t)((r.n + a.tile - 1u) / a.tile);
	t.G = a.F - f0 < LW_SE_LINES ? a.F - f0 : LW_SE_LINES;
	t.mask_at = (row * a.ch + by) * a.line_el;
	t.at = ((row * a.ch + by) * a.F + f0) * a.line_el;
	t.list_at = ((uint64_t)bz * a.ch + by) * a.tiles;
	t.cnt_at = row * a.ch + by;
}

// ---- the kept frames among the lane's tile / 256 consecutive frames
LW_LANES_FN uint32_t lw_se_lane_count(const LwSelectArgs &a, const LwSeTile &t, const uint8_t *LW_LANES_RESTRICT mask, uint32_t tid)
{
	const uint32_t per = a.tile / LW_SE_THREADS, lo = tid * per;
	uint32_t c = 0;
	for (uint32_t k = 0; k < per && lo + k < t.nt; k++)
		c += mask[t.mask_at + t.t0 + lo + k] != 0;
	return c;
}

LW_LANES_FN void lw_se_count(const LwSelectArgs &a, const LwSeTile &t, const uint8_t *LW_LANES_RESTRICT mask, LwSeLds &l, uint32_t tid)
{
	l.cnt[tid] = lw_se_lane_count(a, t, mask, tid);
}

// (behind a barrier) the totals of the groups of 16 lanes; cnt becomes the exclusive prefix within the group
LW_LANES_FN void lw_se_groups(LwSeLds &l, uint32_t tid)
{
	if (tid >= 16u)
		return;
	uint32_t s = 0;
	for (uint32_t k = 0; k < 16u; k++) {
		const uint32_t c = l.cnt[tid * 16u + k];
		l.cnt[tid * 16u + k] = s;
		s += c;
	}
	l.tot[tid] = s;
}

// (behind a barrier) the tile's total
LW_LANES_FN uint32_t lw_se_total(const LwSeLds &l)
{
	uint32_t s = 0;
	for (uint32_t k = 0; k < 16u; k++)
		s += l.tot[k];
	return s;
}

// ---- base and K: partial sums of the row's tile counts
LW_LANES_FN void lw_se_partial(const LwSelectArgs &a, const LwSeTile &t, LwSeLds &l, uint32_t tid)
{
	uint64_t before = 0, all = 0;
	for (uint32_t j = tid; j < t.n_tiles; j += LW_SE_THREADS) {
		const uint32_t c = a.tile_counts[t.list_at + j];
		all += c;
		if (j < t.tile_i)
			before += c;
	}
	l.part[tid] = before, l.part[LW_SE_THREADS + tid] = all;
}

// (behind a barrier) sixteen lanes fold sixteen partial sums each, of both kinds
LW_LANES_FN void lw_se_fold(LwSeLds &l, uint32_t tid)
{
	if (tid >= 32u)
		return;
	uint64_t s = 0;
	for (uint32_t k = 0; k < 16u; k++)
		s += l.part[tid * 16u + k];
	l.part[tid * 16u] = s;
}

// (behind a barrier) which = 0: base, 1: K
LW_LANES_FN uint64_t lw_se_sum(const LwSeLds &l, uint32_t which)
{
	uint64_t s = 0;
	for (uint32_t k = 0; k < 16u; k++)
		s += l.part[(which * 16u + k) * 16u];
	return s;
}

// ---- (behind lw_se_groups and a barrier) the places of the lane's kept frames into the compacted list
LW_LANES_FN void lw_se_places(const LwSelectArgs &a, const LwSeTile &t, const uint8_t *LW_LANES_RESTRICT mask, LwSeLds &l, uint32_t tid)
{
	const uint32_t per = a.tile / LW_SE_THREADS, lo = tid * per;
	uint32_t at = l.cnt[tid];
	for (uint32_t k = 0; k < tid / 16u; k++)
		at += l.tot[k];
	for (uint32_t k = 0; k < per && lo + k < t.nt; k++)
		if (mask[t.mask_at + t.t0 + lo + k] != 0)
			l.place[at++] = (uint16_t)(lo + k);
}

// ---- (behind a barrier) the copy of the tile's kept frames and the tile's share of the tail
LW_LANES_FN void lw_se_copy(const LwSelectArgs &a, const LwSeTile &t, const uint32_t *LW_LANES_RESTRICT src, uint32_t *LW_LANES_RESTRICT dst, const LwSeLds &l,
		uint64_t base, uint64_t K, uint32_t kept, uint32_t tid)
{
	const uint64_t end = t.t0 + a.tile < t.fill_end ? t.t0 + a.tile : t.fill_end;
	const uint64_t z0 = t.t0 > K ? t.t0 : K;
	for (uint32_t g = 0; g < t.G; g++) {
		const uint32_t *x = src + t.at + (uint64_t)g * a.line_el + t.t0;
		uint32_t *y = dst + t.at + (uint64_t)g * a.line_el;
		for (uint32_t j = tid; j < kept; j += LW_SE_THREADS)
			y[base + j] = x[l.place[j]];
		for (uint64_t p = z0 + tid; p < end; p += LW_SE_THREADS)
			y[p] = 0u;
	}
}

#ifndef LW_KERNEL_HOST

__global__ void __launch_bounds__(LW_SE_THREADS) k_select_count(LwSelectArgs a, const uint8_t *__restrict__ mask)
{
	__shared__ LwSeLds l;
	LwSeTile t;
	lw_se_tile(a, blockIdx.x, 0u, blockIdx.y, blockIdx.z, t);
	if (!t.nt)
		return; // (k_select reads the entries of tiles that hold frames only)
	lw_se_count(a, t, mask, l, threadIdx.x);
	__syncthreads();
	lw_se_groups(l, threadIdx.x);
	__syncthreads();
	if (threadIdx.x == 0)
		a.tile_counts[t.list_at + t.tile_i] = lw_se_total(l);
}

__global__ void __launch_bounds__(LW_SE_THREADS) k_select(LwSelectArgs a, const uint32_t *__restrict__ src, const uint8_t *__restrict__ mask,
		uint32_t *__restrict__ dst)
{
	__shared__ LwSeLds l;
	LwSeTile t;
	lw_se_tile(a, blockIdx.x / a.groups, blockIdx.x % a.groups, blockIdx.y, blockIdx.z, t);
	const bool counts = a.d_counts && t.tile_i == 0 && t.grp == 0;
	if (t.t0 >= t.fill_end && !counts)
		return;
	lw_se_partial(a, t, l, threadIdx.x);
	lw_se_count(a, t, mask, l, threadIdx.x);
	__syncthreads();
	lw_se_fold(l, threadIdx.x);
	lw_se_groups(l, threadIdx.x);
	__syncthreads();
	const uint64_t base = lw_se_sum(l, 0u), K = lw_se_sum(l, 1u);
	const uint32_t kept = lw_se_total(l);
	if (counts && threadIdx.x == 0)
		a.d_counts[t.cnt_at] = K;
	lw_se_places(a, t, mask, l, threadIdx.x);
	__syncthreads();
	lw_se_copy(a, t, src, dst, l, base, K, kept, threadIdx.x);
}

static bool lw_se_args_ok(const LwSelectArgs &a, uint32_t n_rows)
{
	return n_rows != 0 && n_rows <= 65535u && a.ch != 0 && a.ch <= 65535u && a.F != 0 && a.rows && a.tile_counts && lw_select_tile_ok(a.tile) &&
		a.tiles != 0 && a.groups == (a.F + LW_SE_LINES - 1u) / LW_SE_LINES && (uint64_t)a.tiles * a.groups <= LW_SE_MAX_TILES;
}

hipError_t lw_launch_select_count(const LwSelectArgs &a, const uint8_t *mask, uint32_t n_rows, hipStream_t st)
{
	if (!lw_se_args_ok(a, n_rows) || !mask)
		return hipErrorInvalidValue;
	return lw_launch_k(k_select_count, dim3(a.tiles, a.ch, n_rows), dim3(LW_SE_THREADS), 0, st, a, mask);
}

hipError_t lw_launch_select(const LwSelectArgs &a, const uint32_t *src, const uint8_t *mask, uint32_t *dst, uint32_t n_rows, hipStream_t st)
{
	if (!lw_se_args_ok(a, n_rows))
		return hipErrorInvalidValue;
	return lw_launch_k(k_select, dim3(a.tiles * a.groups, a.ch, n_rows), dim3(LW_SE_THREADS), 0, st, a, src, mask, dst);
}

#endif // LW_KERNEL_HOST
