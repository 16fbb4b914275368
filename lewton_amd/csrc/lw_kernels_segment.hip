// Speech segments from a frame mask (product code, gfx950): k_segment_count and k_segment, the kernels of lw_segment_rows.  A pass of
// its own from a uint8 mask [row][ch][frame_capacity] to the segments (a_k, b_k) of every row and channel, their count and the
// smoothed mask, by the rule of include/lewton_amd.h ("segments of a frame mask"): pad, fill short gaps, drop short runs.  Integer
// arithmetic only.  A workgroup of 256 lanes takes one tile of one row and channel and recomputes the rule for the tile and a halo of
// H + 1 frames either side, H = max(pad_onset, pad_offset) + min_off + min_on, so that neither the tile nor the grid reaches a bit:
//   load   the mask bytes of the window, frames outside [0, T) as 0, are __ballot words in LDS (a wave per word, round robin);
//   pad    P[t] = some m[u], t - pad_offset <= u <= t + pad_onset: one search over the words of m per frame, a ballot per word;
//   fill   C[t] = P[t], or the nearest set frames either side of t are fewer than min_off frames apart;
//   drop   O[t] = C[t] and the nearest unset frames either side of t are at least min_on frames apart;
//   edges  the starts O[t] & ~O[t - 1] and the last frames O[t] & ~O[t + 1] of the tile's own frames, two more word lists.
// Each pass is wrong within its own reach of a window edge that lies inside the line; the reaches add up to H, and the one frame
// more is what the edges look at.  TWO launches:
//   k_segment_count  the passes, then the popcount of the tile's starts goes to the scratch list tile_counts.
//   k_segment        the lanes add up the list's entries in front of the tile in 64 bits (base; the workgroup of tile 0 adds all of
//                    them: K, into d_counts), 256 partial sums folded in LDS.  An end belongs to the tile of its run's last frame, so the ends in
//                    front of a tile are the starts in front of it, minus one if a run crosses the tile's start (O[tile start - 1]
//                    and O[tile start] are both set).  The passes; then a lane takes the frames tid, tid + 256, ..: a
//                    start's rank in its tile is the popcount of the starts in front of it, likewise an end's, and the two
//                    halves of a span are stored where they belong; the smoothed bytes leave as k_vad's mask does, four at a
//                    4-byte boundary of the ADDRESS as one dword, byte by byte where the tile's start or end cuts a group.
// No atomics, no wait of a workgroup on another, offsets in 64 bits.  Nothing at or beyond T of the mask is read.
// tests/san/segment_host.cpp compiles this file for the host (LW_SEGMENT_HOST) and runs it workgroup by workgroup, the phases in the
// kernels' order.
#include "lw_segment.hpp"

#include "lw_lanes.hpp"
#ifndef LW_KERNEL_HOST
#include "lw_kernels.hpp"
#endif

static_assert(LW_SG_WAVES == LW_LANES_WAVES, "lw_lanes.hpp's loops count four waves to a workgroup");

struct LwSgLds { // the LDS of a workgroup
	uint64_t bits[2][LW_SG_WORDS]; // the passes alternate: bit j of a list is frame t0 - halo + j
	uint64_t starts[LW_SG_WORDS];  // of the tile's own frames
	uint64_t ends[LW_SG_WORDS];    // the last frames of runs, likewise
	uint64_t part[LW_SG_THREADS];  // partial sums of the tile counts
};
static_assert(sizeof(LwSgLds) == LW_SG_LDS, "LW_SG_LDS is the structure's size");

struct LwSgTile { // what a workgroup works on; the same for all its lanes
	uint64_t n, fill_end;
	uint64_t t0;      // first frame of the tile
	uint32_t nt;      // frames of the tile below T
	uint32_t tile_i;  // the tile's number in its row
	uint32_t n_tiles; // tiles of the row that hold frames: ceil(T / tile)
	uint32_t halo;    // H + 1
	uint32_t span;    // frames of the window: tile + 2 halo
	uint32_t words;   // ceil(span / 64)
	uint64_t mask_at; // byte of frame 0 of the row and channel in both masks
	uint64_t list_at; // entry of tile 0 of the row and channel in tile_counts
	uint64_t cnt_at;  // entry of the row and channel in d_counts; times seg_capacity: its first span
};

LW_LANES_FN void lw_sg_tile(const LwSegmentArgs &a, uint32_t tile_i, uint32_t by, uint32_t bz, LwSgTile &t)
{
	const uint64_t row = (uint64_t)a.row0 + bz;
	const LwSegmentRow r = a.rows[row];
	t.n = r.n, t.fill_end = r.fill_end, t.tile_i = tile_i;
	t.t0 = (uint64_t)tile_i * a.tile;
	const uint64_t end = t.t0 + a.tile;
	t.nt = t.t0 < r.n ? (uint32_t)((end < r.n ? end : r.n) - t.t0) : 0u;
	t.n_tiles = (uint32_t)((r.n + a.tile - 1u) / a.tile);
	t.halo = (a.pad_onset > a.pad_offset ? a.pad_onset : a.pad_offset) + a.min_off + a.min_on + 1u;
	t.span = a.tile + 2u * t.halo;
	t.words = (t.span + 63u) / 64u;
	t.mask_at = (row * a.ch + by) * a.line_el;
	t.list_at = ((uint64_t)bz * a.ch + by) * a.tiles;
	t.cnt_at = row * a.ch + by;
}

// what of a tile's work is owed (the same in every lane)
LW_LANES_FN bool lw_sg_owes_count(const LwSegmentArgs &a, const LwSgTile &t)
{
	return a.d_counts && t.tile_i == 0;
}
LW_LANES_FN bool lw_sg_owes_spans(const LwSegmentArgs &a, const LwSgTile &t)
{
	return a.d_spans && t.nt;
}
LW_LANES_FN bool lw_sg_owes_smooth(const LwSegmentArgs &a, const LwSgTile &t)
{
	return a.d_smooth && t.t0 < t.fill_end;
}
LW_LANES_FN bool lw_sg_passes(const LwSegmentArgs &a, const LwSgTile &t) // the rule is evaluated: the tile holds a frame somebody wants
{
	return t.nt && (a.d_spans || a.d_smooth);
}

// ---- the set bits of [lo, hi) of a word list, which may be empty (the searches: lw_lanes.hpp, in this file's index type)
LW_LANES_FN uint32_t lw_sg_count(const uint64_t *b, int32_t lo, int32_t hi)
{
	return lo < hi ? lw_bits_count<int32_t>(b, lo, hi, 0u) : 0u;
}

// ---- the passes: one wave's words of a list (lw_bits_fill).  decision(j, f) is asked for the bits of the window that are frames of the line
template <class P>
LW_LANES_FN void lw_sg_pass(const LwSgTile &t, uint64_t *out, uint32_t wave, uint32_t lane, P decision)
{
	lw_bits_fill(out, t.span, t.words, (int64_t)t.t0 - (int64_t)t.halo, t.n, wave, lane, decision);
}

LW_LANES_FN void lw_sg_load(const LwSegmentArgs &a, const LwSgTile &t, LwSgLds &l, uint32_t wave, uint32_t lane)
{
	lw_sg_pass(t, l.bits[0], wave, lane, [&](int32_t, uint64_t f) { return a.mask[t.mask_at + f] != 0; });
}

// (each behind a barrier) bits[0] -> bits[1] -> bits[0] -> bits[1]: O is bits[1]
LW_LANES_FN void lw_sg_pad(const LwSegmentArgs &a, const LwSgTile &t, LwSgLds &l, uint32_t wave, uint32_t lane)
{
	const uint64_t *m = l.bits[0];
	const int32_t span = (int32_t)t.span;
	lw_sg_pass(t, l.bits[1], wave, lane, [&](int32_t j, uint64_t) {
		const int32_t lo = j - (int32_t)a.pad_offset, hi = j + (int32_t)a.pad_onset + 1;
		return lw_bits_first<int32_t>(m, lo < 0 ? 0 : lo, hi > span ? span : hi, 0u) >= 0;
	});
}

LW_LANES_FN void lw_sg_fill(const LwSegmentArgs &a, const LwSgTile &t, LwSgLds &l, uint32_t wave, uint32_t lane)
{
	const uint64_t *p = l.bits[1];
	const int32_t span = (int32_t)t.span, reach = (int32_t)a.min_off;
	lw_sg_pass(t, l.bits[0], wave, lane, [&](int32_t j, uint64_t) {
		if (lw_bits_bit(p, j))
			return true;
		if (reach < 2)
			return false; // (a gap that holds t has a frame)
		const int32_t lo = j - reach + 1, hi = j + reach;
		const int32_t before = lw_bits_last<int32_t>(p, lo < 0 ? 0 : lo, j, 0u);
		if (before < 0)
			return false;
		const int32_t behind = lw_bits_first<int32_t>(p, j + 1, hi > span ? span : hi, 0u);
		return behind >= 0 && behind - before - 1 < reach;
	});
}

LW_LANES_FN void lw_sg_drop(const LwSegmentArgs &a, const LwSgTile &t, LwSgLds &l, uint32_t wave, uint32_t lane)
{
	const uint64_t *c = l.bits[0];
	const int32_t span = (int32_t)t.span, need = (int32_t)a.min_on;
	lw_sg_pass(t, l.bits[1], wave, lane, [&](int32_t j, uint64_t) {
		if (!lw_bits_bit(c, j))
			return false;
		if (need < 2)
			return true;
		// the nearest unset frames either side, as far as they matter: a side without one within need - 1 frames is long enough
		// by itself, and the window's edge counts as unset (it is, where it lies outside the line)
		const int32_t lo = j - need + 1, hi = j + need;
		int32_t before = lw_bits_last<int32_t>(c, lo < 0 ? 0 : lo, j, ~(uint64_t)0);
		if (before < 0)
			before = lo <= 0 ? -1 : lo - 1;
		int32_t behind = lw_bits_first<int32_t>(c, j + 1, hi > span ? span : hi, ~(uint64_t)0);
		if (behind < 0)
			behind = hi >= span ? span : hi;
		return behind - before - 1 >= need;
	});
}

LW_LANES_FN void lw_sg_edges(const LwSgTile &t, LwSgLds &l, uint32_t wave, uint32_t lane)
{
	const uint64_t *o = l.bits[1];
	const int32_t h = (int32_t)t.halo, end = h + (int32_t)t.nt;
	lw_sg_pass(t, l.starts, wave, lane, [&](int32_t j, uint64_t) { return j >= h && j < end && lw_bits_bit(o, j) && !lw_bits_bit(o, j - 1); });
	lw_sg_pass(t, l.ends, wave, lane, [&](int32_t j, uint64_t) { return j >= h && j < end && lw_bits_bit(o, j) && !lw_bits_bit(o, j + 1); });
}

// (behind a barrier) the tile's starts
LW_LANES_FN uint32_t lw_sg_starts(const LwSgTile &t, const LwSgLds &l)
{
	return lw_sg_count(l.starts, (int32_t)t.halo, (int32_t)(t.halo + t.nt));
}

// ---- base and K: partial sums of the row's tile counts -- those in front of the tile, all of them in tile 0
LW_LANES_FN void lw_sg_partial(const LwSegmentArgs &a, const LwSgTile &t, LwSgLds &l, uint32_t tid)
{
	const uint32_t lim = t.tile_i == 0 || t.tile_i > t.n_tiles ? t.n_tiles : t.tile_i;
	uint64_t s = 0;
	for (uint32_t j = tid; j < lim; j += LW_SG_THREADS)
		s += a.tile_counts[t.list_at + j];
	l.part[tid] = s;
}

// (behind a barrier) sixteen lanes fold sixteen partial sums each
LW_LANES_FN void lw_sg_fold(LwSgLds &l, uint32_t tid)
{
	if (tid >= 16u)
		return;
	uint64_t s = 0;
	for (uint32_t k = 0; k < 16u; k++)
		s += l.part[tid * 16u + k];
	l.part[tid * 16u] = s;
}

// (behind a barrier)
LW_LANES_FN uint64_t lw_sg_sum(const LwSgLds &l)
{
	uint64_t s = 0;
	for (uint32_t k = 0; k < 16u; k++)
		s += l.part[k * 16u];
	return s;
}

// ---- (behind the edges and a barrier) the lane's frames of the tile: the halves of the spans that lie in it
LW_LANES_FN void lw_sg_spans(const LwSegmentArgs &a, const LwSgTile &t, const LwSgLds &l, uint64_t base, uint32_t tid)
{
	const int32_t h = (int32_t)t.halo;
	// an end belongs to the tile of the run's last frame: a run that crosses the tile's start has started in front of it and ends here
	const uint64_t base_ends = base - (lw_bits_bit(l.bits[1], h - 1) && lw_bits_bit(l.bits[1], h) ? 1u : 0u);
	uint64_t *spans = a.d_spans + t.cnt_at * a.seg_capacity * 2u;
	for (uint32_t i = tid; i < t.nt; i += LW_SG_THREADS) {
		const int32_t j = h + (int32_t)i;
		if (lw_bits_bit(l.starts, j)) {
			const uint64_t k = base + lw_sg_count(l.starts, h, j);
			if (k < a.seg_capacity)
				spans[2u * k] = t.t0 + i;
		}
		if (lw_bits_bit(l.ends, j)) {
			const uint64_t k = base_ends + lw_sg_count(l.ends, h, j);
			if (k < a.seg_capacity)
				spans[2u * k + 1u] = t.t0 + i + 1u;
		}
	}
}

// ---- the lane's groups of four bytes of the tile's share of [0, fill_end) of the smoothed mask; passes: O is in LDS.  (The loop
// is lw_mask_write's, kept here: through that function the compiler no longer branches on `passes`, and k_segment's code changes.)
LW_LANES_FN void lw_sg_smooth(const LwSegmentArgs &a, const LwSgTile &t, const LwSgLds &l, bool passes, uint32_t tid)
{
	const uint64_t end = t.t0 + a.tile < t.fill_end ? t.t0 + a.tile : t.fill_end;
	if (t.t0 >= end)
		return;
	uint8_t *m = a.d_smooth + t.mask_at;
	const int64_t base = (int64_t)t.t0 - (int64_t)t.halo;
	const auto byte = [&](uint64_t f) { return passes && f < t.n && lw_bits_bit(l.bits[1], (int32_t)((int64_t)f - base)) ? 1u : 0u; };
	const uint32_t head = (uint32_t)((uintptr_t)(m + t.t0) & 3u);
	const uint32_t groups = (uint32_t)((end - t.t0 + head + 3u) / 4u);
	for (uint32_t g = tid; g < groups; g += LW_SG_THREADS) {
		const int64_t f0 = (int64_t)t.t0 - (int64_t)head + (int64_t)g * 4;
		if (f0 >= (int64_t)t.t0 && (uint64_t)f0 + 4u <= end) { // all four are the tile's: ONE dword
			uint32_t v = 0;
#pragma unroll
			for (uint32_t k = 0; k < 4u; k++)
				v |= byte((uint64_t)f0 + k) << (8u * k);
			*(uint32_t *)(m + f0) = v;
			continue;
		}
		for (int64_t f = f0; f < f0 + 4; f++) // the ragged head and tail of the span
			if (f >= (int64_t)t.t0 && (uint64_t)f < end)
				m[f] = (uint8_t)byte((uint64_t)f);
	}
}

#ifndef LW_KERNEL_HOST

// the passes of a workgroup, each behind the barrier of the one before; O and the edges are complete behind the last barrier
LW_LANES_FN void lw_sg_rule(const LwSegmentArgs &a, const LwSgTile &t, LwSgLds &l)
{
	const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
	lw_sg_load(a, t, l, wave, lane);
	__syncthreads();
	lw_sg_pad(a, t, l, wave, lane);
	__syncthreads();
	lw_sg_fill(a, t, l, wave, lane);
	__syncthreads();
	lw_sg_drop(a, t, l, wave, lane);
	__syncthreads();
	lw_sg_edges(t, l, wave, lane);
	__syncthreads();
}

__global__ void __launch_bounds__(LW_SG_THREADS) k_segment_count(LwSegmentArgs a)
{
	__shared__ LwSgLds l;
	LwSgTile t;
	lw_sg_tile(a, blockIdx.x, blockIdx.y, blockIdx.z, t);
	if (!t.nt)
		return; // (k_segment reads the entries of tiles that hold frames only)
	lw_sg_rule(a, t, l);
	if (threadIdx.x == 0)
		a.tile_counts[t.list_at + t.tile_i] = lw_sg_starts(t, l);
}

__global__ void __launch_bounds__(LW_SG_THREADS) k_segment(LwSegmentArgs a)
{
	__shared__ LwSgLds l;
	LwSgTile t;
	lw_sg_tile(a, blockIdx.x, blockIdx.y, blockIdx.z, t);
	const bool count = lw_sg_owes_count(a, t), spans = lw_sg_owes_spans(a, t), smooth = lw_sg_owes_smooth(a, t);
	if (!count && !spans && !smooth)
		return;
	uint64_t base = 0;
	if (count || spans) { // (the same in every lane)
		lw_sg_partial(a, t, l, threadIdx.x);
		__syncthreads();
		lw_sg_fold(l, threadIdx.x);
		__syncthreads();
		base = lw_sg_sum(l);
		if (count && threadIdx.x == 0)
			a.d_counts[t.cnt_at] = base;
		if (t.tile_i == 0)
			base = 0;
	}
	const bool passes = lw_sg_passes(a, t);
	if (passes)
		lw_sg_rule(a, t, l);
	if (spans)
		lw_sg_spans(a, t, l, base, threadIdx.x);
	if (smooth)
		lw_sg_smooth(a, t, l, passes, threadIdx.x);
}

static bool lw_sg_args_ok(const LwSegmentArgs &a, uint32_t n_rows)
{
	return n_rows != 0 && n_rows <= 65535u && a.ch != 0 && a.ch <= 65535u && a.rows && a.tile_counts && lw_segment_tile_ok(a.tile) && a.tiles != 0 &&
		a.tiles <= LW_SG_MAX_TILES && a.pad_onset <= LW_SG_MAX_SPAN && a.pad_offset <= LW_SG_MAX_SPAN && a.min_off <= LW_SG_MAX_SPAN &&
		a.min_on <= LW_SG_MAX_SPAN && (!a.d_spans || a.seg_capacity);
}

hipError_t lw_launch_segment_count(const LwSegmentArgs &a, uint32_t n_rows, hipStream_t st)
{
	if (!lw_sg_args_ok(a, n_rows) || !a.mask)
		return hipErrorInvalidValue;
	return lw_launch_k(k_segment_count, dim3(a.tiles, a.ch, n_rows), dim3(LW_SG_THREADS), 0, st, a);
}

hipError_t lw_launch_segment(const LwSegmentArgs &a, uint32_t n_rows, hipStream_t st)
{
	if (!lw_sg_args_ok(a, n_rows) || (!a.d_spans && !a.d_counts && !a.d_smooth))
		return hipErrorInvalidValue;
	return lw_launch_k(k_segment, dim3(a.tiles, a.ch, n_rows), dim3(LW_SG_THREADS), 0, st, a);
}

#endif // LW_KERNEL_HOST
