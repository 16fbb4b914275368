// Cepstra and deltas of feature rows (lw_cep_*, include/lewton_amd.h "cepstra and deltas of feature rows"): what lw_cep.cpp (the
// host side) and lw_kernels_cep.hip (k_cep) share -- the delta step (ONE source for the kernel and any host-side use), the delta
// weights, the per-row record, the tile plan, the kernel's arguments and the launcher.  Kept out of lw_kernels.hpp: no other
// translation unit sees it.
#pragma once

#include "lw_lanes.hpp"

#define LW_CP_THREADS 256u  // a workgroup: one frame per lane, halo included
#define LW_CP_GROUP 32u     // output lines (accumulators) a lane carries at a time
#define LW_CP_MAX_WIDTH 16u // LW_CEP_MAX_WIDTH
#define LW_CP_MAX_TILES 0xffffffu // tiles of a launch: tiles * 256 lanes stays below 2^32, the most a grid dimension holds in lanes

// ---- the contract's delta step: acc = fmaf(w_n, after - before, acc).  The subtraction is one rounded f32 operation of its own
// (the units that include this are compiled with -ffp-contract=off, and fmaf is asked for by name).
LW_LANES_HD float lw_cep_delta_step(float w, float after, float before, float acc)
{
	const float d = after - before;
	return __builtin_fmaf(w, d, acc);
}

// c(i) = min(max(i, 0), n - 1) in signed 64-bit integers (n >= 1)
LW_LANES_HD int64_t lw_cep_clamp(int64_t i, int64_t n)
{
	return i < 0 ? 0 : i >= n ? n - 1 : i;
}

// w_n = (float)((double)n / (double)D), D = 2 (1^2 + .. + N^2): one double division, one rounding.  Host only: the kernel gets
// the weights as arguments and divides nothing.
static inline void lw_cep_weights(uint32_t N, float *w)
{
	uint64_t D = 0;
	for (uint64_t n = 1; n <= N; n++)
		D += 2u * n * n;
	for (uint32_t n = 1; n <= N; n++)
		w[n - 1] = (float)((double)n / (double)D);
}

// One row of a call.
struct LwCepRow {
	uint64_t n;        // frames [0, n) of every source line are read, of every destination line computed
	uint64_t fill_end; // max(n, fill_to): [n, fill_end) of every destination line receives +0.0
};
static_assert(sizeof(LwCepRow) == 16, "LwCepRow is read as four dwords");

// The tile plan.  A workgroup of 256 lanes produces `tile` consecutive frames of every destination line of one row and channel.
// Lane i stands on frame t0 - halo + i, clamped into the row (halo = order * width): it carries that frame's statics, the lanes
// `width` and more from either end also its deltas, the lanes `halo` and more from either end -- the tile -- its delta-deltas.
// So tile = 256 - 2 halo: 256 without deltas, 248 at order 2 and width 2 (3 % of the static chains are the halo's), 192 at
// order 2 and width 16.  The bits depend on none of this.
struct LwCepPlan {
	uint32_t halo;  // order * width
	uint32_t tile;  // frames a workgroup produces
	uint32_t group; // accumulators per lane: min(32, n_out rounded up to 8)
	uint32_t lds;   // bytes of LDS a workgroup needs: an image of group * 256 floats per delta level
};

static inline LwCepPlan lw_cep_plan(uint32_t n_out, uint32_t order, uint32_t width)
{
	LwCepPlan p;
	p.halo = order * width;
	p.tile = LW_CP_THREADS - 2u * p.halo;
	const uint32_t up = (n_out + 7u) & ~7u;
	p.group = up < LW_CP_GROUP ? up : LW_CP_GROUP;
	p.lds = order * p.group * LW_CP_THREADS * (uint32_t)sizeof(float);
	return p;
}

struct LwCepArgs {
	const LwCepRow *rows;
	uint64_t line_el; // frame_capacity: elements per line; a source channel is n_in lines, a destination channel n_out * (1 + order)
	uint32_t ch, n_in, n_out, order, width;
	uint32_t identity; // no matrix: the static lines are a bit copy (n_out == n_in)
	uint32_t mt_stride; // floats per row of the transposed matrix: n_out rounded up to 32
	uint32_t row0;      // first row of this launch (blockIdx.z counts from it)
	LwCepPlan plan;
	float w[LW_CP_MAX_WIDTH]; // w_1 .. w_N
};

// k_cep: grid = (tiles of the longest fill_end, channels, rows of this launch <= 65535).  mt: the matrix TRANSPOSED and padded
// with +0.0, [n_in][mt_stride] (what 32 consecutive outputs need of one input is contiguous); NULL for the identity.  Nothing
// outside [0, fill_end) of a destination line is written, nothing at or beyond n of a source line read.
hipError_t lw_launch_cep(const LwCepArgs &a, const float *mt, const float *src, float *dst, uint32_t tiles, uint32_t n_rows, hipStream_t st);
