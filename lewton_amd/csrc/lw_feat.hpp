// Finishing feature rows (lw_feat_*, include/lewton_amd.h "finishing feature rows"): what lw_feat.cpp (the host side) and
// lw_kernels_feat.hip (k_feat_log, k_feat_fin) share -- the contract's LOG itself (one source for the host's lw_feat_log and the
// kernel, double arithmetic only), the kernels' arguments, the per-row records and the tile plan.  Kept out of lw_kernels.hpp: no
// other translation unit sees it.
#pragma once

#include "lw_lanes.hpp"

// ---- LOG (step 2 of the contract).  Every operation below is one IEEE double operation: the units that include this are compiled
// with -ffp-contract=off, the quotients c_k are folded by the compiler, correctly rounded.  `kind` is LW_FEAT_LOG_*.
LW_LANES_HD float lw_feat_log_value(int kind, float v)
{
	if (kind == 0 || v == __builtin_inff())
		return v;
	int e;
	double m = __builtin_frexp((double)v, &e);
	if (m < 0x1.6a09e667f3bcdp-1) {
		m = m * 2.0;
		e = e - 1;
	}
	const double s = (m - 1.0) / (m + 1.0), z = s * s;
	double p = 1.0 / 19.0;
	p = p * z + 1.0 / 17.0;
	p = p * z + 1.0 / 15.0;
	p = p * z + 1.0 / 13.0;
	p = p * z + 1.0 / 11.0;
	p = p * z + 1.0 / 9.0;
	p = p * z + 1.0 / 7.0;
	p = p * z + 1.0 / 5.0;
	p = p * z + 1.0 / 3.0;
	p = p * z + 1.0;
	double r = (double)e * 0x1.62e42fefa39efp-1 + (s + s) * p;
	if (kind >= 2)
		r = r * 0x1.bcb7b1526e50ep-2;
	if (kind == 3)
		r = r * 10.0;
	return (float)r;
}

// ---- the maximum in the total order of the non-NaN floats (+0.0 above -0.0): a float's bits as a signed integer, the negative
// half reversed, compare as integers
LW_LANES_HD int32_t lw_ft_key(float f)
{
	const int32_t i = __builtin_bit_cast(int32_t, f);
	return i < 0 ? i ^ 0x7fffffff : i;
}
LW_LANES_HD float lw_ft_unkey(int32_t k)
{
	return __builtin_bit_cast(float, k < 0 ? k ^ 0x7fffffff : k);
}
#define LW_FT_KEY_LOWEST ((int32_t)0x807fffff) // the key of -inf: below every l

// One row of a call.
struct LwFeatRow {
	uint64_t n_frames; // [0, n_frames) of every line is read and finished
	uint64_t fill_end; // max(n_frames, fill_to): [n_frames, fill_end) receives the fill value
};
static_assert(sizeof(LwFeatRow) == 16, "LwFeatRow is read as four dwords");

// The tile plan: runs of four (lw_lanes.hpp), so all of a tile lies in one scope, and a scope of a row has at most about
// LW_FT_MAX_TILES tiles, whose maxima the second launch reads again.
#define LW_FT_THREADS 256u
#define LW_FT_WAVES 4u
#define LW_FT_MAX_TILES 1024u // tiles per row the plan aims at (a channel has at least one)

typedef LwRunPlan LwFeatPlan;

// false: more runs in a channel than 32 bits count
static inline bool lw_feat_plan(uint32_t ch, uint32_t F, uint64_t span, LwFeatPlan &p)
{
	return lw_run_plan(ch, F, span, LW_FT_MAX_TILES, p);
}

struct LwFeatArgs {
	const float *src;
	float *dst;
	float *part;  // [row of the call][ch][tiles]: the tiles' maxima (first launch -> second launch)
	float *d_max; // NULL, [row] or [row][ch]
	const LwFeatRow *rows;
	uint64_t line_el; // frame_capacity: elements per line; a channel is F lines, a row ch channels
	uint32_t ch, F;
	LwFeatPlan plan;
	uint32_t row0; // first row of this launch (blockIdx.z counts from it)
	int32_t log, scope;
	float floor, top, add, mul;
	float l0;       // LOG(floor)
	uint32_t final; // the first launch is the only one: it stores z, and fills
};

// grid = (tiles per channel, channels, rows of this launch <= 65535).  Nothing outside [0, fill_end) of a line is written.
hipError_t lw_launch_feat_log(const LwFeatArgs &a, uint32_t n_rows, hipStream_t st);
hipError_t lw_launch_feat_fin(const LwFeatArgs &a, uint32_t n_rows, hipStream_t st);
