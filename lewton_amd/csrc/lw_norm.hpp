// Normalising rows (lw_norm_*, include/lewton_amd.h "normalising rows"): what lw_norm.cpp (the host side) and lw_kernels_norm.hip
// (k_norm_sum, k_norm_fold, k_norm_apply) share -- the contract's scalars and its apply step (ONE source for the host's
// lw_norm_scalars and the kernels, double arithmetic only), the chunk triple and its pair tree's zero, the kernels' arguments, the
// per-row records and the plan.  Kept out of lw_kernels.hpp: no other translation unit sees it.
#pragma once

#include "lw_lanes.hpp"

// ---- steps 3 and 4 of the contract.  Every operation below is one IEEE double operation: the units that include this are
// compiled with -ffp-contract=off.  `scale` is LW_NORM_SCALE_* (0 none, 1 std, 2 rms, 3 peak); peak is |x| of the scope's largest
// bit pattern.  sqrt: the host's is correctly rounded; the device's expansion (an rsq estimate refined with fma, which gfx950 has in
// place of a correctly rounded instruction) gave the host's bits on all of 2^24 doubles it was compared on, and the GPU suite
// compares (m, g) of a million scopes with numpy: no correction step is needed here (DESIGN 3.19 says where one would go).
LW_LANES_HD void lw_norm_scalars_value(int center, int scale, double eps, double target, double S1, double S2, float peak, uint64_t N, double &m,
		double &g)
{
	m = 0.0, g = 1.0;
	if (N == 0)
		return;
	const double dn = (double)N;
	const double mu = S1 / dn, q = S2 / dn;
	double v = q - mu * mu;
	if (!(v > 0.0))
		v = 0.0;
	if (center)
		m = mu;
	if (scale == 1)
		g = 1.0 / __builtin_sqrt(v + eps);
	else if (scale == 2)
		g = target / __builtin_sqrt(q + eps);
	else if (scale == 3)
		g = peak == 0.0f ? 1.0 : target / (double)peak;
}

LW_LANES_HD float lw_norm_apply_value(float x, double m, double g)
{
	const double c = (double)x - m;
	return (float)(c * g);
}

// ---- a chunk's triple, and a list entry: the two sums and the bit pattern of the largest |x|
struct LwNormTriple {
	double s1, s2;
	uint32_t pk, pad_;
};
static_assert(sizeof(LwNormTriple) == 24, "LwNormTriple is stored as three 8-byte words");

LW_LANES_HD LwNormTriple lw_wave_add(const LwNormTriple &a, const LwNormTriple &b) // (lw_wave_tree's addition)
{
	return LwNormTriple{a.s1 + b.s1, a.s2 + b.s2, a.pk > b.pk ? a.pk : b.pk, 0u};
}

// One row of a call.
struct LwNormRow {
	uint64_t n;        // [0, n) of every line is read and normalised
	uint64_t fill_end; // max(n, fill_to): [n, fill_end) receives +0.0
	uint64_t part_at;  // the row's chunk list in the partials: lines * chunks triples, line-major
	uint32_t chunks;   // C = ceil(n / 256)
	uint32_t pad_;
};
static_assert(sizeof(LwNormRow) == 32, "LwNormRow is read as eight dwords");

#define LW_NM_THREADS 256u
#define LW_NM_WAVES 4u
#define LW_NM_MAX_TILES 2048u // workgroups per row the plans aim at

// The plan.  k_norm_sum: lw_sum_plan over the chunk slots of all lines of a row (a row with fewer chunks leaves its other slots
// alone).  k_norm_fold: one scope per wave (fold_wave, every list of the call has at most 64 entries) or per workgroup, which then
// keeps the lists of its levels in fold_scratch triples of its own.  k_norm_apply: runs of four, lw_run_plan.
struct LwNormPlan {
	uint32_t sum_chunks;   // ceil(largest n / 256)
	uint32_t sum_per_wave; // slots a wave takes
	uint32_t sum_tiles;    // workgroups per row
	uint32_t scopes;       // per row: 1, ch or ch * F
	uint32_t scope_lines;  // lines per scope: ch * F, F or 1
	uint32_t fold_wave;    // 1: a wave per scope
	uint64_t fold_scratch; // triples per scope (0 under fold_wave)
	uint32_t runs_per_line; // apply, a LwRunPlan's four: ceil((span + 3) / 256), at least 1
	uint32_t runs;          // per channel: F * runs_per_line
	uint32_t per_wave;      // runs a wave takes
	uint32_t tiles;         // per channel
};

// false: a chunk list, or a channel's runs, that 32 bits cannot count
static inline bool lw_norm_plan(uint32_t ch, uint32_t F, int scope, uint64_t most, uint64_t span, LwNormPlan &p)
{
	const uint64_t lines = (uint64_t)ch * F;
	p.scope_lines = scope == 0 ? (uint32_t)lines : scope == 1 ? F : 1u;
	p.scopes = (uint32_t)(lines / p.scope_lines);
	LwSumPlan s;
	LwRunPlan r;
	if (!lw_sum_plan(most, lines, p.scope_lines, LW_NM_MAX_TILES, s) || !lw_run_plan(ch, F, span, LW_NM_MAX_TILES, r))
		return false;
	p.runs_per_line = r.runs_per_line, p.runs = r.runs, p.per_wave = r.per_wave, p.tiles = r.tiles;
	p.sum_chunks = s.chunks, p.sum_per_wave = s.per_wave, p.sum_tiles = s.tiles;
	p.fold_wave = s.longest <= LW_SUM_GROUP;
	p.fold_scratch = p.fold_wave ? 0u : s.fold_scratch;
	return true;
}

struct LwNormArgs {
	const float *src;
	float *dst;
	LwNormTriple *part;    // the rows' chunk lists (k_norm_sum -> k_norm_fold)
	LwNormTriple *scratch; // [row of the call][scope][fold_scratch]: the lists of the workgroup fold's levels
	double *sc;            // [row of the call][scope][2]: m, g (k_norm_fold -> k_norm_apply)
	double *d_stats;       // NULL, or the caller's copy of sc
	const LwNormRow *rows;
	uint64_t line_el; // capacity: elements per line; a channel is F lines, a row ch channels
	uint32_t ch, F;
	LwNormPlan plan;
	uint32_t row0; // first row of this launch (blockIdx.z counts from it)
	int32_t center, scale, scope;
	uint32_t plain; // center = 0, no scale: m = +0.0, g = 1.0 for every scope, nothing is summed
	double eps, target;
};

// k_norm_sum:   grid = (sum_tiles, 1, rows of this launch <= 65535)
// k_norm_fold:  grid = (ceil(scopes / 4) under fold_wave, else scopes, 1, rows of this launch)
// k_norm_apply: grid = (tiles per channel, channels, rows of this launch).  Nothing outside [0, fill_end) of a line is written.
hipError_t lw_launch_norm_sum(const LwNormArgs &a, uint32_t n_rows, hipStream_t st);
hipError_t lw_launch_norm_fold(const LwNormArgs &a, uint32_t n_rows, hipStream_t st);
hipError_t lw_launch_norm_apply(const LwNormArgs &a, uint32_t n_rows, hipStream_t st);
