// Sliding-window normalisation of feature rows (lw_slide_*, include/lewton_amd.h "sliding-window normalisation of feature rows"):
// what lw_slide.cpp (the host side) and lw_kernels_slide.hip (k_slide) share -- the window rule in signed 64-bit integers and the
// scalar step from the window's sums to the output value (ONE source for the kernel, its host build, lw_slide_window and the
// host model of the tests; double arithmetic only, the units are compiled with -ffp-contract=off), the per-row record, the tile
// plan, the kernel's arguments and the launcher.  Kept out of lw_kernels.hpp: no other translation unit sees it.
#pragma once

#include "lw_lanes.hpp"

#define LW_SL_THREADS 256u        // a workgroup
#define LW_SL_BLOCK 16u           // frames of a block sum (rule 2)
#define LW_SL_MAX_WINDOW 2048u    // LW_SLIDE_MAX_WINDOW
#define LW_SL_TILE 1024u          // frames a workgroup owns unless a test says otherwise
#define LW_SL_MIN_TILE 16u        // lw_slide_set_tile_frames: a multiple of 16 in MIN .. MAX
#define LW_SL_MAX_TILE 4096u
#define LW_SL_MAX_LINES 16u       // lines a workgroup stages at a time
#define LW_SL_LDS_BUDGET 65536u   // bytes of LDS a workgroup may plan with: two workgroups to a compute unit of 160 KiB
#define LW_SL_MAX_TILES 0xffffffu // workgroups in a grid's first dimension: tiles * line groups * 256 lanes stays below 2^32

// ---- rule 1: the window [s, e) of frame t of a line of T frames (t < T)
LW_LANES_HD void lw_slide_window_value(uint32_t W, uint32_t min_window, int center, uint64_t t, uint64_t T, int64_t &s, int64_t &e)
{
	const int64_t it = (int64_t)t, iT = (int64_t)T;
	if (center) {
		s = it - (int64_t)(W / 2u);
		e = s + (int64_t)W;
	} else {
		s = it - (int64_t)W;
		e = it + 1;
	}
	if (s < 0) {
		e -= s;
		s = 0;
	}
	if (!center && e > it)
		e = it + 1 > (int64_t)min_window ? it + 1 : (int64_t)min_window;
	if (e > iT) {
		s -= e - iT;
		e = iT;
		if (s < 0)
			s = 0;
	}
}

// ---- rule 4: from the window's sums to the output value.  Every operation is one IEEE double operation.  sqrt: as lw_norm.hpp
// says of the device's expansion.
LW_LANES_HD float lw_slide_value(int norm_vars, float x, double S, double Q, uint64_t n)
{
	const double dn = (double)n;
	const double mu = S / dn;
	const double c = (double)x - mu;
	if (!norm_vars)
		return (float)c;
	if (n == 1)
		return 0.0f;
	double v = Q / dn - mu * mu;
	if (!(v > 1e-10))
		v = 1e-10;
	const double g = 1.0 / __builtin_sqrt(v);
	return (float)(c * g);
}

// One row of a call.
struct LwSlideRow {
	uint64_t n;        // T: frames [0, n) of every line are read and normalised
	uint64_t fill_end; // max(T, fill_to): [T, fill_end) receives +0.0
};
static_assert(sizeof(LwSlideRow) == 16, "LwSlideRow is read as four dwords");

// The tile plan.  A workgroup owns `tile` consecutive frames of `lines` feature lines of one row and channel.  The windows of its
// frames are nested steps -- s and e of rule 1 never decrease with t and s grows by at most one a frame -- so they lie in
// [s(first frame), e(last frame)), at most tile + W frames; the image starts at s rounded DOWN to a block boundary so that the
// image's blocks are the line's: `cols` = tile + W + 15 rounded up to 16.  Per line the image holds cols floats, element i at
// dword i + i / 32 (the skew takes the lanes of the block pass, 16 floats apart, to 32 different banks), and cols / 16 pairs of
// doubles (A_b, Q_b) in front of the floats.  lines = min(F, 16, budget / bytes per line), rounded down to a multiple of four from four
// on: 8 at W = 300, 4 at W = 600 and at W = 2048 with the default tile.
// The bits depend on none of this.
struct LwSlidePlan {
	uint32_t tile;  // frames a workgroup owns: a multiple of 16
	uint32_t cols;  // the most frames of a line the image holds
	uint32_t pitch; // dwords per line of the image's floats
	uint32_t nb;    // block sums per line: cols / 16
	uint32_t lines; // lines of the image
	uint32_t lds;   // bytes of LDS a workgroup needs
};

// false: a tile that is no multiple of 16 in LW_SL_MIN_TILE .. LW_SL_MAX_TILE
static inline bool lw_slide_plan(uint32_t F, uint32_t W, uint32_t tile, LwSlidePlan &p)
{
	if (tile < LW_SL_MIN_TILE || tile > LW_SL_MAX_TILE || tile % LW_SL_BLOCK)
		return false;
	p.tile = tile;
	p.cols = (tile + W + 2u * LW_SL_BLOCK - 2u) & ~(LW_SL_BLOCK - 1u);
	p.pitch = p.cols + p.cols / 32u + 1u;
	p.nb = p.cols / LW_SL_BLOCK;
	const uint32_t per_line = p.pitch * 4u + p.nb * 16u; // (at most 31 656: two lines always fit)
	uint32_t lines = LW_SL_LDS_BUDGET / per_line;
	lines = lines > LW_SL_MAX_LINES ? LW_SL_MAX_LINES : lines;
	lines = lines >= 4u ? lines & ~3u : lines; // the apply phase runs four lines side by side
	p.lines = lines > F ? F : lines;
	p.lds = p.lines * per_line;
	return true;
}

struct LwSlideArgs {
	const LwSlideRow *rows;
	uint64_t line_el; // frame_capacity: elements per line
	uint32_t ch, F, W, min_window;
	int32_t center, norm_vars;
	uint32_t groups; // line groups of a channel: ceil(F / plan.lines); blockIdx.x = tile * groups + group
	uint32_t row0;   // first row of this launch (blockIdx.z counts from it)
	LwSlidePlan plan;
};

// k_slide: grid = (tiles of the longest fill_end * groups, channels, rows of this launch <= 65535)
hipError_t lw_launch_slide(const LwSlideArgs &a, const float *src, float *dst, uint32_t tiles, uint32_t n_rows, hipStream_t st);
