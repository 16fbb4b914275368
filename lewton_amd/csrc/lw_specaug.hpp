// SpecAugment masks (lw_specaug_*, include/lewton_amd.h "masking feature rows"): what lw_specaug.cpp (the host side) and
// lw_kernels_specaug.hip (k_specaug) share -- the span rule of the contract (ONE source for the host's lw_specaug_plan and the
// kernel, on lw_rng.hpp), the per-row record, the kernel's arguments and the launcher.  Kept out of lw_kernels.hpp: no other
// translation unit sees it.
#pragma once

#include "lw_lanes.hpp"
#include "lw_rng.hpp"

#define LW_SA_THREADS 256u        // a workgroup
#define LW_SA_TILE 2048u          // frames of a tile unless a test says otherwise: a multiple of 256 in 256 .. 2048
#define LW_SA_MAX_TILE 2048u
#define LW_SA_MAX_MASKS 32u       // LW_SPECAUG_MAX_MASKS, per kind
#define LW_SA_MAX_WIDTH 65535u    // LW_SPECAUG_MAX_WIDTH
#define LW_SA_MAX_TILES 0xffffffu // workgroups in a grid's first dimension (tiles * F): times 256 lanes it stays below 2^32
#define LW_SA_TIME 0u             // the kinds: counter word 3
#define LW_SA_FREQ 1u
// LDS of k_specaug, static: (start, end) of the group's masks, time masks first
#define LW_SA_LDS (2u * LW_SA_MAX_MASKS * 2u * 8u)

// what of lw_specaug_params the rule takes
struct LwSaRule {
	uint64_t seed;
	uint32_t num_t, min_t, max_t, ratio_num, ratio_den;
	uint32_t num_f, min_f, max_f;
};

// ---- the rule: mask k of kind d of group g of the utterance `id` over n frames (d == LW_SA_TIME) or bins -> [start, end).  All
// of it in unsigned 64-bit integers; n is at most 2^63 (a row's frames are far below: its bytes are addressable), so n - w + 1
// does not wrap.  The width is drawn first and the start over what the width leaves: the mask lies wholly inside [0, n)
LW_LANES_HD void lw_sa_span(const LwSaRule &p, uint64_t id, uint32_t g, uint32_t d, uint32_t k, uint64_t n, uint64_t &start, uint64_t &end)
{
	const uint32_t c[4] = {(uint32_t)id, (uint32_t)(id >> 32), k | g << 16, d}, key[2] = {(uint32_t)p.seed, (uint32_t)(p.seed >> 32)};
	uint32_t x[4];
	lw_philox(c, key, x);
	const uint64_t max_d = d == LW_SA_TIME ? p.max_t : p.max_f, min_d = d == LW_SA_TIME ? p.min_t : p.min_f;
	uint64_t W = max_d < n ? max_d : n;
	if (d == LW_SA_TIME && p.ratio_den != 0) {
		const uint64_t r = (n / p.ratio_den) * p.ratio_num + ((n % p.ratio_den) * p.ratio_num) / p.ratio_den;
		W = W < r ? W : r;
	}
	const uint64_t lo = min_d < W ? min_d : W;
	const uint64_t w = lo + lw_below32(x[0], (uint32_t)(W - lo + 1u)); // (W <= 65535: the count of widths fits 32 bits)
	start = lw_below64((uint64_t)x[1] << 32 | x[2], n - w + 1u);
	end = start + w;
}

// One row of a call.
struct LwSaRow {
	uint64_t n;        // T: frames [0, n) of every line may be read
	uint64_t fill_end; // max(T, fill_to): positions [T, fill_end) of every line receive +0.0
	uint64_t id;       // the utterance: ids[row], or the row's index
	uint64_t pad_;
};
static_assert(sizeof(LwSaRow) == 32, "LwSaRow is read as eight dwords");

struct LwSaArgs {
	const uint32_t *src; // the elements as their bits: both sides of the select are bit copies
	uint32_t *dst;       // == src: the call in place
	int64_t *spans;      // NULL, or [row of the call][G][num_t + num_f][2]
	const LwSaRow *rows;
	uint64_t line_el;    // frame_capacity: elements per line
	LwSaRule rule;
	uint32_t ch, F;
	uint32_t tile, tiles; // frames of a tile; tiles of the longest fill_end (at least 1 where spans are owed)
	uint32_t row0;        // first row of this launch (blockIdx.z counts from it)
	uint32_t per_channel;
	uint32_t fill;        // the bits of lw_specaug_params.fill
};

static inline bool lw_sa_tile_ok(uint32_t tile)
{
	return tile >= LW_SA_THREADS && tile <= LW_SA_MAX_TILE && tile % LW_SA_THREADS == 0;
}

// k_specaug: grid = (tiles * F, channels, rows of this launch <= 65535): workgroup x is tile x % tiles of line x / tiles
hipError_t lw_launch_specaug(const LwSaArgs &a, uint32_t n_rows, hipStream_t st);
