// Energy voice-activity decisions (lw_vad_*, include/lewton_amd.h "energy voice-activity decisions of feature rows"): what
// lw_vad.cpp (the host side) and lw_kernels_vad.hip (k_vad, k_vad_sum, k_vad_fold, k_vad_decide, k_vad_fill) share -- rules 1 and 3
// of the contract (ONE source for the host's lw_vad_threshold / lw_vad_voiced and the kernels), the chunk sum of "normalising
// rows" restated for one line, the per-row record, the plan, the kernels' arguments and the launchers.  Kept out of lw_kernels.hpp:
// no other translation unit sees it.
#pragma once

#include "lw_lanes.hpp"

#define LW_VD_THREADS 256u        // a workgroup
#define LW_VD_WAVES 4u
#define LW_VD_CHUNK LW_SUM_CHUNK   // frames per chunk of the sum: the one of "normalising rows"
#define LW_VD_TILE 1024u          // frames of a tile unless a test says otherwise: a multiple of 256 in 256 .. 2048
#define LW_VD_MAX_TILE 2048u
#define LW_VD_MAX_CONTEXT 256u    // LW_VAD_MAX_CONTEXT
#define LW_VD_FUSED_MAX 16384u    // LW_VAD_FUSED_MAX: 64 chunks, ONE tree over the chunk list
#define LW_VD_MAX_TILES 0xffffffu // workgroups in a grid's first dimension: tiles * 256 lanes stays below 2^32
#define LW_VD_SUM_TILES 2048u     // workgroups per row and channel k_vad_sum's plan aims at
#define LW_VD_WORDS ((LW_VD_MAX_TILE + 2u * LW_VD_MAX_CONTEXT) / 64u) // ballot words of a tile and its context either side
// LDS of k_vad, static: 64 chunk sums + the raw decisions of the tile and its context
#define LW_VD_LDS (LW_SUM_GROUP * 8u + LW_VD_WORDS * 8u)

// ---- rule 1, behind the sum.  Every operation is ONE IEEE f32 operation: the units that include this are compiled with
// -ffp-contract=off.  (float)T is the round-to-nearest-even conversion of the uint64.
LW_LANES_HD float lw_vad_threshold_value(float energy_threshold, float energy_mean_scale, double S, uint64_t T)
{
	if (energy_mean_scale == 0.0f || T == 0)
		return energy_threshold;
	const float sf = (float)S;
	const float p = energy_mean_scale * sf;
	const float q = p / (float)T;
	return energy_threshold + q;
}

// ---- rule 3: ONE rounded f32 multiply, as Kaldi's int * BaseFloat
LW_LANES_HD bool lw_vad_voiced_value(uint64_t num, uint64_t den, float proportion_threshold)
{
	const float need = (float)den * proportion_threshold;
	return (float)num >= need;
}

// One row of a call.
struct LwVadRow {
	uint64_t n;        // T: frames [0, n) of the energy line may be read
	uint64_t fill_end; // max(T, fill_to): mask positions [T, fill_end) receive 0
	uint64_t list_at;  // split form: the row's chunk sums in the list, [ch][chunks] doubles
	uint32_t chunks;   // C = ceil(T / 256)
	uint32_t pad_;
};
static_assert(sizeof(LwVadRow) == 32, "LwVadRow is read as eight dwords");

struct LwVadArgs {
	const float *src;
	uint8_t *mask;
	float *d_thr;    // NULL, or [n_rows][ch]
	double *part;    // split form: the rows' chunk lists (k_vad_sum -> k_vad_fold)
	double *scratch; // split form: [row of the call][ch][fold_scratch], the lists of the fold's levels
	float *thr;      // split form: [row of the call][ch] (k_vad_fold -> k_vad_decide); NULL: k_vad_decide takes energy_threshold
	const LwVadRow *rows;
	uint64_t line_el;      // frame_capacity: elements per line, and per (row, channel) of the mask
	uint64_t fold_scratch; // doubles per row and channel
	uint32_t ch, F, line;
	uint32_t tile, tiles;  // frames of a tile; tiles of the longest fill_end
	uint32_t ctx;          // frames_context
	uint32_t sum_chunks;   // split form: ceil(largest T / 256)
	uint32_t sum_per_wave; // chunks a wave of k_vad_sum takes
	uint32_t sum_tiles;    // workgroups of k_vad_sum per row and channel
	uint32_t row0;         // first row of this launch (blockIdx.z counts from it)
	uint32_t thr_out;      // k_vad_decide: the workgroup of tile 0 stores the threshold into d_thr (no fold has)
	float energy_threshold, energy_mean_scale, proportion_threshold;
};

static inline bool lw_vad_tile_ok(uint32_t tile)
{
	return tile >= LW_VD_THREADS && tile <= LW_VD_MAX_TILE && tile % LW_VD_THREADS == 0;
}

// k_vad_sum's plan from the call's longest row: false where 32 bits cannot count the chunks
static inline bool lw_vad_sum_plan(uint64_t most, LwVadArgs &a)
{
	LwSumPlan s;
	if (!lw_sum_plan(most, 1u, 1u, LW_VD_SUM_TILES, s))
		return false;
	a.sum_chunks = s.chunks, a.sum_per_wave = s.per_wave, a.sum_tiles = s.tiles, a.fold_scratch = s.fold_scratch;
	return true;
}

// k_vad, k_vad_decide: grid = (tiles, channels, rows of this launch <= 65535)
// k_vad_sum:           grid = (sum_tiles, channels, rows of this launch)
// k_vad_fold:          grid = (channels, 1, rows of this launch)
// k_vad_fill:          one workgroup: energy_threshold into n entries of d_thr
hipError_t lw_launch_vad(const LwVadArgs &a, uint32_t n_rows, hipStream_t st);
hipError_t lw_launch_vad_sum(const LwVadArgs &a, uint32_t n_rows, hipStream_t st);
hipError_t lw_launch_vad_fold(const LwVadArgs &a, uint32_t n_rows, hipStream_t st);
hipError_t lw_launch_vad_decide(const LwVadArgs &a, uint32_t n_rows, hipStream_t st);
hipError_t lw_launch_vad_fill(float *d_thr, uint64_t n, float value, hipStream_t st);
