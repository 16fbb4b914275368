// Frame selection (lw_select_*, include/lewton_amd.h "frame decisions and frame selection"): what lw_select.cpp (the host side) and
// lw_kernels_select.hip (k_select_count, k_select) share -- the per-row record, the tile plan, the kernels' arguments and the
// launchers.  Integer arithmetic only.  Kept out of lw_kernels.hpp: no other translation unit sees it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#define LW_SE_THREADS 256u        // a workgroup
#define LW_SE_TILE 1024u          // frames of a tile unless a test says otherwise: a multiple of 256 in 256 .. 2048
#define LW_SE_MAX_TILE 2048u      // (a lane takes tile / 256 consecutive frames; a kept frame's place in its tile is a uint16)
#define LW_SE_LINES 16u           // feature lines a workgroup copies with one compaction of its tile
#define LW_SE_MAX_TILES 0xffffffu // workgroups in a grid's first dimension: tiles * line groups * 256 lanes stays below 2^32
// LDS of k_select, static: 256 counts + 16 group totals + 2 x 256 partial sums of the tile counts + the tile's kept places
#define LW_SE_LDS (256u * 4u + 16u * 4u + 512u * 8u + LW_SE_MAX_TILE * 2u)

// One row of a call.
struct LwSelectRow {
	uint64_t n;        // T: frames [0, n) of the mask and of every source line may be read
	uint64_t fill_end; // max(T, fill_to): positions [K, fill_end) receive +0.0
};
static_assert(sizeof(LwSelectRow) == 16, "LwSelectRow is read as four dwords");

struct LwSelectArgs {
	const LwSelectRow *rows;
	uint32_t *tile_counts; // scratch [row of the call][ch][tiles]: kept frames of every tile (k_select_count -> k_select)
	uint64_t *d_counts;    // NULL, or [n_rows][ch]: K
	uint64_t line_el;      // frame_capacity: elements per line, and per (row, channel) of the mask
	uint32_t ch, F;
	uint32_t tile;   // frames of a tile
	uint32_t tiles;  // tiles of the longest fill_end: the pitch of tile_counts
	uint32_t groups; // line groups of a channel: ceil(F / 16); k_select's blockIdx.x = tile * groups + group
	uint32_t row0;   // first row of this launch (blockIdx.z counts from it)
};

static inline bool lw_select_tile_ok(uint32_t tile)
{
	return tile >= LW_SE_THREADS && tile <= LW_SE_MAX_TILE && tile % LW_SE_THREADS == 0;
}

// k_select_count: grid = (tiles, channels, rows of this launch <= 65535)
// k_select:       grid = (tiles * groups, channels, rows of this launch)
hipError_t lw_launch_select_count(const LwSelectArgs &a, const uint8_t *mask, uint32_t n_rows, hipStream_t st);
hipError_t lw_launch_select(const LwSelectArgs &a, const uint32_t *src, const uint8_t *mask, uint32_t *dst, uint32_t n_rows, hipStream_t st);
