// Speech segments from a frame mask (lw_segment_*, include/lewton_amd.h "segments of a frame mask"): what lw_segment.cpp (the host
// side) and lw_kernels_segment.hip (k_segment_count, k_segment) share -- the per-row record, the tile plan, the kernels' arguments
// and the launchers.  Integer arithmetic only.  Kept out of lw_kernels.hpp: no other translation unit sees it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#define LW_SG_THREADS 256u        // a workgroup
#define LW_SG_WAVES 4u
#define LW_SG_TILE 1024u          // frames of a tile unless a test says otherwise: a multiple of 256 in 256 .. 2048
#define LW_SG_MAX_TILE 2048u
#define LW_SG_MAX_SPAN 1024u      // LW_SEG_MAX_SPAN
#define LW_SG_MAX_HALO (3u * LW_SG_MAX_SPAN + 1u) // H + 1: O[t0 - 1] and O[t0 + tile] tell whether a run starts or ends at a seam
#define LW_SG_MAX_TILES 0xffffffu // workgroups in a grid's first dimension: tiles * 256 lanes stays below 2^32
#define LW_SG_WORDS ((LW_SG_MAX_TILE + 2u * LW_SG_MAX_HALO + 63u) / 64u) // ballot words of a tile and its halo either side
// LDS of k_segment, static: two lists of words the passes alternate between, the starts, the ends, 256 partial sums of the tile counts
#define LW_SG_LDS (4u * LW_SG_WORDS * 8u + LW_SG_THREADS * 8u)

// One row of a call.
struct LwSegmentRow {
	uint64_t n;        // T: frames [0, n) of the mask may be read
	uint64_t fill_end; // max(T, fill_to): positions [T, fill_end) of the smoothed mask receive 0
};
static_assert(sizeof(LwSegmentRow) == 16, "LwSegmentRow is read as four dwords");

struct LwSegmentArgs {
	const LwSegmentRow *rows;
	const uint8_t *mask;
	uint32_t *tile_counts; // scratch [row of the launch][ch][tiles]: segment starts of every tile (k_segment_count -> k_segment)
	uint64_t *d_spans;     // NULL, or [n_rows][ch][seg_capacity][2]
	uint64_t *d_counts;    // NULL, or [n_rows][ch]: K
	uint8_t *d_smooth;     // NULL, or [n_rows][ch][frame_capacity]
	uint64_t line_el;      // frame_capacity: bytes per (row, channel) of both masks
	uint64_t seg_capacity;
	uint32_t ch;
	uint32_t tile;  // frames of a tile
	uint32_t tiles; // tiles of the call's longest span: the pitch of tile_counts
	uint32_t row0;  // first row of this launch (blockIdx.z counts from it)
	uint32_t pad_onset, pad_offset, min_off, min_on;
};

static inline bool lw_segment_tile_ok(uint32_t tile)
{
	return tile >= LW_SG_THREADS && tile <= LW_SG_MAX_TILE && tile % LW_SG_THREADS == 0;
}

// k_segment_count, k_segment: grid = (tiles, channels, rows of this launch <= 65535)
hipError_t lw_launch_segment_count(const LwSegmentArgs &a, uint32_t n_rows, hipStream_t st);
hipError_t lw_launch_segment(const LwSegmentArgs &a, uint32_t n_rows, hipStream_t st);
