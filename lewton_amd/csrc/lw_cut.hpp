// Segment rows (lw_cut_*, include/lewton_amd.h "cutting rows into segment rows"): what lw_cut.cpp (the host side) and
// lw_kernels_cut.hip (k_cut) share -- the per-job record, the kernel's arguments and the launcher.  Bit copies and integer
// arithmetic only.  Kept out of lw_kernels.hpp: no other translation unit sees it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#define LW_CT_THREADS 256u        // a workgroup
#define LW_CT_GROUP 16u           // bytes of a store
#define LW_CT_TILE 16384u         // destination bytes of a workgroup: four 16-byte groups per lane
#define LW_CT_MAX_TILES 0xffffffu // workgroups in a grid's first dimension: tiles * lines of a channel * 256 lanes stays below 2^32

// One job of a call: one output row.
struct LwCutJob {
	uint64_t src_at;   // element of src[row][0][0][start]
	uint64_t len;      // end - start: elements of every line that are copied
	uint64_t fill_end; // max(len, fill_to): positions [len, fill_end) of every destination line receive zero bits
};
static_assert(sizeof(LwCutJob) == 24, "LwCutJob is read as six dwords");

struct LwCutArgs {
	const LwCutJob *jobs;
	const uint8_t *src;
	uint8_t *dst;
	uint64_t src_line; // capacity: elements per source line
	uint64_t dst_line; // out_capacity: elements per destination line
	uint32_t ch, F;
	uint32_t elem;  // bytes of an element: 2 or 4
	uint32_t tiles; // tiles of the longest fill_end
	uint32_t job0;  // first job of this launch (blockIdx.z counts from it)
};

// k_cut: grid = (tiles * F, channels, jobs of this launch <= 65535); blockIdx.x = tile * F + line
hipError_t lw_launch_cut(const LwCutArgs &a, uint32_t n_jobs, hipStream_t st);
