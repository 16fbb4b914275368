// Row resampler (lw_resampler_*, include/lewton_amd.h "resampling rows"): what lw_resample.cpp (the host side) and
// lw_kernels_resample.hip (k_resample) share -- the kernel's arguments, the per-row records and the launch plan.
// Kept out of lw_kernels.hpp: the synthesis kernels' translation units do not see it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

// One source row of a call, read by every workgroup that works on it.
struct LwResampleRow {
	uint64_t len;     // input samples per channel; x[i] = +0.0 outside [0, len)
	uint64_t out_len; // ceil(len * new / orig): the outputs that are written
	uint64_t dst_row; // destination row
};
static_assert(sizeof(LwResampleRow) == 24, "LwResampleRow is read as six dwords");

// Element offsets are 64-bit all the way: sample i of channel c of row r is element r * row + c * ch + i * el.
//   planar      [row][ch][capacity]:  row = ch * capacity, ch = capacity, el = 1
//   interleaved [row][capacity][ch]:  row = capacity * ch, ch = 1,        el = ch
struct LwResampleLayout {
	uint64_t row, ch, el;
};

struct LwResampleArgs {
	const float *src;
	float *dst;
	const float *taps;         // device order [K][new]: taps[k * new + i] = h[(i * orig) mod new][k], i = n mod new; 16-byte aligned and
	                           // padded with zeros to a multiple of four floats
	const LwResampleRow *rows; // the call's source rows, from rows[0]
	LwResampleLayout s, d;
	uint32_t orig, new_, half_width, k_taps;
	uint32_t blocks; // M: a tile is J runs of M * new consecutive outputs
	uint32_t row0;   // first source row of this launch (blockIdx.z counts from it)
	uint32_t tile0;  // first tile of this launch (blockIdx.x counts from it)
};

// Where the taps and the input span of a tile are read from.
enum {
	LW_RS_ROUTE_LDS = 0,         // tap table and input span in LDS
	LW_RS_ROUTE_GLOBAL_TAPS = 1, // input span in LDS, taps from global memory (L2): the table does not fit
	LW_RS_ROUTE_GLOBAL = 2,      // neither fits (orig in the thousands): both from global memory, one output per lane
	LW_RS_ROUTE_COPY = 3         // orig == new: a copy of [0, len), no arithmetic
};

#define LW_RS_THREADS 512u
#define LW_RS_MAX_TILES 0x7fffffu // tiles of ONE launch: tiles * 512 lanes stays below 2^32, the most a grid dimension holds in lanes
                                  // (a launch past it is accepted, and workgroups of it never run); a row with more
                                  // tiles takes several launches, each with its tile0
#define LW_RS_LDS_FLOATS 20480u // 80 KiB per workgroup: two workgroups per CU (160 KiB)
#define LW_RS_PASSES 8u // a tile stops growing at this many full passes of the workgroup

struct LwResamplePlan {
	int route;
	uint32_t j;          // outputs n, n + new, ... per lane that share one tap register: 4, 2 or 1
	uint32_t blocks;     // M
	uint32_t tile;       // outputs per workgroup: M * J * new  (route COPY: LW_RS_THREADS * 4, route GLOBAL: LW_RS_THREADS)
	uint32_t span;       // input samples a tile stages: M * J * orig + K - 1, rounded up to a multiple of four
	uint32_t lds_floats; // span (+ new * K, rounded up likewise, on route LDS); 0 on the routes that stage nothing
};

// The launch geometry from the filter's alone.  taps_in_lds = false is the debug switch that takes a table that would fit through
// the global-taps route.  Register blocking: a lane keeps h[ph][k] for J outputs of its phase; J is the largest of 4, 2, 1 whose
// span fits next to the table, then M is the block count, up to LW_RS_PASSES passes' worth, that fills LW_RS_THREADS-wide passes best
// (new = 1, as in 3 -> 1, needs 512 blocks to occupy every lane once).
static inline LwResamplePlan lw_resample_plan(uint32_t orig, uint32_t new_, uint32_t k_taps, bool taps_in_lds)
{
	LwResamplePlan p{};
	if (orig == new_) {
		p.route = LW_RS_ROUTE_COPY, p.j = 1, p.blocks = 1, p.tile = LW_RS_THREADS * 4u;
		return p;
	}
	const uint64_t table = ((uint64_t)new_ * k_taps + 3) & ~3ull;
	auto span_of = [&](uint64_t j, uint64_t m) { return (m * j * orig + k_taps - 1 + 3) & ~3ull; };
	uint64_t room = LW_RS_LDS_FLOATS;
	if (taps_in_lds && table + span_of(1, 1) <= LW_RS_LDS_FLOATS) {
		p.route = LW_RS_ROUTE_LDS;
		room -= table;
	} else if (span_of(1, 1) <= LW_RS_LDS_FLOATS) {
		p.route = LW_RS_ROUTE_GLOBAL_TAPS;
	} else {
		p.route = LW_RS_ROUTE_GLOBAL, p.j = 1, p.blocks = 1, p.tile = LW_RS_THREADS;
		return p;
	}
	p.j = span_of(4, 1) <= room ? 4u : span_of(2, 1) <= room ? 2u : 1u;
	p.blocks = 1;
	uint64_t best = ~0ull; // lane slots of the passes per unit of work, in 1/65536
	for (uint32_t m = 1; span_of(p.j, m) <= room; m++) {
		const uint64_t units = (uint64_t)m * new_, passes = (units + LW_RS_THREADS - 1) / LW_RS_THREADS;
		const uint64_t cost = passes * LW_RS_THREADS * 65536u / units;
		if (cost < best)
			best = cost, p.blocks = m;
		if (units >= LW_RS_PASSES * LW_RS_THREADS)
			break;
	}
	p.tile = p.blocks * p.j * new_;
	p.span = (uint32_t)span_of(p.j, p.blocks);
	p.lds_floats = p.span + (p.route == LW_RS_ROUTE_LDS ? (uint32_t)table : 0u);
	return p;
}

// grid = (tiles of the longest row, channels, rows of this launch <= 65535); a workgroup whose tile starts at or behind its row's
// out_len does nothing.  Nothing outside [0, out_len) of a destination row and channel is written.
hipError_t lw_launch_resample(const LwResampleArgs &a, const LwResamplePlan &p, uint32_t tiles, uint32_t ch, uint32_t n_rows, hipStream_t st);
