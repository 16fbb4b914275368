// Segment rows (product code, gfx950): k_cut, the kernel of lw_cut_rows.  A pass of its own from rows [row][ch][F][capacity] of 2- or
// 4-byte elements to one output row [ch][F][out_capacity] per job (row, start, end), by the rule of include/lewton_amd.h ("cutting
// rows into segment rows"): dst[i][c][f][j] = src[row][c][f][start + j] for j < len, zero bits on [len, max(len, fill_to)).  Bit
// copies only.  ONE launch: a workgroup of 256 lanes takes 16384 destination bytes of one line of one job.  A lane takes groups of 16
// bytes at a 16-byte boundary of the destination's ADDRESS: a group that lies inside the tile and inside the copied part is ONE
// 16-byte load from the source at whatever alignment the start gives it (the address is a multiple of the element size and no
// more: gfx950 serves such a load, at the price of the cache lines it straddles) and ONE aligned 16-byte store; a group that the
// copy's end cuts is put together element by element and still leaves as one store; a group that the tile's start or end cuts goes
// element by element.  Every byte of [0, fill_end) of a line is written once, nothing else is; nothing outside [start, end) of a
// source line is read.  No atomics, no LDS, offsets in 64 bits.  tests/san/cut_host.cpp compiles this file for the host
// (LW_CUT_HOST) and runs it workgroup by workgroup.
#include "lw_cut.hpp"

#include <string.h>

#include "lw_lanes.hpp"
#ifndef LW_KERNEL_HOST
#include "lw_kernels.hpp"
#endif

typedef uint32_t LwCtV4 __attribute__((vector_size(16)));

struct LwCtTile { // what a workgroup works on; the same for all its lanes
	const uint8_t *s; // byte 0 of the job's part of the source line
	uint8_t *d;       // byte 0 of the destination line
	uint64_t len_b;   // bytes copied
	uint64_t b0, b1;  // the tile's bytes of the line: its share of [0, fill_end)
};

LW_LANES_FN void lw_ct_tile(const LwCutArgs &a, uint32_t bx, uint32_t by, uint32_t bz, LwCtTile &t)
{
	const uint64_t job = (uint64_t)a.job0 + bz;
	const LwCutJob j = a.jobs[job];
	const uint32_t tile_i = bx / a.F, f = bx % a.F;
	const uint64_t line = (uint64_t)by * a.F + f, end_b = j.fill_end * a.elem;
	t.s = a.src + (j.src_at + line * a.src_line) * a.elem;
	t.d = a.dst + ((job * a.ch * a.F + line) * a.dst_line) * a.elem;
	t.len_b = j.len * a.elem;
	t.b0 = (uint64_t)tile_i * LW_CT_TILE;
	t.b1 = t.b0 + LW_CT_TILE < end_b ? t.b0 + LW_CT_TILE : end_b;
}

// the element at byte p of the line: a copy below len_b, zero bits from there on
template <uint32_t ELEM>
LW_LANES_FN uint32_t lw_ct_elem(const LwCtTile &t, uint64_t p)
{
	if (p >= t.len_b)
		return 0u;
	if (ELEM == 4u)
		return *(const uint32_t *)(t.s + p);
	return *(const uint16_t *)(t.s + p);
}

template <uint32_t ELEM>
LW_LANES_FN void lw_ct_lane(const LwCtTile &t, uint32_t tid)
{
	if (t.b0 >= t.b1)
		return;
	const uint32_t head = (uint32_t)((uintptr_t)(t.d + t.b0) & (LW_CT_GROUP - 1u));
	const uint32_t groups = (uint32_t)((t.b1 - t.b0 + head + LW_CT_GROUP - 1u) / LW_CT_GROUP);
	for (uint32_t g = tid; g < groups; g += LW_CT_THREADS) {
		const int64_t p = (int64_t)t.b0 - (int64_t)head + (int64_t)g * LW_CT_GROUP;
		if (p >= (int64_t)t.b0 && (uint64_t)p + LW_CT_GROUP <= t.b1) { // all sixteen bytes are the tile's: ONE store
			LwCtV4 v = {0u, 0u, 0u, 0u};
			if ((uint64_t)p + LW_CT_GROUP <= t.len_b) {
				memcpy(&v, __builtin_assume_aligned(t.s + p, ELEM), LW_CT_GROUP); // ONE load
			} else if ((uint64_t)p < t.len_b) { // the copy ends inside the group
#pragma unroll
				for (uint32_t k = 0; k < LW_CT_GROUP / ELEM; k++)
					v[k * ELEM / 4u] |= lw_ct_elem<ELEM>(t, (uint64_t)p + k * ELEM) << (8u * (k * ELEM % 4u));
			}
			*(LwCtV4 *)(t.d + p) = v;
			continue;
		}
		for (int64_t q = p; q < p + (int64_t)LW_CT_GROUP; q += ELEM) // the ragged head and tail of the tile's bytes
			if (q >= (int64_t)t.b0 && (uint64_t)q < t.b1) {
				const uint32_t e = lw_ct_elem<ELEM>(t, (uint64_t)q);
				if (ELEM == 4u)
					*(uint32_t *)(t.d + q) = e;
				else
					*(uint16_t *)(t.d + q) = (uint16_t)e;
			}
	}
}

LW_LANES_FN void lw_ct_workgroup_lane(const LwCutArgs &a, uint32_t bx, uint32_t by, uint32_t bz, uint32_t tid)
{
	LwCtTile t;
	lw_ct_tile(a, bx, by, bz, t);
	if (a.elem == 4u)
		lw_ct_lane<4u>(t, tid);
	else
		lw_ct_lane<2u>(t, tid);
}

#ifndef LW_KERNEL_HOST

__global__ void __launch_bounds__(LW_CT_THREADS) k_cut(LwCutArgs a)
{
	lw_ct_workgroup_lane(a, blockIdx.x, blockIdx.y, blockIdx.z, threadIdx.x);
}

hipError_t lw_launch_cut(const LwCutArgs &a, uint32_t n_jobs, hipStream_t st)
{
	if (n_jobs == 0 || n_jobs > 65535u || a.ch == 0 || a.ch > 65535u || a.F == 0 || !a.jobs || !a.dst || (a.elem != 2u && a.elem != 4u) || a.tiles == 0 ||
			(uint64_t)a.tiles * a.F > LW_CT_MAX_TILES)
		return hipErrorInvalidValue;
	return lw_launch_k(k_cut, dim3(a.tiles * a.F, a.ch, n_jobs), dim3(LW_CT_THREADS), 0, st, a);
}

#endif // LW_KERNEL_HOST
