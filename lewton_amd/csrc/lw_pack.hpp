// Frame-major model input (lw_pack_*, include/lewton_amd.h "frame-major model input"): what lw_pack.cpp (the host side) and
// lw_kernels_pack.hip (k_pack) share -- the two conversions as integer arithmetic on the bit pattern (ONE source for the kernel,
// its host build and lw_pack_convert), the frame rule, the per-row record, the tile plan, the kernel's arguments and the
// launcher.  Kept out of lw_kernels.hpp: no other translation unit sees it.
#pragma once

#include "lw_lanes.hpp"

#define LW_PK_THREADS 256u // a workgroup
#define LW_PK_GROUP 32u    // feature lines in the LDS image at a time: one line per bank
#define LW_PK_SPAN 288u    // the most source frames a tile's image holds per line
#define LW_PK_MAX_TILES 0xffffffu // tiles of a launch: tiles * 256 lanes stays below 2^32, the most a grid dimension holds in lanes
#define LW_PK_F32 0
#define LW_PK_BF16 1
#define LW_PK_F16 2
#define LW_PK_REPLICATE 0
#define LW_PK_VALID 1

// ---- the contract's conversions of an f32 bit pattern
LW_LANES_HD uint32_t lw_pack_bf16(uint32_t u)
{
	if ((u & 0x7fffffffu) > 0x7f800000u) // a NaN first: the rounding below would carry some into infinity or zero
		return (u >> 16) | 0x40u;
	return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

LW_LANES_HD uint32_t lw_pack_f16(uint32_t u)
{
	const uint32_t s = (u >> 16) & 0x8000u, a = u & 0x7fffffffu;
	if (a > 0x7f800000u)
		return s | 0x7e00u;
	if (a >= 0x47800000u)
		return s | 0x7c00u;
	if (a >= 0x38800000u) {
		const uint32_t m = a - 0x38000000u;
		return s | ((m + 0xfffu + ((m >> 13) & 1u)) >> 13);
	}
	if (a < 0x33000000u)
		return s;
	const uint32_t sh = 126u - (a >> 23), M = (a & 0x7fffffu) | 0x800000u;
	uint32_t r = M >> sh;
	const uint32_t rem = M & ((1u << sh) - 1u), half = 1u << (sh - 1u);
	r += (rem > half || (rem == half && (r & 1u))) ? 1u : 0u;
	return s | r;
}

LW_LANES_HD uint32_t lw_pack_cvt(int dtype, uint32_t u)
{
	return dtype == LW_PK_BF16 ? lw_pack_bf16(u) : dtype == LW_PK_F16 ? lw_pack_f16(u) : u;
}

// T_out of a row of T frames
LW_LANES_HD uint64_t lw_pack_out_frames(int edge, uint32_t W, uint32_t stride, uint64_t T)
{
	if (edge == LW_PK_VALID)
		return T < W ? 0u : (T - W) / stride + 1u;
	return T / stride + (T % stride ? 1u : 0u);
}

// One row of a call.
struct LwPackRow {
	uint64_t n;        // T: frames [0, n) of every source line may be read
	uint64_t n_out;    // T_out: output frames [0, n_out) are computed
	uint64_t fill_end; // max(T_out, fill_to): [T_out, fill_end) receives pad
};
static_assert(sizeof(LwPackRow) == 24, "LwPackRow is read as six dwords");

// The tile plan.  A workgroup takes `tile` consecutive output frames of one row and channel; their source is a span of
// (tile - 1) * stride + W consecutive frames (clamped at the row's ends), which the image holds for 32 lines at a time.  tile is
// the largest of 256, 128, 64, 32, 16 whose span is at most LW_PK_SPAN: 256 at stride 1 (any W), 128 at stride 2, 64 at strides
// 3 and 4, 32 at strides 5 .. 8 (LFR 7/6: a span of 193) and at stride 9 up to W = 9, 16 beyond (stride 16, W = 33: 273).  The pitch of a line is
// the span rounded up to 1 mod 32, so line g, frame s lies on bank (g + s) mod 32.  The bits depend on none of this.
struct LwPackPlan {
	uint32_t tile;  // output frames a workgroup produces
	uint32_t pitch; // floats per line of the image
	uint32_t lines; // lines of the image: min(F, 32)
	uint32_t lds;   // bytes of LDS a workgroup needs
};

static inline LwPackPlan lw_pack_plan(uint32_t F, uint32_t W, uint32_t stride)
{
	LwPackPlan p;
	p.tile = 256u;
	while (p.tile > 16u && (p.tile - 1u) * stride + W > LW_PK_SPAN)
		p.tile >>= 1;
	const uint32_t span = (p.tile - 1u) * stride + W;
	p.pitch = ((span + 30u) & ~31u) + 1u;
	p.lines = F < LW_PK_GROUP ? F : LW_PK_GROUP;
	p.lds = p.lines * p.pitch * (uint32_t)sizeof(float);
	return p;
}

struct LwPackArgs {
	const LwPackRow *rows;
	const float *shift, *scale; // device, D floats each, or NULL
	uint64_t line_el;           // frame_capacity: elements per source line
	uint64_t out_cap;           // out_capacity: frames per destination channel
	uint32_t ch, F, left, stride, W, D;
	int32_t edge, dtype;
	uint32_t pad_bits; // pad, converted
	uint32_t vec;      // the destination's frames start on 16-byte boundaries and F is a multiple of the elements in 16 bytes
	uint32_t row0;     // first row of this launch (blockIdx.z counts from it)
	LwPackPlan plan;
};

// k_pack: grid = (tiles of the longest fill_end, channels, rows of this launch <= 65535).  mask: uint8 [rows][out_cap] or NULL.
hipError_t lw_launch_pack(const LwPackArgs &a, const float *src, void *dst, uint8_t *mask, uint32_t tiles, uint32_t n_rows, hipStream_t st);
