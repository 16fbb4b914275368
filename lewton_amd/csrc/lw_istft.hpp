// Inverse spectral frames of rows (lw_istft_*, include/lewton_amd.h "inverse spectral frames of rows"): what lw_istft.cpp (the
// host side) and lw_kernels_istft.hip (k_istft) share -- the kernel's arguments, the per-row records, the tile plan and the
// device order of the table.  Kept out of lw_kernels.hpp: the other kernels' translation units do not see it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

// One source row of a call, read by every workgroup that works on it.
struct LwIstftRow {
	uint64_t frames;  // T: the frames the source row holds
	uint64_t out_len; // samples per channel that are written: [0, out_len)
	uint64_t dst_row; // destination row
};
static_assert(sizeof(LwIstftRow) == 24, "LwIstftRow is read as six dwords");

// Destination element offsets are 64-bit all the way: sample n of channel c of row r is element r * row + c * ch + n * el.
//   planar      [row][ch][capacity]:  row = ch * capacity, ch = capacity, el = 1
//   interleaved [row][capacity][ch]:  row = capacity * ch, ch = 1,        el = ch
struct LwIstftLayout {
	uint64_t row, ch, el;
};

// The tile plan.  A workgroup of LW_IS_THREADS lanes (four waves) OWNS the padded samples [u m hop, (u + 1) m hop) of one (row,
// channel) and computes the frame signals y_t of the LW_IS_TF = 32 frames from the first one that touches its span, at their true
// indices: every frame that touches the span is among them (below), so the overlap-add of every owned sample is the complete
// ascending fold whatever m and the grid are.  The frame signals are a GEMM, D[k][t] = sum_l G[l][k] X[l][t], on the 32x32x2
// matrix instruction: M = 32 support samples (A operand, from the table), N = 32 frames (B operand, from the source, whose
// lines run along frames), K = the 2 B source lines ascending, in tiles of LW_IS_KT staged through LDS.  The support is walked
// in passes of LW_IS_COLS samples, from the highest k down; within a pass wave w owns the samples [64 w, 64 w + 64) as two
// 32 x 32 output tiles (sample x frame).  Behind a pass's K loop its y goes to LDS and every owned sample adds what the pass
// holds for it, t ascending.
//
// Frames that touch [s0, s0 + m hop): t hop in [s0 - o - W + 1, s0 + m hop - 1 - o], m hop + W - 1 consecutive integers, which
// hold at most m + ceil((W - 1) / hop) <= m + ov multiples of hop (m + ov - 1 where hop divides o).  So m + ov <= 32.
#define LW_IS_THREADS 256u
#define LW_IS_TF 32u    // frames per workgroup: the N of the 32x32x2 matrix instruction
#define LW_IS_KT 16u    // source lines per staged tile
#define LW_IS_COLS 256u // support samples per pass: 4 waves x 2 tiles x 32
#define LW_IS_YS 33u    // row stride of the pass's y [sample][frame] (odd: the overlap-add reads run down consecutive samples)
#define LW_IS_MAX_OV 16u // LW_ISTFT_MAX_OVERLAP
#define LW_IS_MAX_TILES 0xffffffu // tiles of ONE launch (as LW_SP_MAX_TILES)
// LDS, in floats: the table tile [KT][COLS], the source tile [KT][TF], y of the pass [COLS][YS], the running xh of the owned span
#define LW_IS_LDS_A 0u
#define LW_IS_LDS_X (LW_IS_KT * LW_IS_COLS)
#define LW_IS_LDS_Y (LW_IS_LDS_X + LW_IS_KT * LW_IS_TF)
#define LW_IS_LDS_H (LW_IS_LDS_Y + LW_IS_COLS * LW_IS_YS)
#define LW_IS_SPAN_MAX 7168u // floats of xh: the owned span m * hop fits it (hop <= 2048 = LW_SPEC_MAX_FFT: m >= 3)
#define LW_IS_LDS_FLOATS (LW_IS_LDS_H + LW_IS_SPAN_MAX)
static_assert(LW_IS_LDS_FLOATS * 4u <= 80u * 1024u, "two workgroups per CU");
static_assert(LW_IS_LDS_A % 4u == 0, "the table tile is stored 16 bytes at a time");

enum { LW_IS_ROUTE_MFMA = 0, LW_IS_ROUTE_FMA = 1 };

struct LwIstftPlan {
	uint32_t bins;   // B = n_fft / 2 + 1
	uint32_t lines;  // 2 B: the source's lines, re then im
	uint32_t l_pad;  // lines rounded up to LW_IS_KT: the tail's operands are zeros
	uint32_t offset; // o = (n_fft - win_length) / 2
	uint32_t passes; // ceil(win_length / LW_IS_COLS)
	uint32_t ov;     // ceil(win_length / hop)
	uint32_t m;      // owned frames-worth of samples per tile: min(32 - ov, LW_IS_SPAN_MAX / hop)
};

static inline uint32_t lw_istft_max_m(uint32_t ov, uint32_t hop)
{
	const uint32_t a = LW_IS_TF - ov, b = LW_IS_SPAN_MAX / hop;
	return a < b ? a : b;
}

static inline LwIstftPlan lw_istft_plan(uint32_t n_fft, uint32_t win_length, uint32_t hop)
{
	LwIstftPlan p{};
	p.bins = n_fft / 2u + 1u;
	p.lines = 2u * p.bins;
	p.l_pad = (p.lines + LW_IS_KT - 1u) / LW_IS_KT * LW_IS_KT;
	p.offset = (n_fft - win_length) / 2u;
	p.passes = (win_length + LW_IS_COLS - 1u) / LW_IS_COLS;
	p.ov = (win_length + hop - 1u) / hop;
	p.m = lw_istft_max_m(p.ov, hop);
	return p;
}

// Device order of the table: [pass][l < l_pad][LW_IS_COLS], so the tile of (pass, K tile) is one run of KT * COLS floats; zeros
// where l >= 2 B or the sample >= win_length.  Element index of (l, k):
static inline size_t lw_istft_table_at(const LwIstftPlan &p, uint32_t l, uint32_t k)
{
	const uint32_t pass = k / LW_IS_COLS, c = k % LW_IS_COLS;
	return ((size_t)pass * p.l_pad + l) * LW_IS_COLS + c;
}

struct LwIstftArgs {
	const float *src;
	float *dst;
	const float *table; // device order, 16-byte aligned
	const double *w2;   // [win_length]: w[k] * w[k] in double, one rounding
	const LwIstftRow *rows;
	LwIstftLayout d;
	uint64_t s_row, s_ch, s_line; // source: elements per row, per channel (2 B * frame_capacity), per line (frame_capacity)
	uint64_t pad;                 // center ? n_fft / 2 : 0: output sample n is padded sample n + pad
	uint32_t n_fft, hop, win_length, offset, lines, l_pad, passes;
	uint32_t m;     // the tile owns m * hop padded samples
	uint32_t row0;  // first source row of this launch (blockIdx.z counts from it)
	uint32_t tile0; // first tile of this launch (blockIdx.x counts from it)
};

// grid = (tiles of this launch <= LW_IS_MAX_TILES, from a.tile0 on, channels, rows of this launch <= 65535); a workgroup whose
// span starts at or behind pad + out_len of its row does nothing.  Exactly [0, out_len) of a destination row and channel is written.
hipError_t lw_launch_istft(const LwIstftArgs &a, int route, uint32_t tiles, uint32_t ch, uint32_t n_rows, hipStream_t st);
