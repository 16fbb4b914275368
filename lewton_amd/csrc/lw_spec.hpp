// Spectral frames of rows (lw_spec_*, include/lewton_amd.h "spectral frames of rows"): what lw_spec.cpp (the host side) and
// lw_kernels_spec.hip (k_spec) share -- the kernel's arguments, the per-row records, the tile plan and the device order of the
// tables.  Kept out of lw_kernels.hpp: the synthesis kernels' translation units do not see it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

// One source row of a call, read by every workgroup that works on it.
struct LwSpecRow {
	uint64_t len;      // input samples per channel; x[i] = +0.0 outside [0, len)
	uint64_t n_frames; // the frames that are written
	uint64_t dst_row;  // destination row
};
static_assert(sizeof(LwSpecRow) == 24, "LwSpecRow is read as six dwords");

// Source element offsets are 64-bit all the way: sample i of channel c of row r is element r * row + c * ch + i * el.
//   planar      [row][ch][capacity]:  row = ch * capacity, ch = capacity, el = 1
//   interleaved [row][capacity][ch]:  row = capacity * ch, ch = 1,        el = ch
struct LwSpecLayout {
	uint64_t row, ch, el;
};

// The tile plan.  A workgroup of LW_SP_THREADS lanes (four waves) takes LW_SP_TF consecutive frames of one (row, channel) and
// walks the bins in passes of LW_SP_COLS; within a pass wave w owns the columns [64 w, 64 w + 64) as two 32 x 32 output tiles
// (bin x frame), each with a cosine and a sine accumulator: four independent accumulators per wave.  The K loop (the window's
// support, ascending) goes in tiles of LW_SP_KT staged through LDS.
#define LW_SP_THREADS 256u
#define LW_SP_TF 32u    // frames per workgroup: the N of the 32x32x2 matrix instruction
#define LW_SP_MAX_TILES 0xffffffu // tiles of ONE launch: tiles * 256 lanes stays below 2^32, the most a grid dimension holds in lanes
                                  // (a launch past it is accepted, and workgroups of it never run); a row with more
                                  // tiles takes several launches, each with its tile0
#define LW_SP_KT 16u    // support samples per staged tile
#define LW_SP_COLS 256u // bins per pass: 4 waves x 2 tiles x 32
#define LW_SP_XS 33u    // row stride of the staged frame tile [k][frame] (odd: the staging stores spread over the banks)
#define LW_SP_JT 32u    // bins per staged slice of the mel matrix
// LDS, in floats: the basis tile [KT][2][COLS] (the mel slice [JT][mel_pad <= 256] takes its place behind the K loop), the frame
// tile [KT][XS], P of the pass [COLS][TF]
#define LW_SP_LDS_A 0u
#define LW_SP_LDS_X (LW_SP_KT * 2u * LW_SP_COLS)
#define LW_SP_LDS_P (LW_SP_LDS_X + LW_SP_KT * LW_SP_XS)
#define LW_SP_LDS_FLOATS (LW_SP_LDS_P + LW_SP_COLS * LW_SP_TF)
static_assert(LW_SP_JT * 256u <= LW_SP_LDS_X, "the mel slice fits the basis tile's place");
static_assert(LW_SP_LDS_FLOATS * 4u <= 80u * 1024u, "two workgroups per CU");

enum { LW_SP_ROUTE_MFMA = 0, LW_SP_ROUTE_FMA = 1 };

struct LwSpecPlan {
	uint32_t bins;    // B = n_fft / 2 + 1
	uint32_t offset;  // o = (n_fft - win_length) / 2
	uint32_t k_pad;   // win_length rounded up to LW_SP_KT: the tail's operands are zeros
	uint32_t passes;  // ceil(B / LW_SP_COLS)
	uint32_t mel_pad; // n_mels rounded up to 32 (0 without a mel matrix)
	uint32_t j_pad;   // B rounded up to LW_SP_JT: rows of the device mel matrix
};

static inline LwSpecPlan lw_spec_plan(uint32_t n_fft, uint32_t win_length, uint32_t n_mels)
{
	LwSpecPlan p{};
	p.bins = n_fft / 2u + 1u;
	p.offset = (n_fft - win_length) / 2u;
	p.k_pad = (win_length + LW_SP_KT - 1u) / LW_SP_KT * LW_SP_KT;
	p.passes = (p.bins + LW_SP_COLS - 1u) / LW_SP_COLS;
	p.mel_pad = (n_mels + 31u) / 32u * 32u;
	p.j_pad = (p.bins + LW_SP_JT - 1u) / LW_SP_JT * LW_SP_JT;
	return p;
}

// Device order of the basis: [pass][k < k_pad][C | S][LW_SP_COLS], so the tile of (pass, K tile) is one run of KT * 2 * COLS
// floats; zeros where k >= win_length or the bin >= B.  Element index of (k, sine?, bin):
static inline size_t lw_spec_basis_at(const LwSpecPlan &p, uint32_t k, uint32_t sine, uint32_t bin)
{
	const uint32_t pass = bin / LW_SP_COLS, c = bin % LW_SP_COLS;
	return (((size_t)pass * p.k_pad + k) * 2u + sine) * LW_SP_COLS + c;
}
// Device order of the mel matrix: [j < j_pad][mel_pad], fb[q][j] at j * mel_pad + q; zeros in the padding.

static inline uint64_t lw_spec_n_frames(uint64_t len, uint32_t n_fft, uint32_t hop, bool center)
{
	if (len == 0)
		return 0;
	if (center)
		return 1u + len / hop;
	return len < n_fft ? 0 : 1u + (len - n_fft) / hop;
}

// Reflect padding (LW_SPEC_PAD_REFLECT, centred frames): x[i] = x[-i] below 0, x[2 (len - 1) - i] from len on.  ONE reflection has
// to reach every support sample of every frame: -(n_fft / 2) from below, and len - n_fft / 2 + n_fft - 1 (the last sample of frame
// len / hop when hop divides len) from above.  The shortest row that allows it:
static inline uint64_t lw_spec_reflect_min_len(uint32_t n_fft)
{
	return (uint64_t)n_fft - n_fft / 2u + 1u;
}

struct LwSpecArgs {
	const float *src;
	float *dst;
	const float *basis; // device order, 16-byte aligned
	const float *fb;    // device order, 16-byte aligned; NULL without a mel matrix
	const LwSpecRow *rows;
	LwSpecLayout s;
	uint64_t d_row, d_ch, d_line; // destination: elements per row, per channel (F * frame_capacity), per line (frame_capacity)
	int64_t lead;                 // o - pad: sample 0 of frame t's SUPPORT is x[t * hop + lead]
	uint32_t hop, win_length, k_pad, bins, passes, n_mels, mel_pad;
	uint32_t row0; // first source row of this launch (blockIdx.z counts from it)
	uint32_t tile0; // first tile of this launch (blockIdx.x counts from it)
	uint32_t pad_mode; // LW_SPEC_PAD_ZERO / LW_SPEC_PAD_REFLECT / LW_SPEC_PAD_SYMMETRIC: what x[i] is outside [0, len)
	// the per-frame prologue (k_spec<.., .., 1>); all zero: as before
	uint32_t remove_dc; // x'_k = x_k - mu, mu the frame's mean
	uint32_t energy;    // line 0 of the destination is the frame's energy, the spectrum or mel lines follow from line 1
	uint32_t span;      // 31 * hop + win_length when the prologue stages the tile's samples through LDS (lw_spec_span_fits), else 0
	double escale;      // scale * scale, what the energy is multiplied by
	uint32_t output;    // LW_SPEC_OUT_POWER, or LW_SPEC_OUT_COMPLEX: re on the lines [0, bins), im on [bins, 2 bins) (k_spec_complex)
};

// The prologue's sums run over the samples of 32 frames, hop apart.  When the tile's span of 31 * hop + win_length samples fits
// the P region of LDS (free until the first power), it is staged there once, coalesced, sample s at word s + (s >> 5): the skew
// spreads the 32 chain lanes, which read hop words apart, over the banks where hop is a multiple of 32 (hop = 160: bank
// 5 f + k + (k >> 5) mod 32, all different).  Otherwise the chain lanes read the row itself.
#define LW_SP_SPAN_AT(s) ((s) + ((s) >> 5))
static inline bool lw_spec_span_fits(uint32_t hop, uint32_t win_length)
{
	const uint64_t span = (uint64_t)(LW_SP_TF - 1u) * hop + win_length;
	return span + (span >> 5) + 1u <= (uint64_t)LW_SP_COLS * LW_SP_TF;
}

// Kaldi framing (LW_SPEC_FRAMES_KALDI_SNIP, LW_SPEC_FRAMES_KALDI_EDGES): frames are counted by the window, which starts at sample 0
// of the frame.  lead: the input index of support sample 0 of frame 0.
static inline uint64_t lw_spec_kaldi_frames(uint64_t len, uint32_t win_length, uint32_t hop, bool snip)
{
	if (snip)
		return len < win_length ? 0 : 1u + (len - win_length) / hop;
	return (len + hop / 2u) / hop;
}
static inline int64_t lw_spec_kaldi_lead(uint32_t win_length, uint32_t hop, bool snip)
{
	return snip ? 0 : (int64_t)(hop / 2u) - (int64_t)(win_length / 2u);
}

// grid = (tiles of this launch <= LW_SP_MAX_TILES, from a.tile0 on, channels, rows of this launch <= 65535); a workgroup whose
// tile starts at or behind its row's n_frames does nothing.  Nothing outside [0, n_frames) of a destination line is written.
hipError_t lw_launch_spec(const LwSpecArgs &a, int route, uint32_t tiles, uint32_t ch, uint32_t n_rows, hipStream_t st);
