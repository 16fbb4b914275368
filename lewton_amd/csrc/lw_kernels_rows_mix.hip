// Stream-major rows through a channel matrix (product code, gfx950): k_rows_mix, the assembler of lw_rows_synth_mix.  Like
// k_rows (lw_kernels_rows.hip) it runs behind the synthesis kernels on the same HIP stream and moves their packet-major PCM into
// [row][out_ch][sample] (planar) or [row][sample][out_ch] (interleaved) buffers; on the way every destination sample is folded
// from the input channels of its packet position by the rule of include/lewton_amd.h:
//   input channels in ascending order; a coefficient == 0 contributes nothing, == 1 the sample's BITS, any other one rounded f32
//   multiply; the first contribution is the accumulator, every later one one rounded f32 add; no contribution: +0.0.
// The unit is compiled with -ffp-contract=off like all others, so no multiply is fused with an add; samples and accumulators are
// held as bit patterns, so a lone 1.0 is a copy of any NaN payload (and of an i16 sample: the i16 formats take routing matrices
// only, lw_rows_mix.cpp refuses the others, and use the same code with 2-byte loads and stores).
//
// Work: pieces of at most LW_ROWS_MIX_PIECE sample positions of one packet, ALL channels (LwRowMixPiece, lw_kernels.hpp), one WAVE
// per piece, four pieces per workgroup, the grid capped and a grid stride behind it.  The matrix is read with wave-uniform indices
// (scalar loads) and every "is 0 / is 1 / first contribution" decision is a wave-uniform branch; a lane only loads, multiplies,
// adds and stores.  A lane walks the input channels that have a non-zero column and keeps up to LW_ROWS_MIX_OUT accumulators per
// position in registers (instantiated for 2 and for LW_ROWS_MIX_OUT: mono and stereo rows run at a quarter of the registers).
//   planar f32:   when the rows are 16-byte aligned and row_capacity is a multiple of 4 (every output channel shares the
//                 destination's alignment), a scalar head up to the destination's next 16-byte boundary, then a lane owns FOUR
//                 consecutive positions (two such groups per pass for mono and stereo rows): one 16-byte load per input channel, one aligned 16-byte
//                 store per output channel; head and tail together in one scalar pass.  The loads carry only the element's
//                 alignment, like k_rows': behind an odd skip the same instruction reads across 16-byte lines.  Otherwise (odd
//                 row_capacity) everything goes the scalar way.
//   interleaved:  a lane owns positions lane, lane + 64, ... (four per pass); the out_ch samples of a position leave as ONE 8- or
//                 16-byte store for f32 with out_ch 2 or 4 where the destination is aligned so, else one store per sample.
//   i16 planar:   the scalar way.
// Every destination address is formed in 64 bits; source offsets fit 32 bits like the batch's output offsets.
// Bound: HBM bandwidth (one read of the batch's PCM, out_ch / in_ch of a write); no LDS, no scratch.
#include "lw_kernels.hpp"

#include <hip/hip_runtime.h>

#define LW_MIX_WAVES 4u       // pieces per workgroup pass
#define LW_MIX_MAX_GRID 2048u // workgroups; the rest of the list by grid stride
#define LW_MIX_SPAN 4u        // positions per lane and pass, the scalar way

template <int ES> struct LwMixElem;
template <> struct LwMixElem<2> { typedef uint16_t type; };
template <> struct LwMixElem<4> { typedef uint32_t type; };

typedef uint32_t lw_mix_u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t lw_mix_u32x2 __attribute__((ext_vector_type(2)));
struct __attribute__((packed, aligned(4))) LwMixVec { // 16 bytes at an address that is only aligned like an element
	lw_mix_u32x4 v;
};

__device__ __forceinline__ float lw_mix_f(uint32_t u)
{
	return __builtin_bit_cast(float, u);
}
__device__ __forceinline__ uint32_t lw_mix_u(float f)
{
	return __builtin_bit_cast(uint32_t, f);
}

// The folding rule for W positions at once.  load(c, x) fetches input channel c of the lane's positions; it is called once per
// input channel that has a non-zero coefficient in some row.  Everything that depends on the matrix is wave-uniform.
template <uint32_t MO, uint32_t W, class Load>
__device__ __forceinline__ void lw_mix_fold(uint32_t (&acc)[MO][W], const float *__restrict__ coef, uint32_t in_ch, uint32_t out_ch,
		Load load)
{
#pragma unroll
	for (uint32_t o = 0; o < MO; o++)
#pragma unroll
		for (uint32_t w = 0; w < W; w++)
			acc[o][w] = 0u; // +0.0 / 0: the value of a row without a non-zero coefficient
	uint32_t started = 0; // bit o: output channel o has its first contribution
	for (uint32_t c = 0; c < in_ch; c++) {
		bool any = false;
#pragma unroll
		for (uint32_t o = 0; o < MO; o++)
			if (o < out_ch)
				any |= coef[o * in_ch + c] != 0.0f;
		if (!any)
			continue;
		uint32_t x[W];
		load(c, x);
#pragma unroll
		for (uint32_t o = 0; o < MO; o++) {
			if (o >= out_ch)
				continue;
			const float k = coef[o * in_ch + c];
			if (k == 0.0f)
				continue;
			const bool first = !((started >> o) & 1u);
			started |= 1u << o;
			if (k == 1.0f) {
				if (first) {
#pragma unroll
					for (uint32_t w = 0; w < W; w++)
						acc[o][w] = x[w];
				} else {
#pragma unroll
					for (uint32_t w = 0; w < W; w++)
						acc[o][w] = lw_mix_u(lw_mix_f(acc[o][w]) + lw_mix_f(x[w]));
				}
			} else if (first) {
#pragma unroll
				for (uint32_t w = 0; w < W; w++)
					acc[o][w] = lw_mix_u(k * lw_mix_f(x[w]));
			} else {
#pragma unroll
				for (uint32_t w = 0; w < W; w++) {
					const float t = k * lw_mix_f(x[w]);
					acc[o][w] = lw_mix_u(lw_mix_f(acc[o][w]) + t);
				}
			}
		}
	}
}

// The scalar way, W positions per lane and pass: any element size, any layout, any alignment.  The positions are the piece's
// [0, n) with a gap of `gap` positions opened at gap_at (the vector way's head and tail in one go; gap = 0: a whole piece).
template <int ES, bool ITL, uint32_t MO, uint32_t W>
__device__ __forceinline__ void lw_mix_span(const uint8_t *sp, uint8_t *dp, uint32_t n, uint32_t gap_at, uint32_t gap, uint32_t src_stride,
		uint64_t row_capacity, const float *__restrict__ coef, uint32_t in_ch, uint32_t out_ch, uint32_t lane)
{
	typedef typename LwMixElem<ES>::type E;
	const E *s = (const E *)sp;
	E *d = (E *)dp;
	const bool pair = ITL && ES == 4 && out_ch == 2u && ((uintptr_t)dp & 7u) == 0;
	const bool quad = ITL && ES == 4 && MO >= 4 && out_ch == 4u && ((uintptr_t)dp & 15u) == 0;
	for (uint32_t base = 0; base < n; base += 64u * W) {
		uint32_t pos[W]; // the lane's positions; >= its own index, so pos[w] is only used where on[w]
		bool on[W];
#pragma unroll
		for (uint32_t w = 0; w < W; w++) {
			const uint32_t i = base + w * 64u + lane;
			on[w] = i < n;
			pos[w] = i + (i >= gap_at ? gap : 0u);
		}
		uint32_t acc[MO][W];
		lw_mix_fold<MO, W>(acc, coef, in_ch, out_ch, [&](uint32_t c, uint32_t(&x)[W]) {
#pragma unroll
			for (uint32_t w = 0; w < W; w++) {
				const size_t e = ITL ? (size_t)pos[w] * in_ch + c : (size_t)c * src_stride + pos[w];
				x[w] = on[w] ? (uint32_t)s[e] : 0u;
			}
		});
		if (pair) {
#pragma unroll
			for (uint32_t w = 0; w < W; w++)
				if (on[w])
					((lw_mix_u32x2 *)__builtin_assume_aligned(dp, 8))[pos[w]] = lw_mix_u32x2{acc[0][w], acc[1][w]};
		} else if (quad) {
#pragma unroll
			for (uint32_t w = 0; w < W; w++)
				if (on[w])
					((lw_mix_u32x4 *)__builtin_assume_aligned(dp, 16))[pos[w]] =
						lw_mix_u32x4{acc[0][w], acc[1][w], acc[2 % MO][w], acc[3 % MO][w]};
		} else {
#pragma unroll
			for (uint32_t o = 0; o < MO; o++) {
				if (o >= out_ch)
					continue;
#pragma unroll
				for (uint32_t w = 0; w < W; w++) {
					const uint64_t e = ITL ? (uint64_t)pos[w] * out_ch + o : (uint64_t)o * row_capacity + pos[w];
					if (on[w])
						d[e] = (E)acc[o][w];
				}
			}
		}
	}
}

template <int ES, bool ITL, uint32_t MO> // element size in bytes; interleaved or planar; accumulators per position (>= out_ch)
__global__ void __launch_bounds__(64 * LW_MIX_WAVES) k_rows_mix(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst,
		const LwRowMixPiece *__restrict__ pieces, uint32_t n, const float *__restrict__ coef, uint32_t in_ch, uint32_t out_ch, uint64_t row_capacity)
{
	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); // wave-uniform: the descriptor comes in by scalar loads
	for (uint32_t q = blockIdx.x * LW_MIX_WAVES + wave; q < n; q += gridDim.x * LW_MIX_WAVES) {
		const LwRowMixPiece pc = pieces[q];
		const uint8_t *sp = src + (size_t)pc.src_elem * ES;
		uint8_t *dp = dst + (size_t)pc.dst_elem * ES; // 64-bit from the descriptor to the store address
		const uint32_t count = pc.count;
		if (ITL || ES != 4 || (row_capacity & 3u) != 0 || ((uintptr_t)dst & 15u) != 0) {
			lw_mix_span<ES, ITL, MO, LW_MIX_SPAN>(sp, dp, count, count, 0, pc.src_stride, row_capacity, coef, in_ch, out_ch, lane);
			continue;
		}
		// planar f32, every output channel aligned like channel 0: head | groups of four positions | tail
		constexpr uint32_t LW_MIX_GROUPS = MO > 2u ? 1u : 2u; // groups per lane and pass: 8 accumulators per output channel at most
		uint32_t head = (uint32_t)((16u - ((uintptr_t)dp & 15u)) & 15u) / 4u;
		head = head < count ? head : count;
		const uint32_t nvec = (count - head) / 4u;
		const uint8_t *vs = sp + (size_t)head * 4u;
		uint8_t *vd = dp + (size_t)head * 4u;
		for (uint32_t g0 = 0; g0 < nvec; g0 += 64u * LW_MIX_GROUPS) { // (one pass for a piece the host has cut)
			uint32_t acc[MO][4u * LW_MIX_GROUPS];
			lw_mix_fold<MO, 4u * LW_MIX_GROUPS>(acc, coef, in_ch, out_ch, [&](uint32_t c, uint32_t(&x)[4u * LW_MIX_GROUPS]) {
				const LwMixVec *cs = (const LwMixVec *)(vs + (size_t)c * pc.src_stride * 4u);
#pragma unroll
				for (uint32_t v = 0; v < LW_MIX_GROUPS; v++) {
					const uint32_t g = g0 + v * 64u + lane;
					const lw_mix_u32x4 t = g < nvec ? cs[g].v : lw_mix_u32x4{0, 0, 0, 0};
					x[4 * v] = t.x, x[4 * v + 1] = t.y, x[4 * v + 2] = t.z, x[4 * v + 3] = t.w;
				}
			});
#pragma unroll
			for (uint32_t o = 0; o < MO; o++) {
				if (o >= out_ch)
					continue;
				lw_mix_u32x4 *od = (lw_mix_u32x4 *)__builtin_assume_aligned(vd + (size_t)o * row_capacity * 4u, 16);
#pragma unroll
				for (uint32_t v = 0; v < LW_MIX_GROUPS; v++) {
					const uint32_t g = g0 + v * 64u + lane;
					if (g < nvec)
						od[g] = lw_mix_u32x4{acc[o][4 * v], acc[o][4 * v + 1], acc[o][4 * v + 2], acc[o][4 * v + 3]};
				}
			}
		}
		const uint32_t edges = count - nvec * 4u; // head + tail < 7 positions: one pass of one position per lane
		if (edges)
			lw_mix_span<ES, ITL, MO, 1u>(sp, dp, edges, head, nvec * 4u, pc.src_stride, row_capacity, coef, in_ch, out_ch, lane);
	}
}

hipError_t lw_launch_rows_mix(const void *d_src, void *d_dst, const LwRowMixPiece *d_pieces, uint32_t n_pieces, const float *d_coef,
		uint32_t in_ch, uint32_t out_ch, uint64_t row_capacity, int elem_size, bool interleaved, hipStream_t st)
{
	if (n_pieces == 0)
		return hipSuccess;
	if ((elem_size != 2 && elem_size != 4) || out_ch == 0 || out_ch > LW_ROWS_MIX_OUT || in_ch == 0)
		return hipErrorInvalidValue;
	const uint32_t groups = (n_pieces + LW_MIX_WAVES - 1) / LW_MIX_WAVES;
	const dim3 grid(groups < LW_MIX_MAX_GRID ? groups : LW_MIX_MAX_GRID), block(64 * LW_MIX_WAVES);
	const uint8_t *src = (const uint8_t *)d_src;
	uint8_t *dst = (uint8_t *)d_dst;
	const bool small = out_ch <= 2u; // mono and stereo rows: two accumulators per position, a quarter of the registers
#define LW_MIX_LAUNCH(ES, ITL, MO) lw_launch_k(k_rows_mix<ES, ITL, MO>, grid, block, 0, st, src, dst, d_pieces, n_pieces, d_coef, in_ch, out_ch, row_capacity)
	if (elem_size == 2) {
		if (interleaved)
			return small ? LW_MIX_LAUNCH(2, true, 2u) : LW_MIX_LAUNCH(2, true, LW_ROWS_MIX_OUT);
		return small ? LW_MIX_LAUNCH(2, false, 2u) : LW_MIX_LAUNCH(2, false, LW_ROWS_MIX_OUT);
	}
	if (interleaved)
		return small ? LW_MIX_LAUNCH(4, true, 2u) : LW_MIX_LAUNCH(4, true, LW_ROWS_MIX_OUT);
	return small ? LW_MIX_LAUNCH(4, false, 2u) : LW_MIX_LAUNCH(4, false, LW_ROWS_MIX_OUT);
#undef LW_MIX_LAUNCH
}
