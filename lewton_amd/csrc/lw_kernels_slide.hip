// Sliding-window normalisation of feature rows (product code, gfx950): k_slide, the kernel of lw_slide_rows.  A pass of its own
// from f32 [row][ch][F][frame_capacity] rows to rows of the same shape by the rule of include/lewton_amd.h ("sliding-window
// normalisation of feature rows"), bit for bit: every frame minus the mean of its window, optionally over the window's deviation,
// the window sums folded in the contract's order from block sums of 16 frames.  ONE launch.
//   A workgroup of 256 lanes takes `tile` consecutive frames of up to `lines` feature lines of one row and channel (lw_slide.hpp,
//   the tile plan).
//   fill    +0.0 into the tile's share of [T, fill_end); depends on no image and goes first.
//   load    frames [lo, hi) of every line -- the windows of the tile's frames, lo rounded down to a block boundary -- into the
//           LDS image as floats, lanes along the frames (coalesced 4-byte loads; element i at dword i + i / 32).
//   blocks  one lane per (line, block of 16 frames that lies wholly in [lo, hi)): A_b and Q_b, sixteen rounded double adds each,
//           into LDS as doubles.  The lanes of a 32-lane half read floats 16 apart: the skew puts them on 32 different banks.
//   apply   consecutive lanes on consecutive frames: rule 1 for the frame, then per line ONE accumulator over the head elements,
//           the block sums and the tail elements (rule 3), rule 4, and one 4-byte store.  A frame's window is the same for
//           every line, so a lane runs the chains of four lines side by side: each chain is a string of dependent double adds
//           behind LDS loads, and four of them (and the unrolled steps' loads) are what keeps the lane busy.  Head and tail
//           reads of neighbouring lanes are neighbouring dwords; sixteen neighbouring lanes read the same block sum (a broadcast).
// Every owned element is written once, by coalesced 4-byte stores (a wave writes 256 consecutive bytes).  No atomics, no wait of
// a workgroup on another, offsets in 64 bits.  Nothing at or beyond n of a source line is read, nothing outside [0, fill_end) of
// a destination line written.  tests/san/slide_host.cpp compiles this file for the host (LW_SLIDE_HOST) and runs it workgroup by
// workgroup, the phases in the kernel's order.
#include "lw_slide.hpp"

#ifndef LW_KERNEL_HOST
#include "lw_kernels.hpp"
#endif

#define LW_SL_AT(i) ((i) + ((i) >> 5)) // the dword of element i of an image line

struct LwSlTile { // what a workgroup works on; the same for all its lanes
	uint64_t n;       // the row's T
	uint64_t t0;      // first frame of the tile
	uint32_t nt;      // frames of the tile below T (0: the tile only fills)
	uint32_t fill_lo, fill_hi; // frames [t0 + fill_lo, t0 + fill_hi) of the tile receive +0.0
	uint64_t lo;      // the frame of the image's column 0: a multiple of 16
	uint32_t len;     // frames of the image: hi - lo <= plan.cols
	uint32_t G;       // lines of this group
	uint64_t at;      // element of frame 0 of the group's first line in source and destination
};

// false: the tile lies at or beyond the row's fill_end, nothing to do
LW_LANES_FN bool lw_sl_tile(const LwSlideArgs &a, uint32_t bx, uint32_t by, uint32_t bz, LwSlTile &t)
{
	const uint64_t row = (uint64_t)a.row0 + bz;
	const LwSlideRow r = a.rows[row];
	const uint32_t grp = bx % a.groups, f0 = grp * a.plan.lines;
	t.n = r.n, t.t0 = (uint64_t)(bx / a.groups) * a.plan.tile;
	if (t.t0 >= r.fill_end)
		return false;
	const uint64_t end = t.t0 + a.plan.tile;
	t.nt = t.t0 < r.n ? (uint32_t)((end < r.n ? end : r.n) - t.t0) : 0u;
	t.fill_lo = t.nt; // (n <= fill_end, so the fill starts where the data ends, or at the tile's start)
	t.fill_hi = (uint32_t)((end < r.fill_end ? end : r.fill_end) - t.t0);
	t.G = a.F - f0 < a.plan.lines ? a.F - f0 : a.plan.lines;
	t.at = ((row * a.ch + by) * a.F + f0) * a.line_el;
	t.lo = 0, t.len = 0;
	if (t.nt) {
		int64_t s, e, s1, e1;
		lw_slide_window_value(a.W, a.min_window, a.center, t.t0, r.n, s, e);
		lw_slide_window_value(a.W, a.min_window, a.center, t.t0 + t.nt - 1u, r.n, s1, e1);
		t.lo = (uint64_t)s & ~(uint64_t)(LW_SL_BLOCK - 1u);
		t.len = (uint32_t)((uint64_t)e1 - t.lo);
	}
	return true;
}

// ---- +0.0 into frames [fill_lo, fill_hi) of the tile, every line of the group
LW_LANES_FN void lw_sl_fill(const LwSlideArgs &a, const LwSlTile &t, float *LW_LANES_RESTRICT dst, uint32_t tid)
{
	for (uint32_t g = 0; g < t.G; g++) {
		float *y = dst + t.at + (uint64_t)g * a.line_el + t.t0;
		for (uint32_t i = t.fill_lo + tid; i < t.fill_hi; i += LW_SL_THREADS)
			y[i] = 0.0f;
	}
}

// ---- frames [lo, lo + len) of the group's lines into the image
LW_LANES_FN void lw_sl_load(const LwSlideArgs &a, const LwSlTile &t, const float *LW_LANES_RESTRICT src, float *xf, uint32_t tid)
{
	for (uint32_t g = 0; g < t.G; g++) {
		const float *x = src + t.at + (uint64_t)g * a.line_el + t.lo;
		float *img = xf + g * a.plan.pitch;
		for (uint32_t i = tid; i < t.len; i += LW_SL_THREADS)
			img[LW_SL_AT(i)] = x[i];
	}
}

// ---- rule 2 for the blocks that lie wholly in the image: bs[(2 g + 0) * nb + b] = A, bs[(2 g + 1) * nb + b] = Q
template <bool NV>
LW_LANES_FN void lw_sl_blocks(const LwSlideArgs &a, const LwSlTile &t, const float *xf, double *bs, uint32_t tid)
{
	const uint32_t nbk = t.len / LW_SL_BLOCK, items = t.G * nbk;
	for (uint32_t it = tid; it < items; it += LW_SL_THREADS) {
		const uint32_t g = it / nbk, b = it - g * nbk;
		const float *img = xf + g * a.plan.pitch;
		double A = 0.0, Q = 0.0;
#pragma unroll
		for (uint32_t i = 0; i < LW_SL_BLOCK; i++) {
			const double d = (double)img[LW_SL_AT(b * LW_SL_BLOCK + i)];
			A = A + d;
			if (NV)
				Q = Q + d * d;
		}
		bs[(2u * g) * a.plan.nb + b] = A;
		if (NV)
			bs[(2u * g + 1u) * a.plan.nb + b] = Q;
	}
}

// ---- rules 3 and 4 for one frame of NL lines at once: the lines' accumulators are independent chains with the same terms, so
// NL loads are in flight for every step of a chain (the order of every line's additions is the contract's)
template <bool NV, int NL>
LW_LANES_FN void lw_sl_frame(const LwSlideArgs &a, const float *img, const double *Ab, float *LW_LANES_RESTRICT y, uint32_t ls, uint32_t le, uint32_t at,
		uint64_t n)
{
	const uint32_t b0 = (ls + LW_SL_BLOCK - 1u) / LW_SL_BLOCK, b1 = le / LW_SL_BLOCK;
	const uint32_t head = b0 < b1 ? b0 * LW_SL_BLOCK : le, tail = b0 < b1 ? b1 * LW_SL_BLOCK : le;
	const uint32_t pitch = a.plan.pitch, nb2 = 2u * a.plan.nb;
	double S[NL], Q[NL];
#pragma unroll
	for (int l = 0; l < NL; l++)
		S[l] = 0.0, Q[l] = 0.0;
#pragma unroll 2
	for (uint32_t k = ls; k < head; k++) {
#pragma unroll
		for (int l = 0; l < NL; l++) {
			const double d = (double)img[(uint32_t)l * pitch + LW_SL_AT(k)];
			S[l] = S[l] + d;
			if (NV)
				Q[l] = Q[l] + d * d;
		}
	}
	if (b0 < b1) {
#pragma unroll 4
		for (uint32_t b = b0; b < b1; b++) {
#pragma unroll
			for (int l = 0; l < NL; l++) {
				S[l] = S[l] + Ab[(uint32_t)l * nb2 + b];
				if (NV)
					Q[l] = Q[l] + Ab[(uint32_t)l * nb2 + a.plan.nb + b];
			}
		}
#pragma unroll 2
		for (uint32_t k = tail; k < le; k++) {
#pragma unroll
			for (int l = 0; l < NL; l++) {
				const double d = (double)img[(uint32_t)l * pitch + LW_SL_AT(k)];
				S[l] = S[l] + d;
				if (NV)
					Q[l] = Q[l] + d * d;
			}
		}
	}
#pragma unroll
	for (int l = 0; l < NL; l++)
		y[(uint64_t)l * a.line_el] = lw_slide_value(NV, img[(uint32_t)l * pitch + LW_SL_AT(at)], S[l], Q[l], n);
}

// ---- rules 1, 3 and 4 for the tile's frames: consecutive lanes on consecutive frames, the group's lines four, two or one at a time
template <bool NV>
LW_LANES_FN void lw_sl_apply(const LwSlideArgs &a, const LwSlTile &t, const float *xf, const double *bs, float *LW_LANES_RESTRICT dst, uint32_t tid)
{
	for (uint32_t i = tid; i < t.nt; i += LW_SL_THREADS) {
		int64_t s, e;
		lw_slide_window_value(a.W, a.min_window, a.center, t.t0 + i, t.n, s, e);
		const uint32_t ls = (uint32_t)((uint64_t)s - t.lo), le = (uint32_t)((uint64_t)e - t.lo), at = (uint32_t)(t.t0 + i - t.lo);
		const uint64_t n = (uint64_t)(e - s);
		float *y = dst + t.at + t.t0 + i;
		uint32_t g = 0;
		for (; g + 4u <= t.G; g += 4u)
			lw_sl_frame<NV, 4>(a, xf + g * a.plan.pitch, bs + (2u * g) * a.plan.nb, y + (uint64_t)g * a.line_el, ls, le, at, n);
		if (g + 2u <= t.G) {
			lw_sl_frame<NV, 2>(a, xf + g * a.plan.pitch, bs + (2u * g) * a.plan.nb, y + (uint64_t)g * a.line_el, ls, le, at, n);
			g += 2u;
		}
		if (g < t.G)
			lw_sl_frame<NV, 1>(a, xf + g * a.plan.pitch, bs + (2u * g) * a.plan.nb, y + (uint64_t)g * a.line_el, ls, le, at, n);
	}
}

#ifndef LW_KERNEL_HOST

template <bool NV>
__global__ void __launch_bounds__(LW_SL_THREADS) k_slide(LwSlideArgs a, const float *__restrict__ src, float *__restrict__ dst)
{
	extern __shared__ __attribute__((aligned(16))) double lw_sl_lds[];
	LwSlTile t;
	if (!lw_sl_tile(a, blockIdx.x, blockIdx.y, blockIdx.z, t))
		return;
	double *bs = lw_sl_lds;
	float *xf = (float *)(bs + 2u * a.plan.lines * a.plan.nb);
	if (t.fill_hi > t.fill_lo)
		lw_sl_fill(a, t, dst, threadIdx.x);
	if (!t.nt)
		return;
	lw_sl_load(a, t, src, xf, threadIdx.x);
	__syncthreads();
	lw_sl_blocks<NV>(a, t, xf, bs, threadIdx.x);
	__syncthreads();
	lw_sl_apply<NV>(a, t, xf, bs, dst, threadIdx.x);
}

hipError_t lw_launch_slide(const LwSlideArgs &a, const float *src, float *dst, uint32_t tiles, uint32_t n_rows, hipStream_t st)
{
	LwSlidePlan p;
	if (n_rows == 0 || n_rows > 65535u || a.ch == 0 || a.ch > 65535u || tiles == 0 || !a.rows || !dst || a.F == 0 || a.W == 0 ||
			a.W > LW_SL_MAX_WINDOW || a.min_window == 0 || a.min_window > a.W || !lw_slide_plan(a.F, a.W, a.plan.tile, p) || p.cols != a.plan.cols ||
			p.pitch != a.plan.pitch || p.nb != a.plan.nb || p.lines != a.plan.lines || p.lds != a.plan.lds || p.lds > LW_SL_LDS_BUDGET ||
			a.groups != (a.F + p.lines - 1u) / p.lines || (uint64_t)tiles * a.groups > LW_SL_MAX_TILES)
		return hipErrorInvalidValue;
	const dim3 grid(tiles * a.groups, a.ch, n_rows);
	if (a.norm_vars)
		return lw_launch_k(k_slide<true>, grid, dim3(LW_SL_THREADS), (size_t)p.lds, st, a, src, dst);
	return lw_launch_k(k_slide<false>, grid, dim3(LW_SL_THREADS), (size_t)p.lds, st, a, src, dst);
}

#endif // LW_KERNEL_HOST
