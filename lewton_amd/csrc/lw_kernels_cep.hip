// Cepstra and deltas of feature rows (product code, gfx950): k_cep, the kernel of lw_cep_rows.  A pass of its own over f32
// [row][ch][n_in][capacity] rows by the rule of include/lewton_amd.h ("cepstra and deltas of feature rows"), bit for bit: the
// static lines are fmaf chains over the input lines (or a bit copy), the delta lines a regression filter along the frames of the
// static lines, the delta-delta lines the same filter of the delta lines, each with the index clamped into the row.  ONE launch:
// the source is read once and every destination line written once.
//   A workgroup of 256 lanes takes `tile` = 256 - 2 * order * width consecutive frames of one row and channel.  Lane i stands on
//   frame t0 - halo + i CLAMPED into the row and computes everything AT that clamped frame, so a halo lane beyond either end of
//   the row holds exactly what the contract's clamp refers to -- a value computed at the clamped index, not a neighbour's value
//   clamped after the fact.  A lane walks the input lines ascending over coalesced 4-byte loads; the matrix is stored transposed,
//   so that what up to 32 outputs need of one input line is contiguous and the same for every lane (scalar loads).  The outputs
//   are taken in groups of up to 32 accumulators (8, 16, 24 or 32, by what is left), so registers do not grow with n_out; a
//   later group re-reads its frames of the source from cache.  Per group: statics -> store, and into LDS [line][lane];
//   barrier; deltas of the lanes `width` and more from either end, out of LDS at the lanes of the clamped frames -> store, and
//   into a second image; barrier; delta-deltas of the tile's lanes -> store; barrier.  The fill with +0.0 goes with the stores.
// No atomics, no division (the weights arrive as arguments), offsets in 64 bits.  Nothing at or beyond n of a source line is
// read, nothing outside [0, fill_end) of a destination line written.  tests/san/cep_host.cpp compiles this file for the host
// (LW_CEP_HOST) and runs it workgroup by workgroup, the phases in the kernel's order.
#include "lw_cep.hpp"

#ifdef LW_KERNEL_HOST
#define LW_CP_LINE_DONE() (void)0
#else
#include "lw_kernels.hpp"
// Nothing is scheduled across the end of an input line's folds: left alone, the scheduler fetches the weights of all eight lines
// of a step at once, 256 scalar registers' worth, and spills them lane by lane into vector registers inside the loop.
#define LW_CP_LINE_DONE() asm volatile("" ::: "memory")
#endif

#define LW_CP_AHEAD 8u // input lines whose loads a lane issues before it folds them

struct LwCpTile { // what a workgroup works on; the same for all its lanes
	uint64_t n, end; // the row's n and fill_end
	int64_t first;   // the frame lane 0 stands on before clamping: t0 - halo
	uint64_t src_at; // element of line 0, frame 0 of the row and channel in the source
	uint64_t dst_at; // ... and in the destination
	bool data;       // the tile has frames below n: chains are computed; otherwise it only fills
};

// false: the tile lies at or beyond the row's fill_end, nothing to do
LW_LANES_FN bool lw_cp_tile(const LwCepArgs &a, uint32_t bx, uint32_t by, uint32_t bz, LwCpTile &t)
{
	const uint64_t row = (uint64_t)a.row0 + bz, t0 = (uint64_t)bx * a.plan.tile;
	const LwCepRow r = a.rows[row];
	t.n = r.n, t.end = r.fill_end;
	t.first = (int64_t)t0 - (int64_t)a.plan.halo;
	t.src_at = (row * a.ch + by) * a.n_in * a.line_el;
	t.dst_at = (row * a.ch + by) * ((uint64_t)a.n_out * (1u + a.order)) * a.line_el;
	t.data = t0 < r.n;
	return t0 < r.fill_end;
}

// the frame lane `tid` computes at (the tile has data, so n >= 1)
LW_LANES_FN int64_t lw_cp_frame(const LwCpTile &t, uint32_t tid)
{
	return lw_cep_clamp(t.first + (int64_t)tid, (int64_t)t.n);
}

// ---- the statics of G consecutive outputs from q0 at frame cs: s[j] = the chain over f ascending from +0.0, or the bit copy
template <int G>
LW_LANES_FN void lw_cp_static(const LwCepArgs &a, const LwCpTile &t, const float *LW_LANES_RESTRICT mt, const float *LW_LANES_RESTRICT src, uint32_t q0,
		uint32_t g, int64_t cs, float (&s)[G])
{
	const float *x = src + t.src_at + (uint64_t)cs;
	if (a.identity) {
#pragma unroll
		for (int j = 0; j < G; j++)
			s[j] = x[(uint64_t)(q0 + ((uint32_t)j < g ? (uint32_t)j : g - 1u)) * a.line_el]; // (at and beyond g: never stored)
		return;
	}
#pragma unroll
	for (int j = 0; j < G; j++)
		s[j] = 0.0f;
	const float *m = mt + q0; // (the padding of a row is +0.0: the accumulators at and beyond g are never stored)
	uint32_t f = 0;
	for (; f + LW_CP_AHEAD <= a.n_in; f += LW_CP_AHEAD) { // eight input lines' loads in flight per lane; the chains stay in order
		float xv[LW_CP_AHEAD];
#pragma unroll
		for (int u = 0; u < (int)LW_CP_AHEAD; u++, x += a.line_el)
			xv[u] = *x;
#pragma unroll
		for (int u = 0; u < (int)LW_CP_AHEAD; u++, m += a.mt_stride) {
#pragma unroll
			for (int j = 0; j < G; j++)
				s[j] = __builtin_fmaf(xv[u], m[j], s[j]);
			LW_CP_LINE_DONE();
		}
	}
	for (; f < a.n_in; f++, x += a.line_el, m += a.mt_stride) {
		const float xv = *x;
#pragma unroll
		for (int j = 0; j < G; j++)
			s[j] = __builtin_fmaf(xv, m[j], s[j]);
	}
}

// ---- a lane's values into its column of the LDS image [G][256]
template <int G>
LW_LANES_FN void lw_cp_put(float *img, uint32_t tid, const float (&v)[G])
{
#pragma unroll
	for (int j = 0; j < G; j++)
		img[(uint32_t)j * LW_CP_THREADS + tid] = v[j];
}

// does lane tid compute level `level` (1: delta, 2: delta-delta)?  The lanes level * width and more from either end
LW_LANES_FN bool lw_cp_has(const LwCepArgs &a, uint32_t level, uint32_t tid)
{
	return tid >= level * a.width && tid < LW_CP_THREADS - level * a.width;
}

// ---- the delta at frame cs of the G lines of the image: n ascending from +0.0; the neighbours are the lanes that stand on the
// clamped frames c(cs + n) and c(cs - n), which lie in the image (lw_cep.hpp, the tile plan)
template <int G>
LW_LANES_FN void lw_cp_delta(const LwCepArgs &a, const LwCpTile &t, const float *img, int64_t cs, float (&d)[G])
{
#pragma unroll
	for (int j = 0; j < G; j++)
		d[j] = 0.0f;
	for (uint32_t n = 1; n <= a.width; n++) {
		const uint32_t ia = (uint32_t)(lw_cep_clamp(cs + (int64_t)n, (int64_t)t.n) - t.first);
		const uint32_t ib = (uint32_t)(lw_cep_clamp(cs - (int64_t)n, (int64_t)t.n) - t.first);
		const float w = a.w[n - 1];
#pragma unroll
		for (int j = 0; j < G; j++)
			d[j] = lw_cep_delta_step(w, img[(uint32_t)j * LW_CP_THREADS + ia], img[(uint32_t)j * LW_CP_THREADS + ib], d[j]);
	}
}

// ---- the tile's lanes store lines q0 .. q0 + g - 1 of level `level` (0: statics) at their frame: the value below n, +0.0 in
// [n, fill_end), nothing beyond
template <int G>
LW_LANES_FN void lw_cp_store(const LwCepArgs &a, const LwCpTile &t, float *LW_LANES_RESTRICT dst, uint32_t q0, uint32_t g, uint32_t level, uint32_t tid,
		const float (&v)[G])
{
	if (tid < a.plan.halo || tid >= LW_CP_THREADS - a.plan.halo)
		return;
	const uint64_t f = (uint64_t)(t.first + (int64_t)tid); // (>= t0 >= 0)
	if (f >= t.end)
		return;
	const bool data = f < t.n;
	float *o = dst + t.dst_at + ((uint64_t)level * a.n_out + q0) * a.line_el + f;
#pragma unroll
	for (int j = 0; j < G; j++)
		if ((uint32_t)j < g)
			o[(uint64_t)j * a.line_el] = data ? v[j] : 0.0f;
}

#ifndef LW_KERNEL_HOST

// one group of outputs for one lane; every lane of the workgroup comes here (the barriers)
template <int G>
__device__ __forceinline__ void lw_cp_group(const LwCepArgs &a, const LwCpTile &t, const float *__restrict__ mt, const float *__restrict__ src,
		float *__restrict__ dst, float *lds, uint32_t q0, uint32_t g, uint32_t tid)
{
	float v[G];
	if (!t.data) { // (the whole workgroup: nothing below n in this tile)
#pragma unroll
		for (int j = 0; j < G; j++)
			v[j] = 0.0f;
		for (uint32_t level = 0; level <= a.order; level++)
			lw_cp_store<G>(a, t, dst, q0, g, level, tid, v);
		return;
	}
	const int64_t cs = lw_cp_frame(t, tid);
	lw_cp_static<G>(a, t, mt, src, q0, g, cs, v);
	lw_cp_store<G>(a, t, dst, q0, g, 0, tid, v);
	float *img = lds;
	for (uint32_t level = 1; level <= a.order; level++, img += a.plan.group * LW_CP_THREADS) {
		lw_cp_put<G>(img, tid, v);
		__syncthreads(); // the image of the level below is complete before anyone reads a neighbour's column
		if (lw_cp_has(a, level, tid)) {
			lw_cp_delta<G>(a, t, img, cs, v);
			lw_cp_store<G>(a, t, dst, q0, g, level, tid, v);
		}
	}
	if (a.order)
		__syncthreads(); // ... and read to the end before the next group overwrites it
}

__global__ void __launch_bounds__(LW_CP_THREADS) k_cep(LwCepArgs a, const float *__restrict__ mt, const float *__restrict__ src, float *__restrict__ dst)
{
	extern __shared__ __attribute__((aligned(16))) float lw_cp_lds[];
	LwCpTile t;
	if (!lw_cp_tile(a, blockIdx.x, blockIdx.y, blockIdx.z, t))
		return;
	for (uint32_t q0 = 0; q0 < a.n_out; q0 += LW_CP_GROUP) { // (the same trip count and the same branch in every lane)
		const uint32_t left = a.n_out - q0, g = left < LW_CP_GROUP ? left : LW_CP_GROUP;
		if (g > 24u)
			lw_cp_group<32>(a, t, mt, src, dst, lw_cp_lds, q0, g, threadIdx.x);
		else if (g > 16u)
			lw_cp_group<24>(a, t, mt, src, dst, lw_cp_lds, q0, g, threadIdx.x);
		else if (g > 8u)
			lw_cp_group<16>(a, t, mt, src, dst, lw_cp_lds, q0, g, threadIdx.x);
		else
			lw_cp_group<8>(a, t, mt, src, dst, lw_cp_lds, q0, g, threadIdx.x);
	}
}

hipError_t lw_launch_cep(const LwCepArgs &a, const float *mt, const float *src, float *dst, uint32_t tiles, uint32_t n_rows, hipStream_t st)
{
	const LwCepPlan p = lw_cep_plan(a.n_out, a.order, a.width);
	if (n_rows == 0 || n_rows > 65535u || a.ch == 0 || a.ch > 65535u || tiles == 0 || tiles > LW_CP_MAX_TILES || !a.rows || !dst || a.n_in == 0 ||
			a.n_out == 0 || a.order > 2u || a.width > LW_CP_MAX_WIDTH || (a.order != 0) != (a.width != 0) || (a.identity ? a.n_in != a.n_out : !mt) ||
			a.mt_stride < ((a.n_out + LW_CP_GROUP - 1u) & ~(LW_CP_GROUP - 1u)) || p.halo != a.plan.halo || p.tile != a.plan.tile ||
			p.group != a.plan.group || p.lds != a.plan.lds)
		return hipErrorInvalidValue;
	return lw_launch_k(k_cep, dim3(tiles, a.ch, n_rows), dim3(LW_CP_THREADS), (size_t)a.plan.lds, st, a, mt, src, dst);
}

#endif // LW_KERNEL_HOST
