// Row resampler (product code, gfx950): k_resample, the kernel of lw_resample_rows.  A pass of its own over finished rows
// ([row][ch][sample] or [row][sample][ch], f32): every output sample is a K-tap polyphase fold of its row and channel by the rule
// of include/lewton_amd.h ("resampling rows"), bit for bit:
//   n -> base = floor(n * orig / new), ph = (n * orig) mod new;  y[n] = h[ph][0] * x[base - W] (+) h[ph][1] * x[base - W + 1] (+) ...
//   taps in ascending k, every product one rounded f32 multiply, every (+) one rounded f32 add, the first product is the
//   accumulator; x = +0.0 outside [0, len).  The unit is compiled with -ffp-contract=off like all others: no multiply is fused.
//
// Work: a tile = J runs of U = M * new consecutive outputs of one (row, channel), one workgroup of 512 lanes per tile, grid =
// (tiles, channels, rows).  A tile starts at a multiple of new, so its first output has phase 0 and base (n / new) * orig exactly;
// everything behind that is 32-bit arithmetic relative to the tile, the 64-bit part is done once per workgroup.
//   stage  the tile's input span, M * J * orig + K - 1 samples from base - W on, goes to LDS, +0.0 where the row has no sample
//          (i < 0, i >= len: loads go to a clamped index, so what the source holds between len and its capacity is never
//          fetched), eight independent loads in flight per lane; on route LDS the tap table too, 16 bytes at a time.
//   fold   a lane owns the outputs n, n + U, ..., n + (J - 1) * U: ONE phase (U is a multiple of new), inputs M * orig apart.  Per
//          tap it reads h once and keeps it in a register for its J multiplies -- 1 + 1 / J LDS reads per multiply-add pair
//          instead of 2.  The table is stored [k][n mod new] (the host permutes the phases, lw_resample.cpp), so consecutive
//          lanes read consecutive words: no bank conflict on the taps and coalesced loads on the global-taps route.  Consecutive
//          lanes take consecutive outputs, so their x reads are orig / new words apart: 3 at 3 -> 1 (odd: conflict-free),
//          broadcasts when up-sampling, a 2- to 3-way bank conflict at 441 -> 160 (ds_read_b32, 32 banks).
// Routes (lw_resample.hpp): table + span in LDS | span in LDS, taps from global memory (L2) when the table does not fit the
// workgroup's 80 KiB | both from global memory when not even one block's span fits (orig in the thousands) | orig == new: a copy.
// All routes run the same fold in the same order, so they give the same bits.
// Addresses: row, channel and sample offsets are 64-bit from the arguments to the load and the store.  Plain vector loads and
// stores, no scratch (profiles/rows_resample_resource_usage.txt).
//
// The bodies below are written per lane and per phase of the workgroup (stage | barrier | fold) and take the lane's coordinates as
// arguments, so tests/san/resample_host.cpp compiles this file for the host (LW_RESAMPLE_HOST) and runs it lane by lane.
#include "lw_resample.hpp"

#include "lw_lanes.hpp"
#ifndef LW_KERNEL_HOST
#include "lw_kernels.hpp"
#endif

struct LwRsTile { // what a workgroup works on; the same for all its lanes
	uint64_t len, out_len;
	uint64_t n0;   // first output of the tile, a multiple of new
	int64_t x0;    // input sample at index 0 of the span: base(n0) - W
	uint64_t s_at; // element of sample 0 of the source row and channel
	uint64_t d_at; // ... of the destination row and channel
};

LW_LANES_FN bool lw_rs_tile(const LwResampleArgs &a, uint32_t tile_outputs, uint32_t bx, uint32_t by, uint32_t bz, LwRsTile &t)
{
	const LwResampleRow r = a.rows[(uint64_t)a.row0 + bz];
	t.len = r.len, t.out_len = r.out_len;
	t.n0 = ((uint64_t)a.tile0 + bx) * tile_outputs;
	if (t.n0 >= r.out_len)
		return false;
	t.x0 = (int64_t)(t.n0 / a.new_ * a.orig) - (int64_t)a.half_width; // (route GLOBAL does not use it)
	t.s_at = ((uint64_t)a.row0 + bz) * a.s.row + (uint64_t)by * a.s.ch;
	t.d_at = r.dst_row * a.d.row + (uint64_t)by * a.d.ch;
	return true;
}

// x[i] of the tile's row and channel, +0.0 outside [0, len): the load goes to a clamped index (len >= 1 wherever a tile exists), so
// it is branch-free, never leaves [0, len), and what lies between len and the capacity is never fetched
LW_LANES_FN float lw_rs_x(const LwResampleArgs &a, const LwRsTile &t, int64_t i)
{
	const bool in = i >= 0 && (uint64_t)i < t.len;
	const uint64_t c = i < 0 ? 0 : (uint64_t)i < t.len ? (uint64_t)i : t.len - 1;
	const float v = a.src[t.s_at + c * a.s.el];
	return in ? v : 0.0f;
}

struct alignas(16) LwRsF4 {
	float v[4];
};

// ---- stage: span (and table) into LDS; lds = [span][new * K]; eight independent loads in flight per lane
template <int ROUTE> LW_LANES_FN void lw_rs_stage(const LwResampleArgs &a, const LwRsTile &t, uint32_t span, uint32_t tid, uint32_t nthreads, float *lds)
{
	for (uint32_t s0 = tid; s0 < span; s0 += 8u * nthreads) {
		float v[8];
#pragma unroll
		for (uint32_t q = 0; q < 8u; q++) {
			const uint32_t s = s0 + q * nthreads;
			v[q] = lw_rs_x(a, t, t.x0 + (int64_t)(s < span ? s : span - 1u));
		}
#pragma unroll
		for (uint32_t q = 0; q < 8u; q++) {
			const uint32_t s = s0 + q * nthreads;
			if (s < span)
				lds[s] = v[q];
		}
	}
	if (ROUTE == LW_RS_ROUTE_LDS) {
		LwRsF4 *hs = (LwRsF4 *)(lds + span); // span is a multiple of four floats, the table padded to one
		const LwRsF4 *g = (const LwRsF4 *)a.taps;
		const uint32_t n = (a.new_ * a.k_taps + 3u) / 4u;
		for (uint32_t i0 = tid; i0 < n; i0 += 4u * nthreads) {
			LwRsF4 v[4];
#pragma unroll
			for (uint32_t q = 0; q < 4u; q++) {
				const uint32_t i = i0 + q * nthreads;
				v[q] = g[i < n ? i : n - 1u];
			}
#pragma unroll
			for (uint32_t q = 0; q < 4u; q++) {
				const uint32_t i = i0 + q * nthreads;
				if (i < n)
					hs[i] = v[q];
			}
		}
	}
}

// A tile is J runs of U = M * new consecutive outputs; unit u of it = the outputs n, n + U, ..., n + (J - 1) * U with n = n0 + u.
// U is a multiple of new, so they share n mod new (which selects the taps) and their inputs lie M * orig apart.  Returns n, its
// n mod new and the index of x[base(n) - W] in the span.  Consecutive lanes take consecutive outputs: their x reads are
// orig / new words apart.
LW_LANES_FN uint64_t lw_rs_unit(const LwResampleArgs &a, const LwRsTile &t, uint32_t u, uint32_t &i, uint32_t &x_at)
{
	const uint32_t m = u / a.new_;
	i = u - m * a.new_;
	x_at = m * a.orig + (uint32_t)((uint64_t)i * a.orig / a.new_); // i * orig < new * orig <= 2^29: new * K <= 65536, K > 2 * orig / new
	return t.n0 + u;
}

// ---- fold: J outputs of one phase per lane and pass
template <int ROUTE, int J> LW_LANES_FN void lw_rs_fold(const LwResampleArgs &a, const LwRsTile &t, uint32_t span, uint32_t tid, uint32_t nthreads, const float *lds)
{
	const uint32_t nw = a.new_, K = a.k_taps;
	const float *hs = ROUTE == LW_RS_ROUTE_LDS ? lds + span : a.taps;
	const uint32_t units = a.blocks * nw, run = a.blocks * a.orig; // outputs / inputs from one of a lane's J outputs to the next
	for (uint32_t u = tid; u < units; u += nthreads) {
		uint32_t i, x_at;
		const uint64_t n = lw_rs_unit(a, t, u, i, x_at);
		if (n >= t.out_len)
			break;
		const float *x = lds + x_at;
		const float *h = hs + i;
		float acc[J];
		{
			const float h0 = h[0];
#pragma unroll
			for (int j = 0; j < J; j++)
				acc[j] = h0 * x[j * run];
		}
#pragma unroll 4
		for (uint32_t k = 1; k < K; k++) {
			const float hk = h[(size_t)k * nw];
#pragma unroll
			for (int j = 0; j < J; j++) {
				const float p = hk * x[j * run + k];
				acc[j] = acc[j] + p;
			}
		}
#pragma unroll
		for (int j = 0; j < J; j++) {
			const uint64_t nj = n + (uint64_t)j * units;
			if (nj < t.out_len)
				a.dst[t.d_at + nj * a.d.el] = acc[j];
		}
	}
}

// ---- route GLOBAL: one output per lane, nothing staged (tile = nthreads outputs, any start)
LW_LANES_FN int64_t lw_rs_global_index(const LwResampleArgs &a, uint64_t n, uint32_t &i) // base(n) - W and n mod new
{
	const uint64_t q = n / a.new_;
	i = (uint32_t)(n - q * a.new_);
	return (int64_t)(q * a.orig + (uint64_t)i * a.orig / a.new_) - (int64_t)a.half_width;
}

LW_LANES_FN void lw_rs_fold_global(const LwResampleArgs &a, const LwRsTile &t, uint32_t tid)
{
	const uint64_t n = t.n0 + tid;
	if (n >= t.out_len)
		return;
	uint32_t i;
	const int64_t b = lw_rs_global_index(a, n, i);
	const float *h = a.taps + i;
	float acc = h[0] * lw_rs_x(a, t, b);
	for (uint32_t k = 1; k < a.k_taps; k++) {
		const float p = h[(size_t)k * a.new_] * lw_rs_x(a, t, b + (int64_t)k);
		acc = acc + p;
	}
	a.dst[t.d_at + n * a.d.el] = acc;
}

// ---- route COPY (orig == new): bits of [0, len), four per lane
LW_LANES_FN void lw_rs_copy(const LwResampleArgs &a, const LwRsTile &t, uint32_t tid, uint32_t nthreads)
{
	const uint32_t *s = (const uint32_t *)a.src;
	uint32_t *d = (uint32_t *)a.dst;
	for (uint32_t v = 0; v < 4u; v++) {
		const uint64_t n = t.n0 + v * nthreads + tid;
		if (n < t.out_len)
			d[t.d_at + n * a.d.el] = s[t.s_at + n * a.s.el];
	}
}

#ifndef LW_KERNEL_HOST

template <int ROUTE, int J> __global__ void __launch_bounds__(LW_RS_THREADS) k_resample(LwResampleArgs a, uint32_t span)
{
	extern __shared__ float lw_rs_lds[];
	LwRsTile t;
	if (ROUTE == LW_RS_ROUTE_COPY) {
		if (lw_rs_tile(a, LW_RS_THREADS * 4u, blockIdx.x, blockIdx.y, blockIdx.z, t))
			lw_rs_copy(a, t, threadIdx.x, LW_RS_THREADS);
	} else if (ROUTE == LW_RS_ROUTE_GLOBAL) {
		if (lw_rs_tile(a, LW_RS_THREADS, blockIdx.x, blockIdx.y, blockIdx.z, t))
			lw_rs_fold_global(a, t, threadIdx.x);
	} else {
		if (!lw_rs_tile(a, a.blocks * J * a.new_, blockIdx.x, blockIdx.y, blockIdx.z, t))
			return; // (the whole workgroup: the tile is behind its row's end)
		lw_rs_stage<ROUTE>(a, t, span, threadIdx.x, LW_RS_THREADS, lw_rs_lds);
		__syncthreads();
		lw_rs_fold<ROUTE, J>(a, t, span, threadIdx.x, LW_RS_THREADS, lw_rs_lds);
	}
}

template <int ROUTE, int J>
static hipError_t lw_rs_launch(const LwResampleArgs &a, const LwResamplePlan &p, dim3 grid, hipStream_t st)
{
	const size_t lds = (size_t)p.lds_floats * sizeof(float);
	if (lds > 48u * 1024u) { // above the default limit of dynamic LDS: per device, once
		static LwPerDeviceOnce once;
		const hipError_t e = once.run([] {
			return hipFuncSetAttribute((const void *)k_resample<ROUTE, J>, hipFuncAttributeMaxDynamicSharedMemorySize,
					(int)(LW_RS_LDS_FLOATS * sizeof(float)));
		});
		if (e != hipSuccess)
			return e;
	}
	return lw_launch_k(k_resample<ROUTE, J>, grid, dim3(LW_RS_THREADS), lds, st, a, p.span);
}

hipError_t lw_launch_resample(const LwResampleArgs &a, const LwResamplePlan &p, uint32_t tiles, uint32_t ch, uint32_t n_rows, hipStream_t st)
{
	if (tiles == 0 || n_rows == 0)
		return hipSuccess;
	if (ch == 0 || ch > 65535u || n_rows > 65535u || tiles > LW_RS_MAX_TILES || p.lds_floats > LW_RS_LDS_FLOATS || p.blocks != a.blocks)
		return hipErrorInvalidValue;
	const dim3 grid(tiles, ch, n_rows);
	switch (p.route) {
	case LW_RS_ROUTE_COPY:
		return lw_rs_launch<LW_RS_ROUTE_COPY, 1>(a, p, grid, st);
	case LW_RS_ROUTE_GLOBAL:
		return lw_rs_launch<LW_RS_ROUTE_GLOBAL, 1>(a, p, grid, st);
	case LW_RS_ROUTE_LDS:
		return p.j == 4 ? lw_rs_launch<LW_RS_ROUTE_LDS, 4>(a, p, grid, st)
			: p.j == 2 ? lw_rs_launch<LW_RS_ROUTE_LDS, 2>(a, p, grid, st)
			: lw_rs_launch<LW_RS_ROUTE_LDS, 1>(a, p, grid, st);
	case LW_RS_ROUTE_GLOBAL_TAPS:
		return p.j == 4 ? lw_rs_launch<LW_RS_ROUTE_GLOBAL_TAPS, 4>(a, p, grid, st)
			: p.j == 2 ? lw_rs_launch<LW_RS_ROUTE_GLOBAL_TAPS, 2>(a, p, grid, st)
			: lw_rs_launch<LW_RS_ROUTE_GLOBAL_TAPS, 1>(a, p, grid, st);
	}
	return hipErrorInvalidValue;
}

#endif // LW_KERNEL_HOST
