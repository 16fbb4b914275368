// Inverse spectral frames of rows (product code, gfx950): k_istft, the kernel of lw_istft_rows.  A pass of its own over complex
// spectral frames [row][ch][2 B][frame] (what k_spec_complex writes: the re lines, then the im lines) -> rows of f32 PCM, by the
// rule of include/lewton_amd.h ("inverse spectral frames of rows"), bit for bit:
//   y_t[k] = fold over the 2 B source lines, l ascending, of fmaf(X[l][t], G[l][k], acc) from +0.0 -- one chain, never split
//   xh[p]  = fold over the frames t that touch p, t ascending, of acc + y_t[p - t hop - o] from +0.0 (one rounded f32 add each)
//   env[p] = the same fold in double of w2[p - t hop - o];  out[n] = (float)((double)xh[p] / env[p]) where p = n + pad < P and
//   env[p] > 1e-11, else +0.0.  The unit is compiled with -ffp-contract=off like all others.
//
// Work (lw_istft.hpp has the plan): a workgroup of 256 lanes OWNS m hop padded samples of one (row, channel) and computes the
// frame signals of the 32 frames from the first that touches them, the halo included, so that no sum crosses a workgroup: grid =
// (tiles, channels, rows).  The frame signals are a GEMM on v_mfma_f32_32x32x2_f32, whose result is a k-ordered fmaf chain:
//   pass   256 support samples at a time, from the HIGHEST k down: for a fixed p, ascending t is descending k, so what an earlier
//          pass adds to xh[p] comes from earlier frames than what a later one adds.  Wave w owns the samples [64 w, 64 w + 64) of
//          the pass as two 32 x 32 tiles (sample x frame), one accumulator each; a tile wholly behind win_length is skipped.
//   stage  per K tile of 16 source lines: the table tile [16][256] (one contiguous run of the device table, 16 bytes per load)
//          and the source tile [16][32 frames]: consecutive lanes on consecutive frames of a line, 128-byte runs, clamped
//          indices, the +0.0 of a line >= 2 B selected afterwards.  Banks: both operand reads are 32 consecutive words per
//          half-wave.
//   add    y of the pass goes to LDS as [sample][frame], rows 33 words apart; then lane i mod 256 of the owned span adds, for
//          its sample p, the frames the pass holds for it in ascending t (consecutive lanes read consecutive rows: bank
//          k + f mod 32).  xh lives in LDS; a sample is always the same lane's, so it needs no barrier of its own.
//   end    the envelope of a sample is folded on the fly from the device table of w2 (at most 17 doubles, consecutive lanes on
//          consecutive entries), then one double division and one rounding.  Frames >= T of a tile are computed from a copy of
//          the last one and never read.
// Route 1 (LW_IS_ROUTE_FMA) is the same body with the matrix instruction replaced by per-lane fmaf chains over the same LDS
// tiles and the same register layout: the fall-back, the second witness for the bits, and what tests/san/istft_host.cpp compiles
// for the host (LW_ISTFT_HOST) and runs lane by lane.
// Addresses: row, channel, line, frame and sample offsets are 64-bit from the arguments to the load and the store; everything
// else is 32-bit relative to the tile.  Plain vector loads and stores, no scratch, no atomics
// (profiles/rows_istft_resource_usage.txt).
#include "lw_istft.hpp"

#include "lw_lanes.hpp"
#ifndef LW_KERNEL_HOST
#include "lw_kernels.hpp"
#endif

struct LwIsTile { // what a workgroup works on; the same for all its lanes
	uint64_t T, out_len;
	uint64_t s0;   // first padded sample of the owned span
	uint64_t P;    // T == 0 ? 0 : n_fft + (T - 1) hop
	uint64_t tf0;  // first frame of the tile
	uint32_t nf;   // frames of the tile that exist: min(32, T - tf0), 0 when none does
	uint32_t span; // m hop
	int32_t r0;    // s0 - o - tf0 hop: sample i of the span sits at support sample r0 + i - f hop of the tile's frame f
	uint64_t s_at; // element of line 0, frame 0 of the source row and channel
	uint64_t d_at; // element of sample 0 of the destination row and channel
};

struct LwIsLane { // what a lane keeps in registers between the phases of its workgroup
	float acc[2][16]; // [tile][register]: sample = LW_MFMA32_ROW(register, lane), frame = lane & 31
};

LW_LANES_FN bool lw_is_tile(const LwIstftArgs &a, uint32_t bx, uint32_t by, uint32_t bz, LwIsTile &t)
{
	const LwIstftRow r = a.rows[(uint64_t)a.row0 + bz];
	t.T = r.frames, t.out_len = r.out_len;
	t.span = a.m * a.hop;
	t.s0 = ((uint64_t)a.tile0 + bx) * t.span;
	if (t.s0 >= a.pad + r.out_len)
		return false;
	t.P = r.frames == 0 ? 0 : (uint64_t)a.n_fft + (r.frames - 1u) * a.hop;
	// the first frame that touches the span: the least t >= 0 with t hop + o + W - 1 >= s0
	const int64_t lo = (int64_t)t.s0 - (int64_t)a.offset - (int64_t)a.win_length + 1;
	t.tf0 = lo <= 0 ? 0 : ((uint64_t)lo + a.hop - 1u) / a.hop;
	t.nf = r.frames > t.tf0 ? (uint32_t)(r.frames - t.tf0 < LW_IS_TF ? r.frames - t.tf0 : LW_IS_TF) : 0u;
	t.r0 = (int32_t)((int64_t)t.s0 - (int64_t)a.offset - (int64_t)(t.tf0 * a.hop));
	t.s_at = ((uint64_t)a.row0 + bz) * a.s_row + (uint64_t)by * a.s_ch;
	t.d_at = r.dst_row * a.d.row + (uint64_t)by * a.d.ch;
	return true;
}

// the tile's frames [f_lo, f_hi] whose support sample r - f hop lies in [klo, khi): false when there is none
LW_LANES_FN bool lw_is_range(const LwIstftArgs &a, const LwIsTile &t, int32_t r, uint32_t klo, uint32_t khi, uint32_t &f_lo, uint32_t &f_hi)
{
	if (t.nf == 0 || r < (int32_t)klo)
		return false;
	f_hi = (uint32_t)(r - (int32_t)klo) / a.hop;
	if (f_hi > t.nf - 1u)
		f_hi = t.nf - 1u;
	f_lo = r >= (int32_t)khi ? (uint32_t)(r - (int32_t)khi) / a.hop + 1u : 0u;
	return f_lo <= f_hi;
}

struct alignas(16) LwIsF4 {
	float v[4];
};

LW_LANES_FN void lw_is_zero_acc(LwIsLane &st)
{
#pragma unroll
	for (int i = 0; i < 2; i++)
#pragma unroll
		for (int r = 0; r < 16; r++)
			st.acc[i][r] = 0.0f;
}

// xh of the owned span from +0.0; sample i is lane i mod 256's in every phase
LW_LANES_FN void lw_is_zero_span(const LwIsTile &t, uint32_t tid, float *lds)
{
	for (uint32_t i = tid; i < t.span; i += LW_IS_THREADS)
		lds[LW_IS_LDS_H + i] = 0.0f;
}

// ---- stage: K tile kt of pass `pass` into LDS; all of a lane's loads are in flight before its first store
LW_LANES_FN void lw_is_stage(const LwIstftArgs &a, const LwIsTile &t, uint32_t pass, uint32_t kt, uint32_t tid, float *lds)
{
	const uint32_t l0 = kt * LW_IS_KT;
	const LwIsF4 *g = (const LwIsF4 *)(a.table + ((size_t)pass * a.l_pad + l0) * LW_IS_COLS);
	constexpr uint32_t NA = LW_IS_KT * LW_IS_COLS / 4u / LW_IS_THREADS; // 4
	constexpr uint32_t NX = LW_IS_KT * LW_IS_TF / LW_IS_THREADS;        // 2
	LwIsF4 va[NA];
	float vx[NX];
#pragma unroll
	for (uint32_t q = 0; q < NA; q++)
		va[q] = g[tid + q * LW_IS_THREADS];
#pragma unroll
	for (uint32_t q = 0; q < NX; q++) {
		const uint32_t e = tid + q * LW_IS_THREADS, f = e % LW_IS_TF, l = l0 + e / LW_IS_TF;
		const uint32_t lc = l < a.lines ? l : a.lines - 1u, fc = f < t.nf ? f : t.nf - 1u; // (nf >= 1 wherever a K loop runs)
		const float v = a.src[t.s_at + (uint64_t)lc * a.s_line + t.tf0 + fc];
		vx[q] = l < a.lines ? v : 0.0f;
	}
	LwIsF4 *as = (LwIsF4 *)(lds + LW_IS_LDS_A);
#pragma unroll
	for (uint32_t q = 0; q < NA; q++)
		as[tid + q * LW_IS_THREADS] = va[q];
#pragma unroll
	for (uint32_t q = 0; q < NX; q++)
		lds[LW_IS_LDS_X + tid + q * LW_IS_THREADS] = vx[q];
}

// which of a wave's two tiles hold a support sample at all
LW_LANES_FN bool lw_is_tile_live(const LwIstftArgs &a, uint32_t pass, uint32_t wave, uint32_t tt)
{
	return pass * LW_IS_COLS + wave * 64u + tt * 32u < a.win_length;
}

#ifndef LW_KERNEL_HOST
typedef float lw_is_f16 __attribute__((ext_vector_type(16)));
#endif

// ---- fold: the 16 source lines of the staged tile into the lane's accumulators, l ascending
template <int ROUTE> LW_LANES_FN void lw_is_mma(const LwIstftArgs &a, uint32_t pass, uint32_t tid, const float *lds, LwIsLane &st)
{
	const uint32_t lane = tid & 63u, wave = tid >> 6, f = lane & 31u;
	const float *as = lds + LW_IS_LDS_A + wave * 64u, *xs = lds + LW_IS_LDS_X;
#ifndef LW_KERNEL_HOST
	if (ROUTE == LW_IS_ROUTE_MFMA) {
		// A[i = lane & 31][k = lane >> 5] = G[line k][sample i], B[k = lane >> 5][j = lane & 31] = X[line k][frame j]: one f32 each
		const uint32_t h = lane >> 5;
#pragma unroll
		for (uint32_t tt = 0; tt < 2u; tt++) {
			if (!lw_is_tile_live(a, pass, wave, tt))
				continue;
			lw_is_f16 y;
#pragma unroll
			for (int r = 0; r < 16; r++)
				y[r] = st.acc[tt][r];
#pragma unroll
			for (uint32_t kk = 0; kk < LW_IS_KT; kk += 2u)
				y = __builtin_amdgcn_mfma_f32_32x32x2f32(as[(kk + h) * LW_IS_COLS + tt * 32u + f], xs[(kk + h) * LW_IS_TF + f], y, 0, 0, 0);
#pragma unroll
			for (int r = 0; r < 16; r++)
				st.acc[tt][r] = y[r];
		}
		return;
	}
#endif
#pragma unroll
	for (uint32_t tt = 0; tt < 2u; tt++) {
		if (!lw_is_tile_live(a, pass, wave, tt))
			continue;
		for (uint32_t kk = 0; kk < LW_IS_KT; kk++) {
			const float b = xs[kk * LW_IS_TF + f];
			const float *row = as + kk * LW_IS_COLS + tt * 32u;
#pragma unroll
			for (uint32_t r = 0; r < 16u; r++)
				st.acc[tt][r] = __builtin_fmaf(b, row[LW_MFMA32_ROW(r, lane)], st.acc[tt][r]);
		}
	}
}

// ---- y of the pass into LDS, [sample of the pass][frame]
LW_LANES_FN void lw_is_put_y(const LwIstftArgs &a, uint32_t pass, uint32_t tid, float *lds, const LwIsLane &st)
{
	const uint32_t lane = tid & 63u, wave = tid >> 6, f = lane & 31u;
#pragma unroll
	for (uint32_t tt = 0; tt < 2u; tt++) {
		if (!lw_is_tile_live(a, pass, wave, tt))
			continue;
#pragma unroll
		for (uint32_t r = 0; r < 16u; r++)
			lds[LW_IS_LDS_Y + (wave * 64u + tt * 32u + LW_MFMA32_ROW(r, lane)) * LW_IS_YS + f] = st.acc[tt][r];
	}
}

// ---- overlap-add: what the pass holds for each owned sample, t ascending, one rounded add each
LW_LANES_FN void lw_is_add(const LwIstftArgs &a, const LwIsTile &t, uint32_t pass, uint32_t tid, float *lds)
{
	const uint32_t k0 = pass * LW_IS_COLS, k1 = k0 + LW_IS_COLS < a.win_length ? k0 + LW_IS_COLS : a.win_length;
	for (uint32_t i = tid; i < t.span; i += LW_IS_THREADS) {
		const int32_t r = t.r0 + (int32_t)i;
		uint32_t f_lo, f_hi;
		if (!lw_is_range(a, t, r, k0, k1, f_lo, f_hi))
			continue;
		float acc = lds[LW_IS_LDS_H + i];
		for (uint32_t f = f_lo; f <= f_hi; f++)
			acc = acc + lds[LW_IS_LDS_Y + ((uint32_t)r - f * a.hop - k0) * LW_IS_YS + f];
		lds[LW_IS_LDS_H + i] = acc;
	}
}

// ---- end: envelope, division, store.  Exactly the samples n = p - pad in [0, out_len) of the span are written
LW_LANES_FN void lw_is_finish(const LwIstftArgs &a, const LwIsTile &t, uint32_t tid, const float *lds)
{
	for (uint32_t i = tid; i < t.span; i += LW_IS_THREADS) {
		const uint64_t p = t.s0 + i;
		if (p < a.pad || p - a.pad >= t.out_len)
			continue;
		const int32_t r = t.r0 + (int32_t)i;
		uint32_t f_lo, f_hi;
		double env = 0.0;
		if (lw_is_range(a, t, r, 0u, a.win_length, f_lo, f_hi))
			for (uint32_t f = f_lo; f <= f_hi; f++)
				env = env + a.w2[(uint32_t)r - f * a.hop];
		float v = 0.0f;
		if (p < t.P && env > 1e-11)
			v = (float)((double)lds[LW_IS_LDS_H + i] / env);
		a.dst[t.d_at + (p - a.pad) * a.d.el] = v;
	}
}

#ifndef LW_KERNEL_HOST

template <int ROUTE> __global__ void __launch_bounds__(LW_IS_THREADS) k_istft(LwIstftArgs a)
{
	extern __shared__ float lw_is_lds[];
	LwIsTile t;
	if (!lw_is_tile(a, blockIdx.x, blockIdx.y, blockIdx.z, t))
		return; // (the whole workgroup: the span is behind what its row writes)
	const uint32_t tid = threadIdx.x;
	LwIsLane st;
	lw_is_zero_span(t, tid, lw_is_lds);
	if (t.nf) // (uniform; without a frame every sample of the span is +0.0)
		for (uint32_t pass = a.passes; pass-- > 0u;) {
			lw_is_zero_acc(st);
			for (uint32_t kt = 0; kt < a.l_pad / LW_IS_KT; kt++) {
				lw_is_stage(a, t, pass, kt, tid, lw_is_lds);
				__syncthreads();
				lw_is_mma<ROUTE>(a, pass, tid, lw_is_lds, st);
				__syncthreads();
			}
			lw_is_put_y(a, pass, tid, lw_is_lds, st);
			__syncthreads();
			lw_is_add(a, t, pass, tid, lw_is_lds); // (the next pass's barriers stand between these reads and its y)
		}
	lw_is_finish(a, t, tid, lw_is_lds);
}

template <int ROUTE> static hipError_t lw_is_launch(const LwIstftArgs &a, dim3 grid, hipStream_t st)
{
	static LwPerDeviceOnce once; // above the default limit of dynamic LDS: per device, once
	const hipError_t e = once.run([] {
		return hipFuncSetAttribute((const void *)k_istft<ROUTE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(LW_IS_LDS_FLOATS * sizeof(float)));
	});
	if (e != hipSuccess)
		return e;
	return lw_launch_k(k_istft<ROUTE>, grid, dim3(LW_IS_THREADS), (size_t)LW_IS_LDS_FLOATS * sizeof(float), st, a);
}

hipError_t lw_launch_istft(const LwIstftArgs &a, int route, uint32_t tiles, uint32_t ch, uint32_t n_rows, hipStream_t st)
{
	if (tiles == 0 || n_rows == 0)
		return hipSuccess;
	// (m and hop index LDS: what the kernel trusts is checked here)
	if (ch == 0 || ch > 65535u || n_rows > 65535u || tiles > LW_IS_MAX_TILES || a.l_pad == 0 || a.l_pad % LW_IS_KT || a.lines > a.l_pad || a.lines == 0 ||
			a.hop == 0 || a.m == 0 || (uint64_t)a.m * a.hop > LW_IS_SPAN_MAX || a.win_length == 0 || a.hop > a.win_length ||
			a.m + (a.win_length + a.hop - 1u) / a.hop > LW_IS_TF || a.passes != (a.win_length + LW_IS_COLS - 1u) / LW_IS_COLS || !a.table || !a.w2)
		return hipErrorInvalidValue;
	const dim3 grid(tiles, ch, n_rows);
	if (route == LW_IS_ROUTE_MFMA)
		return lw_is_launch<LW_IS_ROUTE_MFMA>(a, grid, st);
	if (route == LW_IS_ROUTE_FMA)
		return lw_is_launch<LW_IS_ROUTE_FMA>(a, grid, st);
	return hipErrorInvalidValue;
}

#endif // LW_KERNEL_HOST
