// Spectral frames of rows (product code, gfx950): k_spec, the kernel of lw_spec_rows.  A pass of its own over finished rows
// ([row][ch][sample] or [row][sample][ch], f32): overlapping frames of a row and channel -> power spectrum or mel features,
// [row][ch][F][frame], by the rule of include/lewton_amd.h ("spectral frames of rows"), bit for bit:
//   re[j] = fold over the window's support, k ascending, of fmaf(x_k, C[k][j], acc) from +0.0;  im[j] likewise with S
//   P[j]  = fmaf(im, im, re * re);  m[q] = fold over j = 0 .. B - 1 ascending of fmaf(P[j], fb[q][j], acc) from +0.0
//   x = +0.0 outside [0, len), or the reflected sample (LW_SPEC_PAD_REFLECT, lw_sp_reflect; LW_SPEC_PAD_SYMMETRIC, lw_sp_symmetric).
//   No chain is ever split; the unit is compiled with -ffp-contract=off like all others.
//   With remove_dc or energy (lw_spec_create_ex) a per-frame prologue runs first (lw_sp_pro_*, k_spec<.., .., 1>): x_k - mu
//   takes x_k's place in the chains, and the frame's energy goes to line 0.  Pre-emphasis, window and scale live in the table.
//
// Work: a tile = LW_SP_TF = 32 consecutive frames of one (row, channel), one workgroup of 256 lanes (four waves) per tile, grid =
// (tiles, channels, rows).  The framed DFT is a GEMM, D[bin][frame] = sum_k basis[k][bin] * x[frame * hop + k], run on
// v_mfma_f32_32x32x2_f32, whose result is a k-ordered fmaf chain: M = 32 bins (A operand, from the basis), N = 32 frames (B
// operand, from the row), so a result's frame is its lane (lane & 31) and stores run over consecutive frames.
//   pass   256 bins at a time (all of them up to n_fft = 510).  Wave w owns the columns [64 w, 64 w + 64) of the pass as two
//          32 x 32 tiles, each with a cosine and a sine accumulator -- four independent accumulators per wave, and re and im of one
//          (bin, frame) in the same lane and register.  Parallelism comes from output tiles only: one output's K loop stays in
//          one accumulator, ascending.  A tile wholly behind the last bin is skipped (wave-uniform).
//   stage  per K tile of 16 support samples: the basis tile [16][C | S][256] (one contiguous run of the device table, 16 bytes
//          per load, eight loads in flight per lane) and the FRAME tile [16][32 frames], laid out per frame in LDS: element
//          (k, f) = x[(f0 + f) * hop + lead + k], loaded with consecutive lanes on consecutive k (coalesced), clamped index,
//          the +0.0 selected afterwards.  The frame matrix exists only here, 2 KiB at a time; any hop up to 65535 costs the
//          same LDS.  Banks: operand reads are 32 consecutive words per half-wave in both tiles (conflict-free, ds_read_b32
//          serves lanes 0-31 and 32-63 separately); the frame tile's rows are 33 words apart so that the staging stores, which
//          run down a column, spread over the banks (2-way instead of 16-way).  hop never reaches an LDS address.
//   tails  k >= win_length: both operands are zeros (fmaf(0, 0, acc) = acc but for the sign of a zero, which is outside the
//          contract).  Bins >= B and frames >= n_frames of a tile are computed and never stored or read.
//   power  P of the pass goes to LDS as [bin][frame].  Without a mel matrix it is stored from there; with one, every lane keeps
//          the accumulators of ONE frame and up to 32 mel bands in registers over all passes and folds P[j] in ascending j, the
//          matrix slice [32 j][mel_pad] staged where the basis tile was (vector fmaf: a tenth of the arithmetic).
//   complex  (LW_SPEC_OUT_COMPLEX, k_spec_complex) re of the pass goes through the same LDS region to the lines [0, B), then im
//          to the lines [B, 2B): the accumulators as they are, P never formed.
// Route 1 (LW_SP_ROUTE_FMA) is the same body with the matrix instruction replaced by per-lane fmaf chains over the same LDS
// tiles and the same register layout: the fall-back, the second witness for the bits, and what tests/san/spec_host.cpp compiles
// for the host (LW_SPEC_HOST) and runs lane by lane.
// Addresses: row, channel and sample offsets are 64-bit from the arguments to the load and the store; everything else is
// 32-bit relative to the tile.  Plain vector loads and stores, no scratch (profiles/rows_spec_resource_usage.txt).
#include "lw_spec.hpp"

#include "lw_lanes.hpp"
#ifndef LW_KERNEL_HOST
#include "lw_kernels.hpp"
#endif

struct LwSpTile { // what a workgroup works on; the same for all its lanes
	uint64_t len, n_frames;
	uint64_t f0;   // first frame of the tile
	int64_t x0;    // input sample under support sample 0 of frame f0
	uint64_t s_at; // element of sample 0 of the source row and channel
	uint64_t d_at; // element of line 0, frame 0 of the destination row and channel
};

struct LwSpLane { // what a lane keeps in registers between the phases of its workgroup
	float acc[4][16]; // [2 * tile + sine][register]: bin = LW_MFMA32_ROW(register, lane), frame = lane & 31
	float mel[8][4];  // band 4 * ((tid >> 5) + 8 * b) + i of frame tid & 31
};

LW_LANES_FN bool lw_sp_tile(const LwSpecArgs &a, uint32_t bx, uint32_t by, uint32_t bz, LwSpTile &t)
{
	const LwSpecRow r = a.rows[(uint64_t)a.row0 + bz];
	t.len = r.len, t.n_frames = r.n_frames;
	t.f0 = ((uint64_t)a.tile0 + bx) * LW_SP_TF;
	if (t.f0 >= r.n_frames)
		return false;
	t.x0 = (int64_t)(t.f0 * a.hop) + a.lead;
	t.s_at = ((uint64_t)a.row0 + bz) * a.s.row + (uint64_t)by * a.s.ch;
	t.d_at = r.dst_row * a.d_row + (uint64_t)by * a.d_ch;
	return true;
}

// input index of support sample k of the tile's frame f
LW_LANES_FN int64_t lw_sp_index(const LwSpecArgs &a, const LwSpTile &t, uint32_t f, uint32_t k)
{
	return t.x0 + (int64_t)((uint64_t)f * a.hop) + (int64_t)k;
}

// where x[i] is read under reflect padding: i itself inside [0, len), -i below, 2 (len - 1) - i from len on, in 64-bit integers
// (one reflection: the host has refused rows for which a support sample would need a second one).  Selects, no branch
LW_LANES_FN int64_t lw_sp_reflect(const LwSpTile &t, int64_t i)
{
	const int64_t up = i < 0 ? -i : i;
	return (uint64_t)up >= t.len ? 2 * ((int64_t)t.len - 1) - up : up;
}

// x[i] of the tile's row and channel; outside [0, len) +0.0, or the reflected sample: the load goes to a clamped index (len >= 1
// wherever a tile exists), so it is branch-free, never leaves [0, len), and what lies between len and the capacity is never
// fetched.  PAD is the pad mode as a compile-time constant -- the kernel is instantiated per mode: a test of a.pad_mode here
// becomes a uniform branch between a lane's loads and ends their overlap -- or LW_SP_PAD_ARGS: as a.pad_mode says
// (the host programs, which call lw_sp_stage without it)
#define LW_SP_PAD_ARGS (-1)
// where x[i] is read under symmetric padding (LW_SPEC_PAD_SYMMETRIC, Kaldi's frames without snip_edges): the edge sample is
// repeated, -i - 1 below 0 and 2 len - 1 - i from len on (one reflection, as above)
LW_LANES_FN int64_t lw_sp_symmetric(const LwSpTile &t, int64_t i)
{
	const int64_t up = i < 0 ? -i - 1 : i;
	return (uint64_t)up >= t.len ? 2 * (int64_t)t.len - 1 - up : up;
}

template <int PAD> LW_LANES_FN float lw_sp_x(const LwSpecArgs &a, const LwSpTile &t, int64_t i)
{
	if (PAD == 1 || (PAD == LW_SP_PAD_ARGS && a.pad_mode == 1))
		i = lw_sp_reflect(t, i);
	if (PAD == 2 || (PAD == LW_SP_PAD_ARGS && a.pad_mode == 2))
		i = lw_sp_symmetric(t, i);
	const bool in = i >= 0 && (uint64_t)i < t.len;
	const uint64_t c = i < 0 ? 0 : (uint64_t)i < t.len ? (uint64_t)i : t.len - 1;
	const float v = a.src[t.s_at + c * a.s.el];
	return in ? v : 0.0f;
}

struct alignas(16) LwSpF4 {
	float v[4];
};

LW_LANES_FN void lw_sp_zero_acc(LwSpLane &st)
{
#pragma unroll
	for (int i = 0; i < 4; i++)
#pragma unroll
		for (int r = 0; r < 16; r++)
			st.acc[i][r] = 0.0f;
}

LW_LANES_FN void lw_sp_zero_mel(LwSpLane &st)
{
#pragma unroll
	for (int b = 0; b < 8; b++)
#pragma unroll
		for (int i = 0; i < 4; i++)
			st.mel[b][i] = 0.0f;
}

// ---- stage: K tile kt of pass `pass` into LDS; all of a lane's loads are in flight before its first store
// PRO (the per-frame prologue ran): x'_k = x_k - mu, one rounded subtraction, of the padded sample and before the tail's zeros;
// mu0 / mu1 are the means of the lane's two frames (lw_sp_pro_mu), +0.0 without remove_dc, which leaves every x as it is
template <int PAD = LW_SP_PAD_ARGS, int PRO = 0>
LW_LANES_FN void lw_sp_stage(const LwSpecArgs &a, const LwSpTile &t, uint32_t pass, uint32_t kt, uint32_t tid, float *lds, float mu0 = 0.0f, float mu1 = 0.0f)
{
	const uint32_t k0 = kt * LW_SP_KT;
	const LwSpF4 *g = (const LwSpF4 *)(a.basis + ((size_t)pass * a.k_pad + k0) * (2u * LW_SP_COLS));
	constexpr uint32_t NA = LW_SP_KT * 2u * LW_SP_COLS / 4u / LW_SP_THREADS; // 8
	constexpr uint32_t NX = LW_SP_KT * LW_SP_TF / LW_SP_THREADS;             // 2
	LwSpF4 va[NA];
	float vx[NX];
#pragma unroll
	for (uint32_t q = 0; q < NA; q++)
		va[q] = g[tid + q * LW_SP_THREADS];
#pragma unroll
	for (uint32_t q = 0; q < NX; q++) {
		const uint32_t e = tid + q * LW_SP_THREADS, kk = e % LW_SP_KT, f = e / LW_SP_KT;
		float v = lw_sp_x<PAD>(a, t, lw_sp_index(a, t, f, k0 + kk));
		if (PRO)
			v = v - (q ? mu1 : mu0);
		vx[q] = k0 + kk < a.win_length ? v : 0.0f;
	}
	LwSpF4 *as = (LwSpF4 *)(lds + LW_SP_LDS_A);
#pragma unroll
	for (uint32_t q = 0; q < NA; q++)
		as[tid + q * LW_SP_THREADS] = va[q];
#pragma unroll
	for (uint32_t q = 0; q < NX; q++) {
		const uint32_t e = tid + q * LW_SP_THREADS, kk = e % LW_SP_KT, f = e / LW_SP_KT;
		lds[LW_SP_LDS_X + kk * LW_SP_XS + f] = vx[q];
	}
}

// which of a wave's two tiles hold a bin at all
LW_LANES_FN bool lw_sp_tile_live(const LwSpecArgs &a, uint32_t pass, uint32_t wave, uint32_t tt)
{
	return pass * LW_SP_COLS + wave * 64u + tt * 32u < a.bins;
}

#ifndef LW_KERNEL_HOST
typedef float lw_sp_f16 __attribute__((ext_vector_type(16)));
#endif

// ---- fold: the 16 support samples of the staged tile into the lane's accumulators, k ascending
template <int ROUTE> LW_LANES_FN void lw_sp_mma(const LwSpecArgs &a, uint32_t pass, uint32_t tid, const float *lds, LwSpLane &st)
{
	const uint32_t lane = tid & 63u, wave = tid >> 6, f = lane & 31u;
	const float *as = lds + LW_SP_LDS_A + wave * 64u, *xs = lds + LW_SP_LDS_X;
#ifndef LW_KERNEL_HOST
	if (ROUTE == LW_SP_ROUTE_MFMA) {
		// A[i = lane & 31][k = lane >> 5] = basis[k][bin i], B[k = lane >> 5][j = lane & 31] = x of frame j: one f32 each
		const uint32_t h = lane >> 5;
#pragma unroll
		for (uint32_t tt = 0; tt < 2u; tt++) {
			if (!lw_sp_tile_live(a, pass, wave, tt))
				continue;
			lw_sp_f16 re, im;
#pragma unroll
			for (int r = 0; r < 16; r++)
				re[r] = st.acc[2 * tt][r], im[r] = st.acc[2 * tt + 1][r];
#pragma unroll
			for (uint32_t kk = 0; kk < LW_SP_KT; kk += 2u) {
				const float b = xs[(kk + h) * LW_SP_XS + f];
				const float *row = as + (kk + h) * (2u * LW_SP_COLS) + tt * 32u + f;
				re = __builtin_amdgcn_mfma_f32_32x32x2f32(row[0], b, re, 0, 0, 0);
				im = __builtin_amdgcn_mfma_f32_32x32x2f32(row[LW_SP_COLS], b, im, 0, 0, 0);
			}
#pragma unroll
			for (int r = 0; r < 16; r++)
				st.acc[2 * tt][r] = re[r], st.acc[2 * tt + 1][r] = im[r];
		}
		return;
	}
#endif
#pragma unroll
	for (uint32_t tt = 0; tt < 2u; tt++) {
		if (!lw_sp_tile_live(a, pass, wave, tt))
			continue;
		for (uint32_t kk = 0; kk < LW_SP_KT; kk++) {
			const float b = xs[kk * LW_SP_XS + f];
			const float *row = as + kk * (2u * LW_SP_COLS) + tt * 32u;
#pragma unroll
			for (uint32_t r = 0; r < 16u; r++) {
				const uint32_t i = LW_MFMA32_ROW(r, lane);
				st.acc[2 * tt][r] = __builtin_fmaf(b, row[i], st.acc[2 * tt][r]);
				st.acc[2 * tt + 1][r] = __builtin_fmaf(b, row[LW_SP_COLS + i], st.acc[2 * tt + 1][r]);
			}
		}
	}
}

// ---- power: P = fmaf(im, im, re * re) of the pass into LDS, [bin of the pass][frame]
LW_LANES_FN void lw_sp_power(const LwSpecArgs &a, uint32_t pass, uint32_t tid, float *lds, const LwSpLane &st)
{
	const uint32_t lane = tid & 63u, wave = tid >> 6, f = lane & 31u;
#pragma unroll
	for (uint32_t tt = 0; tt < 2u; tt++) {
		if (!lw_sp_tile_live(a, pass, wave, tt))
			continue;
#pragma unroll
		for (uint32_t r = 0; r < 16u; r++) {
			const float re = st.acc[2 * tt][r], im = st.acc[2 * tt + 1][r];
			const float sq = re * re;
			lds[LW_SP_LDS_P + (wave * 64u + tt * 32u + LW_MFMA32_ROW(r, lane)) * LW_SP_TF + f] = __builtin_fmaf(im, im, sq);
		}
	}
}

// ---- the pass's bins from the P region of LDS to the lines line0 + bin, consecutive lanes on consecutive frames
LW_LANES_FN void lw_sp_store_lines(const LwSpecArgs &a, const LwSpTile &t, uint32_t pass, uint32_t tid, const float *lds, uint32_t line0)
{
	const uint32_t f = tid % LW_SP_TF;
	if (t.f0 + f >= t.n_frames)
		return;
	for (uint32_t c = tid / LW_SP_TF; c < LW_SP_COLS; c += LW_SP_THREADS / LW_SP_TF) {
		const uint32_t bin = pass * LW_SP_COLS + c;
		if (bin >= a.bins)
			break;
		a.dst[t.d_at + (uint64_t)(bin + line0) * a.d_line + t.f0 + f] = lds[LW_SP_LDS_P + c * LW_SP_TF + f];
	}
}

// ---- without a mel matrix: the power (PRO: the lines follow the energy line when there is one)
template <int PRO = 0> LW_LANES_FN void lw_sp_store_power(const LwSpecArgs &a, const LwSpTile &t, uint32_t pass, uint32_t tid, const float *lds)
{
	lw_sp_store_lines(a, t, pass, tid, lds, PRO ? a.energy : 0u);
}

// ---- complex output (LW_SPEC_OUT_COMPLEX; OUT = 1 in the kernel): re (SINE = 0) or im (SINE = 1) of the pass into the P region,
// laid out as lw_sp_power lays out P, and from there to the lines line0 + bin: re[j] on line j, im[j] on line B + j, the two
// chains themselves and nothing formed from them
template <int SINE> LW_LANES_FN void lw_sp_part(const LwSpecArgs &a, uint32_t pass, uint32_t tid, float *lds, const LwSpLane &st)
{
	const uint32_t lane = tid & 63u, wave = tid >> 6, f = lane & 31u;
#pragma unroll
	for (uint32_t tt = 0; tt < 2u; tt++) {
		if (!lw_sp_tile_live(a, pass, wave, tt))
			continue;
#pragma unroll
		for (uint32_t r = 0; r < 16u; r++)
			lds[LW_SP_LDS_P + (wave * 64u + tt * 32u + LW_MFMA32_ROW(r, lane)) * LW_SP_TF + f] = st.acc[2 * tt + SINE][r];
	}
}

// ---- mel: slice jc (32 bins) of the pass; the matrix slice [32][mel_pad] into the basis tile's place, then the fold
LW_LANES_FN void lw_sp_stage_fb(const LwSpecArgs &a, uint32_t pass, uint32_t jc, uint32_t tid, float *lds)
{
	const uint32_t j0 = pass * LW_SP_COLS + jc * LW_SP_JT, n = LW_SP_JT * a.mel_pad / 4u; // <= 8 per lane
	const LwSpF4 *g = (const LwSpF4 *)(a.fb + (size_t)j0 * a.mel_pad);
	LwSpF4 v[8];
#pragma unroll
	for (uint32_t q = 0; q < 8u; q++) {
		const uint32_t i = tid + q * LW_SP_THREADS;
		v[q] = g[i < n ? i : n - 1u];
	}
	LwSpF4 *fs = (LwSpF4 *)(lds + LW_SP_LDS_A);
#pragma unroll
	for (uint32_t q = 0; q < 8u; q++) {
		const uint32_t i = tid + q * LW_SP_THREADS;
		if (i < n)
			fs[i] = v[q];
	}
}

LW_LANES_FN void lw_sp_mel(const LwSpecArgs &a, uint32_t pass, uint32_t jc, uint32_t tid, const float *lds, LwSpLane &st)
{
	const uint32_t f = tid % LW_SP_TF, g = tid / LW_SP_TF, nb = a.mel_pad / 32u;
	const uint32_t j0 = pass * LW_SP_COLS + jc * LW_SP_JT, nj = a.bins - j0 < LW_SP_JT ? a.bins - j0 : LW_SP_JT;
	const float *ps = lds + LW_SP_LDS_P + jc * LW_SP_JT * LW_SP_TF + f;
	for (uint32_t jj = 0; jj < nj; jj++) {
		const float p = ps[jj * LW_SP_TF];
		const LwSpF4 *w = (const LwSpF4 *)(lds + LW_SP_LDS_A + jj * a.mel_pad) + g;
#pragma unroll
		for (uint32_t b = 0; b < 8u; b++)
			if (b < nb) {
				const LwSpF4 w4 = w[8u * b];
#pragma unroll
				for (int i = 0; i < 4; i++)
					st.mel[b][i] = __builtin_fmaf(p, w4.v[i], st.mel[b][i]);
			}
	}
}

template <int PRO = 0> LW_LANES_FN void lw_sp_store_mel(const LwSpecArgs &a, const LwSpTile &t, uint32_t tid, const LwSpLane &st)
{
	const uint32_t f = tid % LW_SP_TF, g = tid / LW_SP_TF, line0 = PRO ? a.energy : 0u;
	if (t.f0 + f >= t.n_frames)
		return;
#pragma unroll
	for (uint32_t b = 0; b < 8u; b++)
#pragma unroll
		for (uint32_t i = 0; i < 4u; i++) {
			const uint32_t q = 4u * (g + 8u * b) + i;
			if (q < a.n_mels)
				a.dst[t.d_at + (uint64_t)(q + line0) * a.d_line + t.f0 + f] = st.mel[b][i];
		}
}

// slices of the mel matrix that pass `pass` folds
LW_LANES_FN uint32_t lw_sp_slices(const LwSpecArgs &a, uint32_t pass)
{
	const uint32_t left = a.bins - pass * LW_SP_COLS, n = left < LW_SP_COLS ? left : LW_SP_COLS;
	return (n + LW_SP_JT - 1u) / LW_SP_JT;
}

// ---- the per-frame prologue (remove_dc || energy; include/lewton_amd.h "DC removal and energy"): of each of the tile's 32 frames
//   S1 = the fold of (double)x_k, k ascending from +0.0, sequential;  S2 = the same fold of (double)x_k * (double)x_k (exact)
// over the W support samples after padding; mu = (float)(S1 / W) goes to the staging step, E to line 0 of the destination.  Four
// phases with a barrier behind each, all before the first stage of the K loop, in LDS that is free until then: the tile's span
// of samples in the P region (LW_SP_SPAN_AT; a.span = 0: it does not fit, and the chains read the row), the sums and mu where
// the frame tile will be.  The 64 chains of W dependent f64 additions are what the prologue costs: 32 lanes of wave 0 fold S1, 32
// lanes of wave 1 fold S2, side by side on two SIMDs.
#define LW_SP_PRO_S1 LW_SP_LDS_X                    // [32] doubles
#define LW_SP_PRO_S2 (LW_SP_LDS_X + 2u * LW_SP_TF)  // [32] doubles
#define LW_SP_PRO_MU (LW_SP_LDS_X + 4u * LW_SP_TF)  // [32] floats
static_assert(5u * LW_SP_TF <= LW_SP_KT * LW_SP_XS && LW_SP_LDS_X % 2u == 0, "the prologue's sums fit the frame tile's place, 8-byte aligned");

LW_LANES_FN void lw_sp_put_d(float *at, double v)
{
	__builtin_memcpy(at, &v, sizeof v);
}

LW_LANES_FN double lw_sp_get_d(const float *at)
{
	double v;
	__builtin_memcpy(&v, at, sizeof v);
	return v;
}

template <int PAD = LW_SP_PAD_ARGS> LW_LANES_FN void lw_sp_pro_span(const LwSpecArgs &a, const LwSpTile &t, uint32_t tid, float *lds)
{
	// eight loads of a lane in flight before its first store (a load beyond the span goes to a clamped index like any other)
	for (uint32_t s0 = tid; s0 < a.span; s0 += 8u * LW_SP_THREADS) {
		float v[8];
#pragma unroll
		for (uint32_t q = 0; q < 8u; q++)
			v[q] = lw_sp_x<PAD>(a, t, t.x0 + (int64_t)(s0 + q * LW_SP_THREADS));
#pragma unroll
		for (uint32_t q = 0; q < 8u; q++) {
			const uint32_t s = s0 + q * LW_SP_THREADS;
			if (s < a.span)
				lds[LW_SP_LDS_P + LW_SP_SPAN_AT(s)] = v[q];
		}
	}
}

template <int PAD = LW_SP_PAD_ARGS> LW_LANES_FN void lw_sp_pro_sums(const LwSpecArgs &a, const LwSpTile &t, uint32_t tid, float *lds)
{
	const uint32_t wave = tid >> 6, f = tid & 63u;
	if (wave > 1u || f >= LW_SP_TF)
		return;
	double s = 0.0;
	if (a.span) {
		const uint32_t s0 = f * a.hop;
		const float *p = lds + LW_SP_LDS_P;
		if (wave == 0) { // (a loop per wave: no select, and no multiply in the S1 chain)
#pragma unroll 8
			for (uint32_t k = 0; k < a.win_length; k++)
				s = s + (double)p[LW_SP_SPAN_AT(s0 + k)];
		} else {
#pragma unroll 8
			for (uint32_t k = 0; k < a.win_length; k++) {
				const double d = (double)p[LW_SP_SPAN_AT(s0 + k)];
				s = s + d * d;
			}
		}
	} else {
#pragma unroll 8
		for (uint32_t k = 0; k < a.win_length; k++) {
			const double d = (double)lw_sp_x<PAD>(a, t, lw_sp_index(a, t, f, k));
			s = s + (wave ? d * d : d);
		}
	}
	lw_sp_put_d(lds + (wave ? LW_SP_PRO_S2 : LW_SP_PRO_S1) + 2u * f, s);
}

// mu of the tile's frames into LDS (+0.0 without remove_dc), and E of the frames that exist to line 0: every operation one
// rounding (the unit is compiled with -ffp-contract=off), Ed = 0 unless Ed > 0 (a NaN too)
LW_LANES_FN void lw_sp_pro_finish(const LwSpecArgs &a, const LwSpTile &t, uint32_t tid, float *lds)
{
	if (tid >= LW_SP_TF)
		return;
	const double S1 = lw_sp_get_d(lds + LW_SP_PRO_S1 + 2u * tid), S2 = lw_sp_get_d(lds + LW_SP_PRO_S2 + 2u * tid), W = (double)a.win_length;
	const float mu = (float)(S1 / W);
	lds[LW_SP_PRO_MU + tid] = a.remove_dc ? mu : 0.0f;
	if (!a.energy || t.f0 + tid >= t.n_frames)
		return;
	double Ed = S2;
	if (a.remove_dc) {
		const double sq = S1 * S1, part = sq / W;
		Ed = S2 - part;
	}
	if (!(Ed > 0.0))
		Ed = 0.0;
	a.dst[t.d_at + t.f0 + tid] = (float)(Ed * a.escale);
}

// the means of the two frames a lane stages in every K tile (frame e / LW_SP_KT of e = tid + q * 256)
LW_LANES_FN void lw_sp_pro_mu(uint32_t tid, const float *lds, float &mu0, float &mu1)
{
	mu0 = lds[LW_SP_PRO_MU + tid / LW_SP_KT];
	mu1 = lds[LW_SP_PRO_MU + tid / LW_SP_KT + LW_SP_THREADS / LW_SP_KT];
}

#ifndef LW_KERNEL_HOST

// The body of both kernels.  OUT is the object's output (LW_SPEC_OUT_*) as a compile-time constant, for PAD's reason: k_spec is
// the body with OUT = 0, the kernel it was before the complex output existed (profiles/rows_spec_resource_usage.txt), and
// k_spec_complex the body with OUT = 1 and no prologue.
// PRO = 0 is the kernel without the prologue, to the instruction: what every object without remove_dc and energy runs
template <int ROUTE, int PAD, int PRO, int OUT> LW_LANES_FN void lw_sp_body(const LwSpecArgs &a, float *lw_sp_lds)
{
	LwSpTile t;
	if (!lw_sp_tile(a, blockIdx.x, blockIdx.y, blockIdx.z, t))
		return; // (the whole workgroup: the tile is behind its row's last frame)
	const uint32_t tid = threadIdx.x;
	LwSpLane st;
	lw_sp_zero_mel(st);
	float mu0 = 0.0f, mu1 = 0.0f;
	if (PRO) {
		lw_sp_pro_span<PAD>(a, t, tid, lw_sp_lds);
		__syncthreads();
		lw_sp_pro_sums<PAD>(a, t, tid, lw_sp_lds);
		__syncthreads();
		lw_sp_pro_finish(a, t, tid, lw_sp_lds);
		__syncthreads();
		lw_sp_pro_mu(tid, lw_sp_lds, mu0, mu1);
		__syncthreads();
	}
	for (uint32_t pass = 0; pass < a.passes; pass++) {
		lw_sp_zero_acc(st);
		for (uint32_t kt = 0; kt < a.k_pad / LW_SP_KT; kt++) {
			lw_sp_stage<PAD, PRO>(a, t, pass, kt, tid, lw_sp_lds, mu0, mu1);
			__syncthreads();
			lw_sp_mma<ROUTE>(a, pass, tid, lw_sp_lds, st);
			__syncthreads();
		}
		if (OUT) { // re of the pass, then im, through the P region; the next pass's barriers stand behind the last reads
			lw_sp_part<0>(a, pass, tid, lw_sp_lds, st);
			__syncthreads();
			lw_sp_store_lines(a, t, pass, tid, lw_sp_lds, 0u);
			__syncthreads();
			lw_sp_part<1>(a, pass, tid, lw_sp_lds, st);
			__syncthreads();
			lw_sp_store_lines(a, t, pass, tid, lw_sp_lds, a.bins);
			continue;
		}
		lw_sp_power(a, pass, tid, lw_sp_lds, st);
		__syncthreads();
		if (a.n_mels == 0) {
			lw_sp_store_power<PRO>(a, t, pass, tid, lw_sp_lds);
			continue; // (the next pass's barriers stand between these reads and its power stores)
		}
		for (uint32_t jc = 0; jc < lw_sp_slices(a, pass); jc++) {
			lw_sp_stage_fb(a, pass, jc, tid, lw_sp_lds);
			__syncthreads();
			lw_sp_mel(a, pass, jc, tid, lw_sp_lds, st);
			__syncthreads();
		}
	}
	if (!OUT && a.n_mels)
		lw_sp_store_mel<PRO>(a, t, tid, st);
}

template <int ROUTE, int PAD, int PRO> __global__ void __launch_bounds__(LW_SP_THREADS) k_spec(LwSpecArgs a)
{
	extern __shared__ float lw_sp_lds[];
	lw_sp_body<ROUTE, PAD, PRO, 0>(a, lw_sp_lds);
}

template <int ROUTE, int PAD> __global__ void __launch_bounds__(LW_SP_THREADS) k_spec_complex(LwSpecArgs a)
{
	extern __shared__ float lw_sp_lds[];
	lw_sp_body<ROUTE, PAD, 0, 1>(a, lw_sp_lds);
}

template <int ROUTE, int PAD> static hipError_t lw_sp_launch_complex(const LwSpecArgs &a, dim3 grid, hipStream_t st)
{
	static LwPerDeviceOnce once;
	const hipError_t e = once.run([] {
		return hipFuncSetAttribute((const void *)k_spec_complex<ROUTE, PAD>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(LW_SP_LDS_FLOATS * sizeof(float)));
	});
	if (e != hipSuccess)
		return e;
	return lw_launch_k(k_spec_complex<ROUTE, PAD>, grid, dim3(LW_SP_THREADS), (size_t)LW_SP_LDS_FLOATS * sizeof(float), st, a);
}

template <int ROUTE, int PAD, int PRO> static hipError_t lw_sp_launch(const LwSpecArgs &a, dim3 grid, hipStream_t st)
{
	static LwPerDeviceOnce once; // above the default limit of dynamic LDS: per device, once
	const hipError_t e = once.run([] {
		return hipFuncSetAttribute((const void *)k_spec<ROUTE, PAD, PRO>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(LW_SP_LDS_FLOATS * sizeof(float)));
	});
	if (e != hipSuccess)
		return e;
	return lw_launch_k(k_spec<ROUTE, PAD, PRO>, grid, dim3(LW_SP_THREADS), (size_t)LW_SP_LDS_FLOATS * sizeof(float), st, a);
}

template <int ROUTE, int PAD> static hipError_t lw_sp_launch_pro(const LwSpecArgs &a, dim3 grid, hipStream_t st)
{
	if (a.output == 1u)
		return lw_sp_launch_complex<ROUTE, PAD>(a, grid, st);
	return a.remove_dc || a.energy ? lw_sp_launch<ROUTE, PAD, 1>(a, grid, st) : lw_sp_launch<ROUTE, PAD, 0>(a, grid, st);
}

hipError_t lw_launch_spec(const LwSpecArgs &a, int route, uint32_t tiles, uint32_t ch, uint32_t n_rows, hipStream_t st)
{
	if (tiles == 0 || n_rows == 0)
		return hipSuccess;
	if (ch == 0 || ch > 65535u || n_rows > 65535u || tiles > LW_SP_MAX_TILES || a.k_pad == 0 || a.k_pad % LW_SP_KT || a.mel_pad > 256u || a.mel_pad % 32u ||
			(a.n_mels != 0 && !a.fb) || a.output > 1u || (a.output == 1u && (a.n_mels || a.remove_dc || a.energy)))
		return hipErrorInvalidValue;
	const dim3 grid(tiles, ch, n_rows);
	if (route != LW_SP_ROUTE_MFMA && route != LW_SP_ROUTE_FMA)
		return hipErrorInvalidValue;
	if (a.span && (a.span != (LW_SP_TF - 1u) * a.hop + a.win_length || !lw_spec_span_fits(a.hop, a.win_length))) // (it indexes LDS)
		return hipErrorInvalidValue;
	if (a.pad_mode == 0)
		return route == LW_SP_ROUTE_MFMA ? lw_sp_launch_pro<LW_SP_ROUTE_MFMA, 0>(a, grid, st) : lw_sp_launch_pro<LW_SP_ROUTE_FMA, 0>(a, grid, st);
	if (a.pad_mode == 1)
		return route == LW_SP_ROUTE_MFMA ? lw_sp_launch_pro<LW_SP_ROUTE_MFMA, 1>(a, grid, st) : lw_sp_launch_pro<LW_SP_ROUTE_FMA, 1>(a, grid, st);
	if (a.pad_mode == 2)
		return route == LW_SP_ROUTE_MFMA ? lw_sp_launch_pro<LW_SP_ROUTE_MFMA, 2>(a, grid, st) : lw_sp_launch_pro<LW_SP_ROUTE_FMA, 2>(a, grid, st);
	return hipErrorInvalidValue;
}

#endif // LW_KERNEL_HOST
