// Frame-major model input (product code, gfx950): k_pack, the kernel of lw_pack_rows.  A pass of its own from f32
// [row][ch][F][frame_capacity] rows to [row][ch][out_capacity][W * F] frames of f32, bf16 or f16 by the rule of
// include/lewton_amd.h ("frame-major model input"), bit for bit: a tiled transpose with a gather along time.  ONE launch: the
// source is read once and the destination written once.
//   A workgroup of 256 lanes takes `tile` consecutive output frames of one row and channel (lw_pack.hpp, the tile plan).  Per
//   group of up to 32 feature lines:
//   load   the span of source frames the tile needs, line by line, lanes along the frames (coalesced 4-byte loads, each at a
//          clamped or valid frame index), into the LDS image [line][pitch].  32 consecutive lanes store to 32 consecutive
//          dwords: no bank conflict whatever the pitch.
//   store  lanes along the destination.  A lane owns a UNIT of E consecutive elements of one frame and context position p = (u, k):
//          E = 4 (f32) or 8 (bf16, f16) -- 16 bytes -- where the destination's alignment and F allow, else E = 1.  32 / E lanes
//          cover the 32 lines of p, so a 32-lane half holds E consecutive p.  The pitch is 1 mod 32, so line g, frame s is on bank
//          (g + s) mod 32; in step i a lane reads line g0 + ((i + p - s) mod E) of its unit, bank = g0 + (i + p) mod E (mod 32):
//          lanes of one p differ by multiples of E, lanes of different p differ mod E -- no conflict (ds_read_b32, 32 banks per
//          half).  The E values are rotated back in registers, shifted, scaled, converted, packed and stored as one vector.
//   The fill with pad and the mask (channel 0 only) go first; they depend on no image.
// No atomics, offsets in 64 bits.  Nothing at or beyond n of a source line is read, nothing outside [0, fill_end) of a
// destination channel written.  tests/san/pack_host.cpp compiles this file for the host (LW_PACK_HOST) and runs it workgroup by
// workgroup, the phases in the kernel's order.
#include "lw_pack.hpp"

#ifdef LW_KERNEL_HOST
#include <cstring>
#else
#include "lw_kernels.hpp"
#endif

struct LwPkTile { // what a workgroup works on; the same for all its lanes
	uint64_t n;       // the row's T
	uint64_t u0;      // first output frame of the tile
	uint32_t nu;      // output frames of the tile below T_out (0: the tile only fills)
	uint32_t fill_lo, fill_hi; // frames [u0 + fill_lo, u0 + fill_hi) of the tile receive pad
	uint32_t span;    // source frames the nu frames need: (nu - 1) * stride + W
	int64_t first;    // the source frame of the image's column 0, before clamping
	uint64_t src_at;  // element of line 0, frame 0 of the row and channel in the source
	uint64_t dst_at;  // element of frame 0 of the row and channel in the destination
	uint64_t mask_at; // ... of the row in the mask
};

// false: the tile lies at or beyond the row's fill_end, nothing to do
LW_LANES_FN bool lw_pk_tile(const LwPackArgs &a, uint32_t bx, uint32_t by, uint32_t bz, LwPkTile &t)
{
	const uint64_t row = (uint64_t)a.row0 + bz;
	const LwPackRow r = a.rows[row];
	t.n = r.n, t.u0 = (uint64_t)bx * a.plan.tile;
	if (t.u0 >= r.fill_end)
		return false;
	const uint64_t hi = t.u0 + a.plan.tile;
	t.nu = t.u0 < r.n_out ? (uint32_t)((hi < r.n_out ? hi : r.n_out) - t.u0) : 0u;
	t.fill_lo = t.nu; // (n_out <= fill_end, so the fill starts where the data ends, or at the tile's start)
	t.fill_hi = (uint32_t)((hi < r.fill_end ? hi : r.fill_end) - t.u0);
	t.span = t.nu ? (t.nu - 1u) * a.stride + a.W : 0u;
	t.first = (int64_t)(t.u0 * a.stride) - (a.edge == LW_PK_REPLICATE ? (int64_t)a.left : 0);
	t.src_at = (row * a.ch + by) * a.F * a.line_el;
	t.dst_at = (row * a.ch + by) * a.out_cap * a.D;
	t.mask_at = row * a.out_cap;
	return true;
}

// E consecutive converted elements from element `at` of the destination: one store of 16 bytes (E = 4: f32; E = 8: two to a
// dword), or of one element (E = 1)
template <int E>
LW_LANES_FN void lw_pk_put(const LwPackArgs &a, void *LW_LANES_RESTRICT dst, uint64_t at, const uint32_t (&c)[E])
{
	if (E == 1) {
		if (a.dtype == LW_PK_F32)
			((uint32_t *)dst)[at] = c[0];
		else
			((uint16_t *)dst)[at] = (uint16_t)c[0];
		return;
	}
	uint32_t w[4];
#pragma unroll
	for (int i = 0; i < 4; i++)
		w[i] = E == 4 ? c[i] : (c[(2 * i) % E] | (c[(2 * i + 1) % E] << 16));
#ifdef LW_KERNEL_HOST
	memcpy((char *)dst + at * (E == 4 ? 4u : 2u), w, 16);
#else
	*(uint4 *)((char *)dst + at * (E == 4 ? 4u : 2u)) = make_uint4(w[0], w[1], w[2], w[3]);
#endif
}

// ---- the mask of the tile's frames: the lanes of channel 0
LW_LANES_FN void lw_pk_mask(const LwPackArgs &a, const LwPkTile &t, uint8_t *LW_LANES_RESTRICT mask, uint32_t tid)
{
	if (tid < t.fill_hi)
		mask[t.mask_at + t.u0 + tid] = tid < t.nu ? 1u : 0u;
}

// ---- pad into frames [fill_lo, fill_hi) of the tile: one contiguous run of the destination
template <int E>
LW_LANES_FN void lw_pk_fill(const LwPackArgs &a, const LwPkTile &t, void *LW_LANES_RESTRICT dst, uint32_t tid)
{
	uint32_t c[E];
#pragma unroll
	for (int i = 0; i < E; i++)
		c[i] = a.pad_bits;
	const uint64_t at = t.dst_at + (t.u0 + t.fill_lo) * a.D;
	const uint32_t units = (t.fill_hi - t.fill_lo) * (a.D / (uint32_t)E); // (at most 256 * 33 * 65535)
	for (uint32_t i = tid; i < units; i += LW_PK_THREADS)
		lw_pk_put<E>(a, dst, at + (uint64_t)i * E, c);
}

// ---- lines f0 .. f0 + G - 1 of the tile's span into the image: wave w takes lines w, w + 4, ..., its lanes the frames
LW_LANES_FN void lw_pk_load(const LwPackArgs &a, const LwPkTile &t, const uint32_t *LW_LANES_RESTRICT src, uint32_t *img, uint32_t f0, uint32_t G,
		uint32_t tid)
{
	for (uint32_t s = tid & 63u; s < t.span; s += 64u) {
		int64_t fr = t.first + (int64_t)s;
		if (a.edge == LW_PK_REPLICATE)
			fr = fr < 0 ? 0 : fr >= (int64_t)t.n ? (int64_t)t.n - 1 : fr;
		const uint32_t *x = src + t.src_at + (uint64_t)fr; // (VALID: fr < n for every column of the span)
#pragma unroll 4
		for (uint32_t g = tid >> 6; g < G; g += LW_PK_THREADS / 64u)
			img[g * a.plan.pitch + s] = x[(uint64_t)(f0 + g) * a.line_el];
	}
}

// ---- the image into the destination: unit L = (q = L % (32 / E), p = L / (32 / E)), p = (u, k) = (p / W, p % W)
template <int E>
LW_LANES_FN void lw_pk_store(const LwPackArgs &a, const LwPkTile &t, const uint32_t *img, void *LW_LANES_RESTRICT dst, uint32_t f0, uint32_t G, uint32_t tid)
{
	const uint32_t Q = LW_PK_GROUP / (uint32_t)E, units = t.nu * a.W * Q;
	for (uint32_t L = tid; L < units; L += LW_PK_THREADS) {
		const uint32_t g0 = (L % Q) * (uint32_t)E, p = L / Q;
		if (g0 >= G)
			continue;
		const uint32_t u = p / a.W, k = p - u * a.W, s = u * a.stride + k;
		const uint32_t rot = (p - s) & (uint32_t)(E - 1);
		uint32_t v[E];
#pragma unroll
		for (int i = 0; i < E; i++)
			v[i] = img[(g0 + (((uint32_t)i + rot) & (uint32_t)(E - 1))) * a.plan.pitch + s];
		// v[i] holds line g0 + (i + rot) % E: rotate it back, a power of two at a time
#pragma unroll
		for (int b = 1; b < E; b <<= 1) {
			uint32_t w[E];
#pragma unroll
			for (int i = 0; i < E; i++)
				w[i] = (rot & (uint32_t)b) ? v[(i - b + E) % E] : v[i];
#pragma unroll
			for (int i = 0; i < E; i++)
				v[i] = w[i];
		}
		const uint32_t j = k * a.F + f0 + g0;
		if (a.shift || a.scale) {
#pragma unroll
			for (int i = 0; i < E; i++) {
				float x = __builtin_bit_cast(float, v[i]);
				if (a.shift)
					x = x + a.shift[j + (uint32_t)i];
				if (a.scale)
					x = x * a.scale[j + (uint32_t)i];
				v[i] = __builtin_bit_cast(uint32_t, x);
			}
		}
#pragma unroll
		for (int i = 0; i < E; i++)
			v[i] = lw_pack_cvt(a.dtype, v[i]);
		lw_pk_put<E>(a, dst, t.dst_at + (t.u0 + u) * a.D + j, v);
	}
}

#ifndef LW_KERNEL_HOST

template <int E>
__device__ __forceinline__ void lw_pk_block(const LwPackArgs &a, const LwPkTile &t, const uint32_t *__restrict__ src, void *__restrict__ dst,
		uint32_t *img, uint32_t tid)
{
	if (t.fill_hi > t.fill_lo)
		lw_pk_fill<E>(a, t, dst, tid);
	if (!t.nu)
		return;
	for (uint32_t f0 = 0; f0 < a.F; f0 += LW_PK_GROUP) { // (the same trip count in every lane)
		const uint32_t left = a.F - f0, G = left < LW_PK_GROUP ? left : LW_PK_GROUP;
		if (f0)
			__syncthreads(); // the image is read to the end before the next group overwrites it
		lw_pk_load(a, t, src, img, f0, G, tid);
		__syncthreads();
		lw_pk_store<E>(a, t, img, dst, f0, G, tid);
	}
}

__global__ void __launch_bounds__(LW_PK_THREADS) k_pack(LwPackArgs a, const uint32_t *__restrict__ src, void *__restrict__ dst, uint8_t *__restrict__ mask)
{
	extern __shared__ __attribute__((aligned(16))) uint32_t lw_pk_lds[];
	LwPkTile t;
	if (!lw_pk_tile(a, blockIdx.x, blockIdx.y, blockIdx.z, t))
		return;
	if (mask && blockIdx.y == 0)
		lw_pk_mask(a, t, mask, threadIdx.x);
	if (!a.vec)
		lw_pk_block<1>(a, t, src, dst, lw_pk_lds, threadIdx.x);
	else if (a.dtype == LW_PK_F32)
		lw_pk_block<4>(a, t, src, dst, lw_pk_lds, threadIdx.x);
	else
		lw_pk_block<8>(a, t, src, dst, lw_pk_lds, threadIdx.x);
}

hipError_t lw_launch_pack(const LwPackArgs &a, const float *src, void *dst, uint8_t *mask, uint32_t tiles, uint32_t n_rows, hipStream_t st)
{
	const LwPackPlan p = lw_pack_plan(a.F, a.W, a.stride);
	const uint32_t E = a.dtype == LW_PK_F32 ? 4u : 8u;
	if (n_rows == 0 || n_rows > 65535u || a.ch == 0 || a.ch > 65535u || tiles == 0 || tiles > LW_PK_MAX_TILES || !a.rows || !dst || a.F == 0 ||
			a.stride == 0 || a.W == 0 || a.left >= a.W || a.D != a.W * a.F || a.dtype < LW_PK_F32 || a.dtype > LW_PK_F16 ||
			(a.edge != LW_PK_REPLICATE && a.edge != LW_PK_VALID) || p.tile != a.plan.tile || p.pitch != a.plan.pitch || p.lines != a.plan.lines ||
			p.lds != a.plan.lds || (a.vec && (a.F % E || ((uintptr_t)dst & 15u))))
		return hipErrorInvalidValue;
	const uint32_t *bits = (const uint32_t *)src; // values travel as bit patterns: a copy keeps a NaN's payload
	return lw_launch_k(k_pack, dim3(tiles, a.ch, n_rows), dim3(LW_PK_THREADS), (size_t)a.plan.lds, st, a, bits, dst, mask);
}

#endif // LW_KERNEL_HOST
