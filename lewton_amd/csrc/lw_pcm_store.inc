// PCM sample stores of every kernel family (included by lw_kernels.hip, lw_kernels_long.hip, lw_kernels_big.hip): the sample
// conversion (samples.rs:92-103) and the store of one, two or four consecutive samples of one channel in the kernel-internal output
// format FMT (LwOutFmt, lw_kernels.hpp).  The stereo unit forms (store_interleaved2*, ola_store_itl2_10*) keep their own lane shuffles.
//
// Each primitive takes its pointer and 32-bit index terms in the association its callers compute them: `ptr + a + b` with uint32_t
// terms widens each term on its own, so folding `a + b` into one 32-bit index would be a different program.  k_long's ola_store and
// store_quad, and k_ola_generic's four-sample path, keep their own stores: through these primitives hipcc schedules them differently.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

typedef float float2_t __attribute__((ext_vector_type(2)));
typedef float float4_t __attribute__((ext_vector_type(4)));
typedef short short2_t __attribute__((ext_vector_type(2)));

// 8-byte PCM store as a write-through (sc1) store: the bytes leave the L2 while the kernel is still running instead of
// staying dirty until the end-of-kernel write-back (16.8 MB of dirty PCM cost ~2.7 us at every kernel boundary)
__device__ __forceinline__ void store_pcm8(void *p, uint32_t lo, uint32_t hi)
{
	__hip_atomic_store(reinterpret_cast<unsigned long long *>(p), ((unsigned long long)hi << 32) | lo, __ATOMIC_RELAXED,
			__HIP_MEMORY_SCOPE_AGENT);
}

// 16-byte write-through store (f32 PCM, stream state).  Inline asm because the builtin path offers sc1 only up to 8
// bytes; the trailing s_nop keeps hipcc from overwriting the data registers before the store has read them.
__device__ __forceinline__ void store16_wt(void *p, float4_t v)
{
	asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
}

// two samples already times 32768 and truncated toward zero (v_cvt_i32_f32: saturating, NaN -> 0) to i16 by the saturating pack
// v_cvt_pk_i16_i32 -- equal to the reference's compare/clamp/`as i16` (the bounds are integers)
union LwPk16 {
	short2_t s;
	uint32_t u;
};
__device__ __forceinline__ LwPk16 pcm_pack_i16(int a, int b)
{
	LwPk16 p;
	p.s = __builtin_amdgcn_cvt_pk_i16(a, b);
	return p;
}

// one sample by compares (k_ola_generic): x*32768, clamp to [-32768, 32767], truncate toward zero; NaN -> 0
__device__ __forceinline__ int16_t to_i16(float x)
{
	const float t = x * 32768.0f;
	if (t > 32767.0f)
		return 32767;
	if (t < -32768.0f)
		return -32768;
	return (int16_t)(int)t; // in range: truncation toward zero; NaN -> 0 (v_cvt_i32_f32), like Rust `as`
}

// The 16 samples of a lane after ola_block (O[c2][k]: .x = position q_k of the left quarter, .y = its mirror), as four groups of four
// consecutive positions: v[0] at 4l, v[1] at 8L - 4 - 4l, v[2] at 8L + 4l, v[3] at 16L - 4 - 4l (L lanes per channel half)
struct LwQuads {
	float v[4][4];
};
__device__ __forceinline__ LwQuads pcm_quads(const float2_t (&O)[2][4])
{
	return {{{O[0][3].x, O[0][2].x, O[1][3].x, O[1][2].x}, {O[1][1].x, O[1][0].x, O[0][1].x, O[0][0].x},
		{O[0][0].y, O[0][1].y, O[1][0].y, O[1][1].y}, {O[1][2].y, O[1][3].y, O[0][2].y, O[0][3].y}}};
}

// Four consecutive samples v (already x 32768 for the i16 formats) as write-through stores: planar at out + e0 + e1 + pos (one
// 16- or 8-byte store), interleaved at out + e0 + (pos + k) * stride + e1 (e0: the packet's first element, e1: the channel's offset)
template <int FMT>
__device__ __forceinline__ void pcm_store4(void *out, uint32_t e0, uint32_t e1, uint32_t pos, uint32_t stride, const float (&v)[4])
{
	if (FMT == LW_OUT_F32_PLANAR) {
		store16_wt(reinterpret_cast<float *>(out) + e0 + e1 + pos, float4_t{v[0], v[1], v[2], v[3]});
	} else if (FMT == LW_OUT_F32_INTERLEAVED) {
		float *o = reinterpret_cast<float *>(out) + e0;
		const uint32_t off = pos * stride + e1;
		o[off] = v[0];
		o[off + stride] = v[1];
		o[off + 2u * stride] = v[2];
		o[off + 3u * stride] = v[3];
	} else {
		const LwPk16 a = pcm_pack_i16((int)v[0], (int)v[1]), b = pcm_pack_i16((int)v[2], (int)v[3]);
		int16_t *o = reinterpret_cast<int16_t *>(out) + e0;
		if (FMT == LW_OUT_I16_PLANAR) {
			store_pcm8(o + e1 + pos, a.u, b.u);
		} else {
			const uint32_t off = pos * stride + e1;
			o[off] = a.s.x;
			o[off + stride] = a.s.y;
			o[off + 2u * stride] = b.s.x;
			o[off + 3u * stride] = b.s.y;
		}
	}
}

// Two consecutive samples (k_big): plain stores at out + elem0 + pos (planar) or out + elem0 + (pos + k) * stride (interleaved)
template <int FMT>
__device__ __forceinline__ void pcm_store2(void *out, uint32_t elem0, uint32_t pos, uint32_t stride, float a, float b)
{
	if (FMT == LW_OUT_F32_PLANAR) {
		*reinterpret_cast<float2_t *>(reinterpret_cast<float *>(out) + elem0 + pos) = float2_t{a, b};
	} else if (FMT == LW_OUT_F32_INTERLEAVED) {
		float *o = reinterpret_cast<float *>(out) + elem0;
		o[pos * stride] = a;
		o[(pos + 1u) * stride] = b;
	} else {
		const LwPk16 v = pcm_pack_i16((int)(a * 32768.0f), (int)(b * 32768.0f));
		int16_t *o = reinterpret_cast<int16_t *>(out) + elem0;
		if (FMT == LW_OUT_I16_PLANAR) {
			*reinterpret_cast<uint32_t *>(o + pos) = v.u;
		} else {
			o[pos * stride] = v.s.x;
			o[(pos + 1u) * stride] = v.s.y;
		}
	}
}

// One sample (k_ola_generic): a plain store at out + idx
template <int FMT>
__device__ __forceinline__ void pcm_store1(void *out, uint32_t idx, float x)
{
	if (lw_out_f32(FMT))
		((float *)out)[idx] = x;
	else
		((int16_t *)out)[idx] = to_i16(x);
}
