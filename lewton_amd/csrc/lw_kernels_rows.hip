// Stream-major rows (product code, gfx950): k_rows, a segmented copy that runs behind the synthesis kernels on the same HIP
// stream and moves their packet-major PCM into [row][channel][sample] (planar) or [row][sample][channel] (interleaved) device
// buffers.  The synthesis kernels and their store primitives do not know about it.
//
// Work: a list of pieces {source element, count, destination element} the host has cut (lw_rows.cpp) to at most
// LW_ROWS_PIECE elements each, one WAVE per piece, four pieces per workgroup, the grid capped and a grid stride behind it.
// A piece moves a scalar head up to the next 16-byte boundary of its DESTINATION, then 16-byte vectors (every load of the piece
// issued before its first store: at most LW_ROWS_PIECE * 4 / 16 / 64 = 8 per lane), then a scalar tail.  The vector loads carry
// only the element's alignment: when source and destination are congruent mod 16 -- the common case, a packet yields a multiple
// of 16 samples and rows start aligned -- they are aligned dwordx4 loads; behind an odd skip, in a row of odd capacity or in
// interleaved 5.1 after a skip the same instruction reads across 16-byte lines and the stores stay aligned.
//
// Every destination address is formed in 64 bits (a rows tensor passes 2^32 elements at three stereo rows of 2^30 samples);
// source offsets are 32-bit like the batch's output offsets.  Nothing outside [dst, dst + count) is written.
// Bound: HBM bandwidth (one read and one write of the batch's PCM); no LDS, no scratch.
#include "lw_kernels.hpp"

#include <hip/hip_runtime.h>

#define LW_ROWS_WAVES 4u       // pieces per workgroup pass
#define LW_ROWS_MAX_GRID 2048u // workgroups; the rest of the list by grid stride

template <int ES> struct LwRowsElem;
template <> struct LwRowsElem<2> { typedef uint16_t type; };
template <> struct LwRowsElem<4> { typedef uint32_t type; };

// 16 bytes at an address that is only aligned like an element (one global_load_dwordx4 all the same)
typedef uint32_t lw_rows_u32x4 __attribute__((ext_vector_type(4)));
template <int ES> struct __attribute__((packed, aligned(ES))) LwRowsVec {
	lw_rows_u32x4 v;
};

template <int ES> // element size in bytes
__global__ void __launch_bounds__(64 * LW_ROWS_WAVES) k_rows(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst,
		const LwRowSeg *__restrict__ segs, uint32_t n)
{
	typedef typename LwRowsElem<ES>::type E;
	constexpr uint32_t EPV = 16 / ES;                      // elements per vector
	constexpr uint32_t VPL = LW_ROWS_PIECE / EPV / 64;     // vectors per lane and pass
	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); // wave-uniform: the descriptor comes in by scalar loads
	for (uint32_t p = blockIdx.x * LW_ROWS_WAVES + wave; p < n; p += gridDim.x * LW_ROWS_WAVES) {
		const LwRowSeg s = segs[p];
		const uint8_t *sp = src + (size_t)s.src_elem * ES;
		uint8_t *dp = dst + (size_t)s.dst_elem * ES; // 64-bit from the descriptor to the store address
		const uint32_t count = s.count;
		uint32_t head = (uint32_t)((16u - ((uintptr_t)dp & 15u)) & 15u) / ES;
		head = head < count ? head : count;
		if (lane < head)
			((E *)dp)[lane] = ((const E *)sp)[lane];
		const uint32_t nvec = (count - head) / EPV;
		const uint8_t *vs = sp + (size_t)head * ES;
		lw_rows_u32x4 *vd = (lw_rows_u32x4 *)__builtin_assume_aligned(dp + (size_t)head * ES, 16);
		for (uint32_t base = 0; base < nvec; base += 64u * VPL) { // (one pass for a piece the host has cut)
			lw_rows_u32x4 v[VPL];
#pragma unroll
			for (uint32_t k = 0; k < VPL; k++) {
				const uint32_t i = base + k * 64u + lane;
				v[k] = i < nvec ? ((const LwRowsVec<ES> *)vs)[i].v : lw_rows_u32x4{0, 0, 0, 0};
			}
#pragma unroll
			for (uint32_t k = 0; k < VPL; k++) {
				const uint32_t i = base + k * 64u + lane;
				if (i < nvec)
					vd[i] = v[k];
			}
		}
		const uint32_t done = head + nvec * EPV, tail = count - done; // tail < EPV
		if (lane < tail)
			((E *)dp)[done + lane] = ((const E *)sp)[done + lane];
	}
}

hipError_t lw_launch_rows(const void *d_src, void *d_dst, const LwRowSeg *d_segs, uint32_t n_segs, int elem_size, hipStream_t st)
{
	if (n_segs == 0)
		return hipSuccess;
	if (elem_size != 2 && elem_size != 4)
		return hipErrorInvalidValue;
	const uint32_t groups = (n_segs + LW_ROWS_WAVES - 1) / LW_ROWS_WAVES;
	const dim3 grid(groups < LW_ROWS_MAX_GRID ? groups : LW_ROWS_MAX_GRID), block(64 * LW_ROWS_WAVES);
	const uint8_t *src = (const uint8_t *)d_src;
	uint8_t *dst = (uint8_t *)d_dst;
	if (elem_size == 2)
		return lw_launch_k(k_rows<2>, grid, block, 0, st, src, dst, d_segs, n_segs);
	return lw_launch_k(k_rows<4>, grid, block, 0, st, src, dst, d_segs, n_segs);
}
