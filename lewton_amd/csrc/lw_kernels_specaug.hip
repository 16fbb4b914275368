// SpecAugment masks (product code, gfx950): k_specaug, the kernel of lw_specaug_rows.  ONE pass over f32 [row][ch][F][frame_capacity]
// rows by the rule of include/lewton_amd.h ("masking feature rows"): an element is `fill` where a time mask of its group holds its
// frame or a frequency mask holds its line, else a bit copy of the source; positions [T, fill_end) of every line receive +0.0.
// The masks are a pure function of (seed, id, group, kind, number) through lw_sa_span (lw_specaug.hpp, on lw_rng.hpp's Philox), so
// every workgroup draws its group's masks AGAIN rather than read them from anywhere: no launch in front of this one, no list.
//   A workgroup of 256 lanes takes one tile of one line (row, c, f):
//   SPANS   lane k < num_t + num_f evaluates ONE mask into LDS, time masks first (at most 1 KiB); one barrier.  The workgroup of
//           tile 0, line 0 of a group stores the group's (start, end) pairs into d_spans.
//   STREAM  the tile's share of [0, fill_end) in groups of four consecutive frames at a 16-byte boundary of the DESTINATION's
//           address.  A group that lies whole inside the share leaves as ONE 16-byte store, and arrives by ONE 16-byte load where
//           the source's address allows it and all four frames are below T; the ragged head and tail of the share (frame_capacity
//           may be odd: a line starts anywhere) go dword by dword.  A group whose four frames are all masked is not loaded at all,
//           nor is anything of a line that a frequency mask holds.
//   IN PLACE (src == dst)  a workgroup whose tile meets no mask and no fill span returns without touching memory; otherwise it
//           stores fill over the intersections and +0.0 over the fill span, and loads nothing.
// The elements travel as uint32: fill's own bits, NaN payloads and -0.0 arrive as they are.  Offsets and frame numbers in 64 bits
// (a row may have more than 2^32 frames, a tensor more than 2^32 elements).  No atomics, no wait of a workgroup on another.  Nothing
// at or beyond T of the source is read, nothing outside [0, fill_end) of a line is written.  A frame is tested against each time
// mask of the group by two compares on a whole group of four (the bits of [start, end) that fall into it): with the two to ten
// masks of the recipes that is cheaper than a bit list of the tile in LDS, which costs the same compares per FRAME to build.
// tests/san/specaug_host.cpp compiles this file for the host (LW_KERNEL_HOST) and runs lw_sa_workgroup, the kernels' own driver
// of the phases, workgroup by workgroup.
#include "lw_specaug.hpp"

#ifndef LW_KERNEL_HOST
#include "lw_kernels.hpp"
#endif

typedef uint32_t LwSaU4 __attribute__((vector_size(16)));

struct LwSaLds { // the LDS of a workgroup
	uint64_t span[2u * LW_SA_MAX_MASKS][2]; // (start, end): time masks 0 .. num_t - 1, then the frequency masks
};
static_assert(sizeof(LwSaLds) == LW_SA_LDS, "LW_SA_LDS is the structure's size");

struct LwSaTile { // what a workgroup works on; the same for all its lanes
	uint64_t n, fill_end, id;
	uint64_t t0, end;  // the tile's share of [0, fill_end): [t0, end), empty where t0 >= end
	uint64_t at;       // element of frame 0 of the line
	uint64_t spans_at; // first int64 of the group's pairs in a.spans
	uint32_t f, group;
	bool owes;         // this workgroup stores the group's spans
};

LW_LANES_FN void lw_sa_tile(const LwSaArgs &a, uint32_t bx, uint32_t by, uint32_t bz, LwSaTile &t)
{
	const uint64_t row = (uint64_t)a.row0 + bz;
	const LwSaRow r = a.rows[row];
	const uint32_t tile_i = bx % a.tiles;
	t.n = r.n, t.fill_end = r.fill_end, t.id = r.id;
	t.f = bx / a.tiles;
	t.group = a.per_channel ? by : 0u;
	t.t0 = (uint64_t)tile_i * a.tile;
	t.end = t.t0 + a.tile < t.fill_end ? t.t0 + a.tile : t.fill_end;
	t.at = ((row * a.ch + by) * a.F + t.f) * a.line_el;
	const uint32_t masks = a.rule.num_t + a.rule.num_f;
	t.spans_at = (row * (a.per_channel ? a.ch : 1u) + t.group) * masks * 2u;
	t.owes = a.spans && masks && tile_i == 0 && t.f == 0 && (a.per_channel || by == 0);
}

// a workgroup with nothing to write and no spans to store has nothing to do (the same in every lane)
LW_LANES_FN bool lw_sa_idle(const LwSaTile &t)
{
	return t.t0 >= t.end && !t.owes;
}

// ---- SPANS: lane tid's mask of the group into LDS, and into d_spans where this workgroup owes them
LW_LANES_FN void lw_sa_spans_lane(const LwSaArgs &a, const LwSaTile &t, LwSaLds &l, uint32_t tid)
{
	const uint32_t masks = a.rule.num_t + a.rule.num_f;
	if (tid >= masks)
		return;
	const bool time = tid < a.rule.num_t;
	uint64_t start, end;
	lw_sa_span(a.rule, t.id, t.group, time ? LW_SA_TIME : LW_SA_FREQ, time ? tid : tid - a.rule.num_t, time ? t.n : (uint64_t)a.F, start, end);
	l.span[tid][0] = start, l.span[tid][1] = end;
	if (t.owes)
		a.spans[t.spans_at + 2u * tid] = (int64_t)start, a.spans[t.spans_at + 2u * tid + 1u] = (int64_t)end;
}

// (behind the barrier) whether a frequency mask holds the line
LW_LANES_FN bool lw_sa_line_masked(const LwSaArgs &a, const LwSaTile &t, const LwSaLds &l)
{
	bool m = false;
	for (uint32_t k = a.rule.num_t; k < a.rule.num_t + a.rule.num_f; k++)
		m = m || (l.span[k][0] <= t.f && t.f < l.span[k][1]);
	return m;
}

// bit j: frame g0 + j is in [lo, hi) (g0 may be -3 .. -1 at the head of a line)
LW_LANES_FN uint32_t lw_sa_bits(int64_t g0, int64_t lo, int64_t hi)
{
	if (lo >= g0 + 4 || hi <= g0 || lo >= hi)
		return 0u;
	const uint32_t b = lo > g0 ? (uint32_t)(lo - g0) : 0u, e = hi < g0 + 4 ? (uint32_t)(hi - g0) : 4u;
	return ((1u << e) - 1u) & ~((1u << b) - 1u);
}

// bit j: frame g0 + j is inside a time mask of the group
LW_LANES_FN uint32_t lw_sa_time_bits(const LwSaArgs &a, const LwSaLds &l, int64_t g0)
{
	uint32_t m = 0;
	for (uint32_t k = 0; k < a.rule.num_t; k++)
		m |= lw_sa_bits(g0, (int64_t)l.span[k][0], (int64_t)l.span[k][1]);
	return m;
}

// (in place) whether the tile has an element to write: a fill span, a masked line with frames, or a time mask that meets its frames
LW_LANES_FN bool lw_sa_tile_written(const LwSaArgs &a, const LwSaTile &t, const LwSaLds &l, bool line_masked)
{
	if (t.t0 >= t.end)
		return false;
	if (t.end > t.n) // positions at or beyond T: the fill span
		return true;
	if (line_masked)
		return true;
	bool any = false;
	for (uint32_t k = 0; k < a.rule.num_t; k++)
		any = any || (l.span[k][0] < t.end && l.span[k][1] > t.t0 && l.span[k][0] < l.span[k][1]);
	return any;
}

// ---- STREAM: lane tid's groups of four of the tile's share [t0, end)
template <bool IN_PLACE>
LW_LANES_FN void lw_sa_stream(const LwSaArgs &a, const LwSaTile &t, const LwSaLds &l, bool line_masked, uint32_t tid)
{
	if (t.t0 >= t.end)
		return;
	uint32_t *dst = a.dst + t.at;
	const uint32_t head = (uint32_t)(((uintptr_t)(dst + t.t0) >> 2) & 3u); // elements of the first group in front of t0
	const uint32_t groups = (uint32_t)((t.end - t.t0 + head + 3u) / 4u);
	const bool src_sits = ((((uintptr_t)a.src ^ (uintptr_t)a.dst) >> 2) & 3u) == 0; // the source's groups are at 16-byte boundaries too
	for (uint32_t g = tid; g < groups; g += LW_SA_THREADS) {
		const int64_t g0 = (int64_t)t.t0 - (int64_t)head + (int64_t)g * 4;
		const uint32_t live = lw_sa_bits(g0, (int64_t)t.t0, (int64_t)t.end); // the share's frames of the group
		const uint32_t below = lw_sa_bits(g0, 0, (int64_t)t.n);              // ... those below T
		const uint32_t masked = (line_masked ? 15u : lw_sa_time_bits(a, l, g0)) & below;
		const uint32_t write = IN_PLACE ? live & (masked | ~below) : live;
		if (!write)
			continue;
		uint32_t v[4] = {0u, 0u, 0u, 0u}; // +0.0 at and beyond T
		if (!IN_PLACE) {
			const uint32_t need = live & below & ~masked; // the frames that are copies
			if (need) { // (a group that is all fill or all +0.0 is not loaded)
				const uint32_t *LW_LANES_RESTRICT s = a.src + ((int64_t)t.at + g0);
				if (need == 15u && src_sits) { // ONE 16-byte load
					const LwSaU4 q = *(const LwSaU4 *)s;
					v[0] = q[0], v[1] = q[1], v[2] = q[2], v[3] = q[3];
				} else {
#pragma unroll
					for (uint32_t j = 0; j < 4u; j++)
						if (need >> j & 1u)
							v[j] = s[j];
				}
			}
		}
#pragma unroll
		for (uint32_t j = 0; j < 4u; j++)
			if (masked >> j & 1u)
				v[j] = a.fill;
		if (write == 15u) { // ONE 16-byte store
			LwSaU4 q;
			q[0] = v[0], q[1] = v[1], q[2] = v[2], q[3] = v[3];
			*(LwSaU4 *)(dst + g0) = q;
			continue;
		}
#pragma unroll
		for (uint32_t j = 0; j < 4u; j++)
			if (write >> j & 1u)
				dst[g0 + (int64_t)j] = v[j];
	}
}

// ---- what a workgroup does, in this order: ONE source for the kernels below and for tests/san/specaug_host.cpp.  lanes(phase,
// barrier) runs phase(tid) for the workgroup's lanes and, where barrier is set, ends at the workgroup's barrier: on the device
// the lane itself and __syncthreads(), on the host a loop over the 256 lanes.  Both returns are the same in every lane
template <bool IN_PLACE, class Lanes>
LW_LANES_FN void lw_sa_workgroup(const LwSaArgs &a, LwSaLds &l, uint32_t bx, uint32_t by, uint32_t bz, const Lanes &lanes)
{
	LwSaTile t;
	lw_sa_tile(a, bx, by, bz, t);
	if (lw_sa_idle(t))
		return;
	lanes([&](uint32_t tid) { lw_sa_spans_lane(a, t, l, tid); }, true);
	const bool line_masked = lw_sa_line_masked(a, t, l);
	if (IN_PLACE && !lw_sa_tile_written(a, t, l, line_masked))
		return;
	lanes([&](uint32_t tid) { lw_sa_stream<IN_PLACE>(a, t, l, line_masked, tid); }, false);
}

#ifndef LW_KERNEL_HOST

template <bool IN_PLACE>
LW_LANES_FN void lw_sa_on_device(const LwSaArgs &a, LwSaLds &l)
{
	lw_sa_workgroup<IN_PLACE>(a, l, blockIdx.x, blockIdx.y, blockIdx.z, [](const auto &phase, bool barrier) {
		phase(threadIdx.x);
		if (barrier)
			__syncthreads();
	});
}

__global__ void __launch_bounds__(LW_SA_THREADS) k_specaug(LwSaArgs a)
{
	__shared__ LwSaLds l;
	lw_sa_on_device<false>(a, l);
}

__global__ void __launch_bounds__(LW_SA_THREADS) k_specaug_inplace(LwSaArgs a)
{
	__shared__ LwSaLds l;
	lw_sa_on_device<true>(a, l);
}

hipError_t lw_launch_specaug(const LwSaArgs &a, uint32_t n_rows, hipStream_t st)
{
	if (n_rows == 0 || n_rows > 65535u || a.ch == 0 || a.ch > 65535u || a.F == 0 || !a.rows || !lw_sa_tile_ok(a.tile) || a.tiles == 0 ||
			(uint64_t)a.tiles * a.F > LW_SA_MAX_TILES || a.rule.num_t > LW_SA_MAX_MASKS || a.rule.num_f > LW_SA_MAX_MASKS)
		return hipErrorInvalidValue;
	const dim3 grid(a.tiles * a.F, a.ch, n_rows);
	return a.src == a.dst ? lw_launch_k(k_specaug_inplace, grid, dim3(LW_SA_THREADS), 0, st, a) : lw_launch_k(k_specaug, grid, dim3(LW_SA_THREADS), 0, st, a);
}

#endif // LW_KERNEL_HOST
