// Normalising rows (lw_norm_*, lw_norm_rows; include/lewton_amd.h "normalising rows"): mean removal and scaling by the standard
// deviation, the RMS or the peak of a row, a channel or a line of f32 [row][ch][F][capacity] rows, and the fill, a contract on
// bits whose sums have a fixed order.  Everything about a call is decided here on the host before anything is queued (the
// refusals, the plans, which launches are needed); k_norm_sum, k_norm_fold and k_norm_apply (lw_kernels_norm.hip) do the work.
// The call's per-row records travel through pinned arrays in rotation, each guarded by an event, as lw_feat_rows' do; the chunk
// lists, the fold's scratch and the scopes' scalars live in device arrays of the same rotation.  Nothing else in the library
// calls into this file.
#include "lw_internal.hpp"
#include "lw_norm.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

#define LW_NM_SLOTS 3 // record arrays in rotation: calls queued back to back do not wait for each other's kernels

struct lw_nm_slot {
	LwNormRow *h = nullptr, *d = nullptr; // pinned / device, cap records each
	size_t cap = 0;
	void *dev[3] = {nullptr, nullptr, nullptr}; // device: the chunk lists, the fold's scratch (triples), the scalars (doubles)
	size_t dev_cap[3] = {0, 0, 0};              // bytes
	hipEvent_t done = nullptr;                  // recorded behind the last launch that read d or wrote dev
	bool pending = false;
};

struct lw_norm {
	int device = 0;
	lw_norm_params p{};
	lw_nm_slot slot[LW_NM_SLOTS];
	unsigned next = 0;
	int last_launches = -1;
	std::vector<LwNormRow> rows;
};

extern "C" {

lw_norm *lw_norm_create(int device, const lw_norm_params *p, int *err)
{
	int dummy;
	if (!err)
		err = &dummy;
	*err = LW_OK;
	if (!p) {
		*err = LW_ERR_NULL_ARG;
		return nullptr;
	}
	const bool targeted = p->scale == LW_NORM_SCALE_RMS || p->scale == LW_NORM_SCALE_PEAK;
	if (p->scale < LW_NORM_SCALE_NONE || p->scale > LW_NORM_SCALE_PEAK || p->scope < LW_NORM_SCOPE_ROW || p->scope > LW_NORM_SCOPE_LINE ||
			(p->center != 0 && p->center != 1) || p->reserved != 0 || !(p->eps >= 0.0 && std::isfinite(p->eps)) ||
			(targeted && !(p->target > 0.0 && std::isfinite(p->target)))) {
		*err = LW_ERR_UNSUPPORTED;
		return nullptr;
	}
	int ndev = 0;
	if (!lw_hip_ok(hipGetDeviceCount(&ndev), "hipGetDeviceCount") || device < 0 || device >= ndev || !lw_hip_ok(hipSetDevice(device), "hipSetDevice")) {
		*err = LW_ERR_DEVICE;
		return nullptr;
	}
	auto nm = std::make_unique<lw_norm>();
	nm->device = device, nm->p = *p;
	bool ok = true;
	for (auto &sl : nm->slot)
		ok = ok && lw_hip_ok(hipEventCreateWithFlags(&sl.done, hipEventDisableTiming), "hipEventCreate(norm rows)");
	if (!ok) {
		*err = LW_ERR_DEVICE;
		lw_norm_destroy(nm.release());
		return nullptr;
	}
	return nm.release();
}

void lw_norm_destroy(lw_norm *nm)
{
	if (!nm)
		return;
	(void)hipSetDevice(nm->device);
	(void)hipDeviceSynchronize();
	for (auto &s : nm->slot) {
		if (s.h)
			(void)hipHostFree(s.h);
		if (s.d)
			(void)hipFree(s.d);
		for (void *p : s.dev)
			if (p)
				(void)hipFree(p);
		if (s.done)
			(void)hipEventDestroy(s.done);
	}
	delete nm;
}

int lw_norm_scalars(const lw_norm *nm, double S1, double S2, float P, uint64_t N, double *m, double *g)
{
	if (!nm || !m || !g)
		return LW_ERR_NULL_ARG;
	lw_norm_scalars_value(nm->p.center, nm->p.scale, nm->p.eps, nm->p.target, S1, S2, P, N, *m, *g);
	return LW_OK;
}

int lw_norm_last_launches(const lw_norm *nm)
{
	return nm ? nm->last_launches : -1;
}

int lw_norm_rows(lw_norm *nm, uint32_t ch, uint32_t F, const void *d_src, void *d_dst, size_t n_rows, size_t capacity, const uint64_t *n,
		const uint64_t *fill_to, double *d_stats, void *hip_stream)
{
	if (!nm || (!n && n_rows))
		return LW_ERR_NULL_ARG;
	if (ch == 0 || ch > 255 || F == 0 || F > 65535 || n_rows > UINT32_MAX)
		return LW_ERR_CAPACITY;
	const uint64_t lines = (uint64_t)ch * F;
	uint64_t e = 0; // the buffer must be addressable in 64 bits of BYTES
	if (__builtin_mul_overflow(lines, (uint64_t)capacity, &e) || __builtin_mul_overflow(e, (uint64_t)n_rows, &e) || e > UINT64_MAX / 4)
		return LW_ERR_CAPACITY;
	// ---- plan: every row is checked before anything is queued, so a refused call has written nothing
	const bool plain = !nm->p.center && nm->p.scale == LW_NORM_SCALE_NONE; // m = +0.0, g = 1.0: nothing is summed
	nm->rows.clear();
	uint64_t most = 0, span = 0, parts = 0;
	for (size_t i = 0; i < n_rows; i++) {
		const uint64_t fill = fill_to ? fill_to[i] : 0;
		if (n[i] > capacity || fill > capacity)
			return LW_ERR_CAPACITY;
		const uint64_t chunks = (n[i] + LW_NM_CHUNK - 1u) / LW_NM_CHUNK;
		if (lines * chunks > UINT32_MAX) // (chunks < 2^56, lines < 2^24: the product cannot wrap)
			return LW_ERR_CAPACITY;
		nm->rows.push_back(LwNormRow{n[i], std::max(n[i], fill), parts, (uint32_t)chunks, 0u});
		if (!plain)
			parts += lines * chunks;
		most = std::max(most, n[i]);
		span = std::max(span, nm->rows.back().fill_end);
	}
	if ((most && !d_src) || (span && !d_dst))
		return LW_ERR_NULL_ARG;
	LwNormPlan plan{};
	if (!lw_norm_plan(ch, F, nm->p.scope, most, span, plan))
		return LW_ERR_CAPACITY;
	if (n_rows == 0 || (span == 0 && !d_stats)) {
		nm->last_launches = 0;
		return LW_OK;
	}
	const bool sum = !plain && most != 0, fold = !plain || d_stats;
	// ---- queue: the records, then the launches, 65535 rows each
	HIP_TRY(hipSetDevice(nm->device));
	hipStream_t st = (hipStream_t)hip_stream;
	lw_nm_slot &s = nm->slot[nm->next];
	if (s.pending) { // an earlier call's copy of these records, or its lists, may still be in use
		HIP_TRY(hipEventSynchronize(s.done));
		s.pending = false;
	}
	if (s.cap < n_rows) {
		if (s.h)
			(void)hipHostFree(s.h);
		if (s.d)
			(void)hipFree(s.d);
		s.h = s.d = nullptr;
		s.cap = 0;
		const size_t cap = std::max<size_t>(n_rows, 64);
		HIP_TRY(hipHostMalloc((void **)&s.h, cap * sizeof(LwNormRow), 0));
		HIP_TRY(hipMalloc((void **)&s.d, cap * sizeof(LwNormRow)));
		s.cap = cap;
	}
	const uint64_t scopes = (uint64_t)n_rows * plan.scopes;
	const uint64_t need[3] = {sum ? parts * sizeof(LwNormTriple) : 0u, sum ? scopes * plan.fold_scratch * sizeof(LwNormTriple) : 0u,
		fold ? scopes * 2u * sizeof(double) : 0u};
	for (int i = 0; i < 3; i++)
		if (s.dev_cap[i] < need[i]) {
			if (s.dev[i])
				(void)hipFree(s.dev[i]);
			s.dev[i] = nullptr;
			s.dev_cap[i] = 0;
			HIP_TRY(hipMalloc(&s.dev[i], need[i]));
			s.dev_cap[i] = need[i];
		}
	std::memcpy(s.h, nm->rows.data(), n_rows * sizeof(LwNormRow));
	HIP_TRY(hipMemcpyAsync(s.d, s.h, n_rows * sizeof(LwNormRow), hipMemcpyHostToDevice, st));
	LwNormArgs a{};
	a.src = (const float *)d_src, a.dst = (float *)d_dst, a.rows = s.d, a.d_stats = d_stats;
	a.part = sum ? (LwNormTriple *)s.dev[0] : nullptr, a.scratch = sum ? (LwNormTriple *)s.dev[1] : nullptr, a.sc = fold ? (double *)s.dev[2] : nullptr;
	a.line_el = capacity, a.ch = ch, a.F = F, a.plan = plan;
	a.center = nm->p.center, a.scale = nm->p.scale, a.scope = nm->p.scope, a.plain = plain, a.eps = nm->p.eps, a.target = nm->p.target;
	int launches = 0;
	for (int pass = 0; pass < 3; pass++) {
		if ((pass == 0 && !sum) || (pass == 1 && !fold) || (pass == 2 && span == 0))
			continue;
		for (size_t r0 = 0; r0 < n_rows; r0 += 65535) {
			a.row0 = (uint32_t)r0;
			const uint32_t nr = (uint32_t)std::min<size_t>(n_rows - r0, 65535);
			HIP_TRY(pass == 0 ? lw_launch_norm_sum(a, nr, st) : pass == 1 ? lw_launch_norm_fold(a, nr, st) : lw_launch_norm_apply(a, nr, st));
			launches++;
		}
	}
	HIP_TRY(hipEventRecord(s.done, st));
	s.pending = true;
	nm->last_launches = launches;
	nm->next = (nm->next + 1) % LW_NM_SLOTS;
	return LW_OK;
}

} // extern "C"
