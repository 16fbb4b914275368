// Finishing feature rows (lw_feat_*, lw_feat_rows; include/lewton_amd.h "finishing feature rows"): log compression, the
// dynamic-range clamp under a scope's maximum, an affine map and the fill of f32 [row][ch][F][frame_capacity] feature rows, a
// contract on bits.  Everything about a call is decided here on the host before anything is queued (the refusals, the tile plan,
// whether the maximum is needed at all); k_feat_log and k_feat_fin (lw_kernels_feat.hip) do the work.  The call's per-row records
// travel through pinned arrays in rotation, each guarded by an event, as lw_spec_rows' do; the tiles' maxima live in a device
// array of the same rotation.  Nothing else in the library calls into this file.
#include "lw_internal.hpp"
#include "lw_feat.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

#define LW_FT_SLOTS 3 // record arrays in rotation: calls queued back to back do not wait for each other's kernels

struct lw_ft_slot {
	LwFeatRow *h = nullptr, *d = nullptr; // pinned / device, cap records each
	size_t cap = 0;
	float *part = nullptr; // device, part_cap floats
	size_t part_cap = 0;
	hipEvent_t done = nullptr; // recorded behind the last launch that read d or part
	bool pending = false;
};

struct lw_feat {
	int device = 0;
	lw_feat_params p{};
	float l0 = 0.0f;
	lw_ft_slot slot[LW_FT_SLOTS];
	unsigned next = 0;
	int last_launches = -1;
	std::vector<LwFeatRow> rows;
};

extern "C" {

lw_feat *lw_feat_create(int device, const lw_feat_params *p, int *err)
{
	int dummy;
	if (!err)
		err = &dummy;
	*err = LW_OK;
	if (!p) {
		*err = LW_ERR_NULL_ARG;
		return nullptr;
	}
	const bool logs = p->log != LW_FEAT_LOG_NONE;
	if (p->log < LW_FEAT_LOG_NONE || p->log > LW_FEAT_LOG_DB || (p->scope != LW_FEAT_SCOPE_ROW && p->scope != LW_FEAT_SCOPE_CHANNEL) ||
			std::isnan(p->floor) || (logs && !(p->floor > 0.0f && std::isfinite(p->floor))) || std::isnan(p->top) || p->top < 0.0f ||
			std::isnan(p->add) || std::isnan(p->mul)) {
		*err = LW_ERR_UNSUPPORTED;
		return nullptr;
	}
	int ndev = 0;
	if (!lw_hip_ok(hipGetDeviceCount(&ndev), "hipGetDeviceCount") || device < 0 || device >= ndev || !lw_hip_ok(hipSetDevice(device), "hipSetDevice")) {
		*err = LW_ERR_DEVICE;
		return nullptr;
	}
	auto ft = std::make_unique<lw_feat>();
	ft->device = device, ft->p = *p;
	ft->l0 = lw_feat_log_value(p->log, p->floor);
	bool ok = true;
	for (auto &sl : ft->slot)
		ok = ok && lw_hip_ok(hipEventCreateWithFlags(&sl.done, hipEventDisableTiming), "hipEventCreate(feat rows)");
	if (!ok) {
		*err = LW_ERR_DEVICE;
		lw_feat_destroy(ft.release());
		return nullptr;
	}
	return ft.release();
}

void lw_feat_destroy(lw_feat *ft)
{
	if (!ft)
		return;
	(void)hipSetDevice(ft->device);
	(void)hipDeviceSynchronize();
	for (auto &s : ft->slot) {
		if (s.h)
			(void)hipHostFree(s.h);
		if (s.d)
			(void)hipFree(s.d);
		if (s.part)
			(void)hipFree(s.part);
		if (s.done)
			(void)hipEventDestroy(s.done);
	}
	delete ft;
}

float lw_feat_log(const lw_feat *ft, float v)
{
	if (!ft || std::isnan(v) || (ft->p.log != LW_FEAT_LOG_NONE && !(v > 0.0f)))
		return NAN;
	return lw_feat_log_value(ft->p.log, v);
}

int lw_feat_last_launches(const lw_feat *ft)
{
	return ft ? ft->last_launches : -1;
}

int lw_feat_rows(lw_feat *ft, uint32_t ch, uint32_t F, const void *d_src, void *d_dst, size_t n_rows, size_t frame_capacity, const uint64_t *n_frames,
		const uint64_t *fill_to, float *d_max, void *hip_stream)
{
	if (!ft || (!n_frames && n_rows))
		return LW_ERR_NULL_ARG;
	if (ch == 0 || ch > 255 || F == 0 || F > 65535 || n_rows > UINT32_MAX)
		return LW_ERR_CAPACITY;
	uint64_t e = 0; // the buffer must be addressable in 64 bits of BYTES
	if (__builtin_mul_overflow((uint64_t)ch * F, (uint64_t)frame_capacity, &e) || __builtin_mul_overflow(e, (uint64_t)n_rows, &e) || e > UINT64_MAX / 4)
		return LW_ERR_CAPACITY;
	// ---- plan: every row is checked before anything is queued, so a refused call has written nothing
	ft->rows.clear();
	uint64_t most = 0, span = 0;
	for (size_t i = 0; i < n_rows; i++) {
		const uint64_t fill = fill_to ? fill_to[i] : 0;
		if (n_frames[i] > frame_capacity || fill > frame_capacity)
			return LW_ERR_CAPACITY;
		ft->rows.push_back(LwFeatRow{n_frames[i], std::max(n_frames[i], fill)});
		most = std::max(most, n_frames[i]);
		span = std::max(span, ft->rows.back().fill_end);
	}
	if ((most && !d_src) || (span && !d_dst))
		return LW_ERR_NULL_ARG;
	LwFeatPlan plan{};
	if (!lw_feat_plan(ch, F, span, plan))
		return LW_ERR_CAPACITY;
	const bool final = ft->p.top == INFINITY && !d_max; // no maximum is needed: one launch
	if (n_rows == 0 || (span == 0 && !d_max)) {
		ft->last_launches = 0;
		return LW_OK;
	}
	// ---- queue: the records, then the launches, 65535 rows each
	HIP_TRY(hipSetDevice(ft->device));
	hipStream_t st = (hipStream_t)hip_stream;
	lw_ft_slot &s = ft->slot[ft->next];
	if (s.pending) { // an earlier call's copy of these records, or its maxima, may still be in use
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
		HIP_TRY(hipHostMalloc((void **)&s.h, cap * sizeof(LwFeatRow), 0));
		HIP_TRY(hipMalloc((void **)&s.d, cap * sizeof(LwFeatRow)));
		s.cap = cap;
	}
	const size_t parts = final ? 0 : n_rows * (size_t)ch * plan.tiles;
	if (s.part_cap < parts) {
		if (s.part)
			(void)hipFree(s.part);
		s.part = nullptr;
		s.part_cap = 0;
		HIP_TRY(hipMalloc((void **)&s.part, parts * sizeof(float)));
		s.part_cap = parts;
	}
	std::memcpy(s.h, ft->rows.data(), n_rows * sizeof(LwFeatRow));
	HIP_TRY(hipMemcpyAsync(s.d, s.h, n_rows * sizeof(LwFeatRow), hipMemcpyHostToDevice, st));
	LwFeatArgs a{};
	a.src = (const float *)d_src, a.dst = (float *)d_dst, a.part = final ? nullptr : s.part, a.d_max = d_max, a.rows = s.d;
	a.line_el = frame_capacity, a.ch = ch, a.F = F, a.plan = plan;
	a.log = ft->p.log, a.scope = ft->p.scope, a.floor = ft->p.floor, a.top = ft->p.top, a.add = ft->p.add, a.mul = ft->p.mul;
	a.l0 = ft->l0, a.final = final;
	int launches = 0;
	for (int pass = 0; pass < (final ? 1 : 2); pass++)
		for (size_t r0 = 0; r0 < n_rows; r0 += 65535) {
			a.row0 = (uint32_t)r0;
			const uint32_t n = (uint32_t)std::min<size_t>(n_rows - r0, 65535);
			HIP_TRY(pass == 0 ? lw_launch_feat_log(a, n, st) : lw_launch_feat_fin(a, n, st));
			launches++;
		}
	HIP_TRY(hipEventRecord(s.done, st));
	s.pending = true;
	ft->last_launches = launches;
	ft->next = (ft->next + 1) % LW_FT_SLOTS;
	return LW_OK;
}

} // extern "C"
