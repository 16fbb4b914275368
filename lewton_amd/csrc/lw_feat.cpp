// Finishing feature rows (lw_feat_*, lw_feat_rows; include/lewton_amd.h "finishing feature rows"): log compression, the
// dynamic-range clamp under a scope's maximum, an affine map and the fill of f32 [row][ch][F][frame_capacity] feature rows, a
// contract on bits.  Everything about a call is decided here on the host before anything is queued (the refusals, the tile plan,
// whether the maximum is needed at all); k_feat_log and k_feat_fin (lw_kernels_feat.hip) do the work.  The call's per-row records
// are staged as lw_stage.hpp describes; the tiles' maxima live in a device array of the same rotation.  Nothing else in the
// library calls into this file.
#include "lw_stage.hpp"
#include "lw_feat.hpp"

#include <cmath>

struct lw_feat {
	int device = 0;
	lw_feat_params p{};
	float l0 = 0.0f;
	LwStageRing<LwFeatRow> ring;
	LwStageBuf part[LW_STAGE_SLOTS]; // the tiles' maxima, floats
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
	if (lw_stage_device(device)) {
		*err = LW_ERR_DEVICE;
		return nullptr;
	}
	auto ft = std::make_unique<lw_feat>();
	ft->device = device, ft->p = *p;
	ft->l0 = lw_feat_log_value(p->log, p->floor);
	if (!ft->ring.create("hipEventCreate(feat rows)")) {
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
	ft->ring.destroy();
	for (auto &b : ft->part)
		b.release();
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
	if (!lw_rows_bytes_ok((uint64_t)ch * F, frame_capacity, n_rows))
		return LW_ERR_CAPACITY;
	// ---- plan: every row is checked before anything is queued, so a refused call has written nothing
	ft->rows.clear();
	LwFillSpan m;
	if (int rc = lw_stage_fill_rows(n_rows, n_frames, fill_to, frame_capacity, d_src, d_dst, m, [&](uint64_t n, uint64_t fill_end) {
		    ft->rows.push_back(LwFeatRow{n, fill_end});
		    return LW_OK;
	    }))
		return rc;
	LwFeatPlan plan{};
	if (!lw_feat_plan(ch, F, m.span, plan))
		return LW_ERR_CAPACITY;
	const bool final = ft->p.top == INFINITY && !d_max; // no maximum is needed: one launch
	if (n_rows == 0 || (m.span == 0 && !d_max)) {
		ft->last_launches = 0;
		return LW_OK;
	}
	// ---- queue: the records, then the launches
	HIP_TRY(hipSetDevice(ft->device));
	hipStream_t st = (hipStream_t)hip_stream;
	if (int rc = ft->ring.acquire(n_rows))
		return rc;
	LwStageBuf &part = ft->part[ft->ring.next];
	if (int rc = part.reserve(final ? 0 : n_rows * (size_t)ch * plan.tiles * sizeof(float)))
		return rc;
	LwStageGuard staged = ft->ring.guard(st);
	if (int rc = ft->ring.upload(ft->rows, st))
		return rc;
	LwFeatArgs a{};
	a.src = (const float *)d_src, a.dst = (float *)d_dst, a.part = final ? nullptr : (float *)part.p, a.d_max = d_max, a.rows = ft->ring.dev();
	a.line_el = frame_capacity, a.ch = ch, a.F = F, a.plan = plan;
	a.log = ft->p.log, a.scope = ft->p.scope, a.floor = ft->p.floor, a.top = ft->p.top, a.add = ft->p.add, a.mul = ft->p.mul;
	a.l0 = ft->l0, a.final = final;
	int launches = 0;
	for (int pass = 0; pass < (final ? 1 : 2); pass++) {
		const int k = lw_stage_launch(n_rows, "lw_launch_feat_{log,fin}", [&](uint32_t row0, uint32_t n) {
			a.row0 = row0;
			return pass == 0 ? lw_launch_feat_log(a, n, st) : lw_launch_feat_fin(a, n, st);
		});
		if (k < 0)
			return LW_ERR_DEVICE;
		launches += k;
	}
	if (int rc = staged.commit())
		return rc;
	ft->last_launches = launches;
	return LW_OK;
}

} // extern "C"
