// Normalising rows (lw_norm_*, lw_norm_rows; include/lewton_amd.h "normalising rows"): mean removal and scaling by the standard
// deviation, the RMS or the peak of a row, a channel or a line of f32 [row][ch][F][capacity] rows, and the fill, a contract on
// bits whose sums have a fixed order.  Everything about a call is decided here on the host before anything is queued (the
// refusals, the plans, which launches are needed); k_norm_sum, k_norm_fold and k_norm_apply (lw_kernels_norm.hip) do the work.
// The call's per-row records are staged as lw_stage.hpp describes; the chunk lists, the fold's scratch and the scopes' scalars
// live in device arrays of the same rotation.  Nothing else in the library calls into this file.
#include "lw_stage.hpp"
#include "lw_norm.hpp"

#include <cmath>

struct lw_norm {
	int device = 0;
	lw_norm_params p{};
	LwStageRing<LwNormRow> ring;
	LwStageBuf dev[LW_STAGE_SLOTS][3]; // the chunk lists, the fold's scratch (triples), the scalars (doubles)
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
	if (lw_stage_device(device)) {
		*err = LW_ERR_DEVICE;
		return nullptr;
	}
	auto nm = std::make_unique<lw_norm>();
	nm->device = device, nm->p = *p;
	if (!nm->ring.create("hipEventCreate(norm rows)")) {
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
	nm->ring.destroy();
	for (auto &slot : nm->dev)
		for (auto &b : slot)
			b.release();
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
	if (!lw_rows_bytes_ok(lines, capacity, n_rows))
		return LW_ERR_CAPACITY;
	// ---- plan: every row is checked before anything is queued, so a refused call has written nothing
	const bool plain = !nm->p.center && nm->p.scale == LW_NORM_SCALE_NONE; // m = +0.0, g = 1.0: nothing is summed
	nm->rows.clear();
	uint64_t parts = 0;
	LwFillSpan m;
	if (int rc = lw_stage_fill_rows(n_rows, n, fill_to, capacity, d_src, d_dst, m, [&](uint64_t n_i, uint64_t fill_end) {
		    const uint64_t chunks = (n_i + LW_SUM_CHUNK - 1u) / LW_SUM_CHUNK;
		    if (lines * chunks > UINT32_MAX) // (chunks < 2^56, lines < 2^24: the product cannot wrap)
			    return LW_ERR_CAPACITY;
		    nm->rows.push_back(LwNormRow{n_i, fill_end, parts, (uint32_t)chunks, 0u});
		    if (!plain)
			    parts += lines * chunks;
		    return LW_OK;
	    }))
		return rc;
	const uint64_t most = m.most, span = m.span;
	LwNormPlan plan{};
	if (!lw_norm_plan(ch, F, nm->p.scope, most, span, plan))
		return LW_ERR_CAPACITY;
	if (n_rows == 0 || (span == 0 && !d_stats)) {
		nm->last_launches = 0;
		return LW_OK;
	}
	const bool sum = !plain && most != 0, fold = !plain || d_stats;
	// ---- queue: the records, then the launches
	HIP_TRY(hipSetDevice(nm->device));
	hipStream_t st = (hipStream_t)hip_stream;
	if (int rc = nm->ring.acquire(n_rows))
		return rc;
	const uint64_t scopes = (uint64_t)n_rows * plan.scopes;
	const uint64_t need[3] = {sum ? parts * sizeof(LwNormTriple) : 0u, sum ? scopes * plan.fold_scratch * sizeof(LwNormTriple) : 0u,
		fold ? scopes * 2u * sizeof(double) : 0u};
	LwStageBuf(&dev)[3] = nm->dev[nm->ring.next];
	for (int i = 0; i < 3; i++)
		if (int rc = dev[i].reserve(need[i]))
			return rc;
	LwStageGuard staged = nm->ring.guard(st);
	if (int rc = nm->ring.upload(nm->rows, st))
		return rc;
	LwNormArgs a{};
	a.src = (const float *)d_src, a.dst = (float *)d_dst, a.rows = nm->ring.dev(), a.d_stats = d_stats;
	a.part = sum ? (LwNormTriple *)dev[0].p : nullptr, a.scratch = sum ? (LwNormTriple *)dev[1].p : nullptr, a.sc = fold ? (double *)dev[2].p : nullptr;
	a.line_el = capacity, a.ch = ch, a.F = F, a.plan = plan;
	a.center = nm->p.center, a.scale = nm->p.scale, a.scope = nm->p.scope, a.plain = plain, a.eps = nm->p.eps, a.target = nm->p.target;
	int launches = 0;
	for (int pass = 0; pass < 3; pass++) {
		if ((pass == 0 && !sum) || (pass == 1 && !fold) || (pass == 2 && span == 0))
			continue;
		const int k = lw_stage_launch(n_rows, "lw_launch_norm_{sum,fold,apply}", [&](uint32_t row0, uint32_t nr) {
			a.row0 = row0;
			return pass == 0 ? lw_launch_norm_sum(a, nr, st) : pass == 1 ? lw_launch_norm_fold(a, nr, st) : lw_launch_norm_apply(a, nr, st);
		});
		if (k < 0)
			return LW_ERR_DEVICE;
		launches += k;
	}
	if (int rc = staged.commit())
		return rc;
	nm->last_launches = launches;
	return LW_OK;
}

} // extern "C"
