// Sliding-window normalisation of feature rows (lw_slide_*, lw_slide_rows; include/lewton_amd.h "sliding-window normalisation of
// feature rows"): Kaldi's apply-cmvn-sliding over f32 [row][ch][F][frame_capacity] rows -- a contract on bits with a fixed order
// of its double sums.  Everything about a call is decided here on the host before anything is queued (the refusals, the tile
// plan); k_slide (lw_kernels_slide.hip) does the work in one launch per 65535 rows.  The call's per-row records are staged as
// lw_stage.hpp describes.  Nothing else in the library calls into this file.
#include "lw_stage.hpp"
#include "lw_slide.hpp"

static_assert(LW_SL_MAX_WINDOW == LW_SLIDE_MAX_WINDOW, "the kernel's limit is the header's");

struct lw_slide {
	int device = 0;
	lw_slide_params p{};
	int lds_limit = 0;
	uint32_t tile = LW_SL_TILE;
	LwStageRing<LwSlideRow> ring;
	int last_launches = -1;
	std::vector<LwSlideRow> rows;
};

extern "C" {

lw_slide *lw_slide_create(int device, const lw_slide_params *p, int *err)
{
	int dummy;
	if (!err)
		err = &dummy;
	*err = LW_OK;
	if (!p) {
		*err = LW_ERR_NULL_ARG;
		return nullptr;
	}
	if (p->min_cmn_window < 1 || p->min_cmn_window > p->cmn_window || p->cmn_window > LW_SLIDE_MAX_WINDOW || (p->center != 0 && p->center != 1) ||
			(p->norm_vars != 0 && p->norm_vars != 1)) {
		*err = LW_ERR_UNSUPPORTED;
		return nullptr;
	}
	int lds_limit = 0;
	if (lw_stage_device(device) ||
			!lw_hip_ok(hipDeviceGetAttribute(&lds_limit, hipDeviceAttributeMaxSharedMemoryPerBlock, device), "hipDeviceGetAttribute(LDS per workgroup)") ||
			lds_limit < (int)LW_SL_LDS_BUDGET) { // k_slide plans with the whole budget
		*err = LW_ERR_DEVICE;
		return nullptr;
	}
	auto sl = std::make_unique<lw_slide>();
	sl->device = device, sl->p = *p, sl->lds_limit = lds_limit;
	if (!sl->ring.create("hipEventCreate(slide rows)")) {
		*err = LW_ERR_DEVICE;
		lw_slide_destroy(sl.release());
		return nullptr;
	}
	return sl.release();
}

void lw_slide_destroy(lw_slide *sl)
{
	if (!sl)
		return;
	(void)hipSetDevice(sl->device);
	(void)hipDeviceSynchronize();
	sl->ring.destroy();
	delete sl;
}

int lw_slide_window(const lw_slide *sl, uint64_t t, uint64_t T, uint64_t *start, uint64_t *end)
{
	if (!sl || !start || !end)
		return LW_ERR_NULL_ARG;
	if (t >= T || T > (uint64_t)INT64_MAX)
		return LW_ERR_CAPACITY;
	int64_t s, e;
	lw_slide_window_value(sl->p.cmn_window, sl->p.min_cmn_window, sl->p.center, t, T, s, e);
	*start = (uint64_t)s, *end = (uint64_t)e;
	return LW_OK;
}

uint32_t lw_slide_tile_frames(const lw_slide *sl)
{
	return sl ? sl->tile : 0u;
}

int lw_slide_set_tile_frames(lw_slide *sl, uint32_t tile)
{
	if (!sl)
		return LW_ERR_NULL_ARG;
	LwSlidePlan plan;
	if (!lw_slide_plan(1u, sl->p.cmn_window, tile, plan))
		return LW_ERR_UNSUPPORTED;
	sl->tile = tile;
	return LW_OK;
}

int lw_slide_last_launches(const lw_slide *sl)
{
	return sl ? sl->last_launches : -1;
}

int lw_slide_rows(lw_slide *sl, uint32_t ch, uint32_t F, const void *d_src, void *d_dst, size_t n_rows, size_t frame_capacity,
		const uint64_t *n_frames, const uint64_t *fill_to, void *hip_stream)
{
	if (!sl || (!n_frames && n_rows))
		return LW_ERR_NULL_ARG;
	if (ch == 0 || ch > 255 || F == 0 || F > 65535u || n_rows > UINT32_MAX || frame_capacity > (uint64_t)INT64_MAX)
		return LW_ERR_CAPACITY;
	if (!lw_rows_bytes_ok((uint64_t)ch * F, frame_capacity, n_rows))
		return LW_ERR_CAPACITY;
	// ---- plan: every row is checked before anything is queued, so a refused call has written nothing
	sl->rows.clear();
	LwFillSpan span;
	if (int rc = lw_stage_fill_rows(n_rows, n_frames, fill_to, frame_capacity, d_src, d_dst, span, [&](uint64_t n, uint64_t fill_end) {
			sl->rows.push_back(LwSlideRow{n, fill_end});
			return LW_OK;
		}))
		return rc;
	LwSlidePlan plan;
	if (!lw_slide_plan(F, sl->p.cmn_window, sl->tile, plan))
		return LW_ERR_UNSUPPORTED; // (lw_slide_set_tile_frames has let none such in)
	const uint32_t groups = (F + plan.lines - 1u) / plan.lines;
	const uint64_t tiles = (span.span + plan.tile - 1u) / plan.tile;
	if (tiles > LW_SL_MAX_TILES || tiles * groups > LW_SL_MAX_TILES) // what a grid of 256-lane workgroups can count in its first dimension
		return LW_ERR_CAPACITY;
	if (n_rows == 0 || span.span == 0) {
		sl->last_launches = 0;
		return LW_OK;
	}
	// ---- queue: the records, then the launches
	HIP_TRY(hipSetDevice(sl->device));
	hipStream_t st = (hipStream_t)hip_stream;
	if (int rc = sl->ring.acquire(n_rows))
		return rc;
	LwStageGuard staged = sl->ring.guard(st);
	if (int rc = sl->ring.upload(sl->rows, st))
		return rc;
	LwSlideArgs a{};
	a.rows = sl->ring.dev(), a.line_el = frame_capacity, a.ch = ch, a.F = F, a.W = sl->p.cmn_window, a.min_window = sl->p.min_cmn_window;
	a.center = sl->p.center, a.norm_vars = sl->p.norm_vars, a.groups = groups, a.plan = plan;
	const int launches = lw_stage_launch(n_rows, "lw_launch_slide", [&](uint32_t row0, uint32_t n) {
		a.row0 = row0;
		return lw_launch_slide(a, (const float *)d_src, (float *)d_dst, (uint32_t)tiles, n, st);
	});
	if (launches < 0)
		return LW_ERR_DEVICE;
	if (int rc = staged.commit())
		return rc;
	sl->last_launches = launches;
	return LW_OK;
}

} // extern "C"
