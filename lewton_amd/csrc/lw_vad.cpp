// Energy voice-activity decisions (lw_vad_*, lw_vad_rows; include/lewton_amd.h "energy voice-activity decisions of feature rows"):
// Kaldi's compute-vad-energy over one line of f32 [row][ch][F][frame_capacity] rows, into a uint8 mask [row][ch][frame_capacity]
// that lw_select_rows takes -- a contract on bits.  Everything about a call is decided here on the host before anything is queued
// (the refusals, the form); the kernels of lw_kernels_vad.hip do the work: k_vad in one launch per 65535 rows while every row's
// span is at most LW_VAD_FUSED_MAX frames, k_vad_sum, k_vad_fold and k_vad_decide otherwise, k_vad_decide alone without a mean.
// The call's per-row records are staged as lw_stage.hpp describes; the chunk lists, the fold's levels and the thresholds of the
// split form go through scratch of the same rotation.  Nothing else in the library calls into this file.
#include "lw_stage.hpp"
#include "lw_vad.hpp"

#include <cmath>

static_assert(LW_VD_MAX_CONTEXT == LW_VAD_MAX_CONTEXT && LW_VD_FUSED_MAX == LW_VAD_FUSED_MAX, "the kernels' limits are the header's");

struct lw_vad {
	int device = 0;
	lw_vad_params p{};
	uint32_t tile = LW_VD_TILE;
	int route = LW_VAD_ROUTE_AUTO;
	LwStageRing<LwVadRow> ring;
	LwStageBuf scratch[LW_STAGE_SLOTS]; // split form: the chunk lists, the fold's levels, the thresholds of the call that holds the slot
	int last_launches = -1;
	std::vector<LwVadRow> rows;
};

extern "C" {

lw_vad *lw_vad_create(int device, const lw_vad_params *p, int *err)
{
	int dummy;
	if (!err)
		err = &dummy;
	*err = LW_OK;
	if (!p) {
		*err = LW_ERR_NULL_ARG;
		return nullptr;
	}
	if (!std::isfinite(p->energy_threshold) || !std::isfinite(p->energy_mean_scale) || p->energy_mean_scale < 0.0f ||
			p->frames_context > LW_VAD_MAX_CONTEXT || !(p->proportion_threshold > 0.0f && p->proportion_threshold < 1.0f) || p->reserved != 0) {
		*err = LW_ERR_UNSUPPORTED;
		return nullptr;
	}
	int lds_limit = 0;
	if (lw_stage_device(device) ||
			!lw_hip_ok(hipDeviceGetAttribute(&lds_limit, hipDeviceAttributeMaxSharedMemoryPerBlock, device), "hipDeviceGetAttribute(LDS per workgroup)") ||
			lds_limit < (int)LW_VD_LDS) { // k_vad's workgroup does not fit this device
		*err = LW_ERR_DEVICE;
		return nullptr;
	}
	auto v = std::make_unique<lw_vad>();
	v->device = device, v->p = *p;
	if (!v->ring.create("hipEventCreate(vad rows)")) {
		*err = LW_ERR_DEVICE;
		lw_vad_destroy(v.release());
		return nullptr;
	}
	return v.release();
}

void lw_vad_destroy(lw_vad *v)
{
	if (!v)
		return;
	(void)hipSetDevice(v->device);
	(void)hipDeviceSynchronize();
	v->ring.destroy();
	for (auto &b : v->scratch)
		b.release();
	delete v;
}

int lw_vad_threshold(const lw_vad *v, double S, uint64_t T, float *thr)
{
	if (!v || !thr)
		return LW_ERR_NULL_ARG;
	*thr = lw_vad_threshold_value(v->p.energy_threshold, v->p.energy_mean_scale, S, T);
	return LW_OK;
}

int lw_vad_voiced(const lw_vad *v, uint64_t num, uint64_t den)
{
	if (!v)
		return -1;
	return lw_vad_voiced_value(num, den, v->p.proportion_threshold) ? 1 : 0;
}

uint32_t lw_vad_tile_frames(const lw_vad *v)
{
	return v ? v->tile : 0u;
}

int lw_vad_set_tile_frames(lw_vad *v, uint32_t tile)
{
	if (!v)
		return LW_ERR_NULL_ARG;
	if (!lw_vad_tile_ok(tile))
		return LW_ERR_UNSUPPORTED;
	v->tile = tile;
	return LW_OK;
}

int lw_vad_set_route(lw_vad *v, int route)
{
	if (!v)
		return LW_ERR_NULL_ARG;
	if (route != LW_VAD_ROUTE_AUTO && route != LW_VAD_ROUTE_FUSED && route != LW_VAD_ROUTE_SPLIT)
		return LW_ERR_UNSUPPORTED;
	v->route = route;
	return LW_OK;
}

int lw_vad_last_launches(const lw_vad *v)
{
	return v ? v->last_launches : -1;
}

int lw_vad_rows(lw_vad *v, uint32_t ch, uint32_t F, const void *d_src, uint8_t *d_mask, float *d_thr, size_t n_rows, size_t frame_capacity,
		const uint64_t *n_frames, const uint64_t *fill_to, void *hip_stream)
{
	if (!v || (!n_frames && n_rows))
		return LW_ERR_NULL_ARG;
	if (ch == 0 || ch > 255 || F == 0 || F > 65535u || v->p.line >= F || n_rows > UINT32_MAX)
		return LW_ERR_CAPACITY;
	if (!lw_rows_bytes_ok((uint64_t)ch * F, frame_capacity, n_rows))
		return LW_ERR_CAPACITY;
	// ---- plan: every row is checked before anything is queued, so a refused call has written nothing
	v->rows.clear();
	LwFillSpan span;
	uint64_t list = 0; // doubles of the chunk lists: every row's [ch][chunks]
	if (int rc = lw_stage_fill_rows(n_rows, n_frames, fill_to, frame_capacity, d_src, d_mask, span, [&](uint64_t n, uint64_t fill_end) {
			const uint64_t chunks = (n + LW_SUM_CHUNK - 1u) / LW_SUM_CHUNK;
			if (chunks > UINT32_MAX)
				return LW_ERR_CAPACITY;
			v->rows.push_back(LwVadRow{n, fill_end, list, (uint32_t)chunks, 0u});
			list += chunks * ch; // (n <= capacity and lw_rows_bytes_ok: no overflow)
			return LW_OK;
		}))
		return rc;
	const uint64_t tiles = (span.span + v->tile - 1u) / v->tile;
	if (tiles > LW_VD_MAX_TILES)
		return LW_ERR_CAPACITY; // what a grid of 256-lane workgroups can count in its first dimension
	if (v->route == LW_VAD_ROUTE_FUSED && span.span > LW_VAD_FUSED_MAX)
		return LW_ERR_UNSUPPORTED;
	LwVadArgs a{};
	a.src = (const float *)d_src, a.mask = d_mask, a.d_thr = d_thr, a.line_el = frame_capacity, a.ch = ch, a.F = F, a.line = v->p.line;
	a.tile = v->tile, a.tiles = (uint32_t)tiles, a.ctx = v->p.frames_context;
	a.energy_threshold = v->p.energy_threshold, a.energy_mean_scale = v->p.energy_mean_scale, a.proportion_threshold = v->p.proportion_threshold;
	const bool sums = v->p.energy_mean_scale != 0.0f && span.most != 0; // otherwise every threshold is energy_threshold
	const bool split = sums && (v->route == LW_VAD_ROUTE_SPLIT || (v->route == LW_VAD_ROUTE_AUTO && span.span > LW_VAD_FUSED_MAX));
	size_t part_bytes = 0, levels_bytes = 0, thr_bytes = 0;
	if (split) {
		uint64_t levels = 0;
		if (!lw_vad_sum_plan(span.most, a) || __builtin_mul_overflow((uint64_t)n_rows * ch, a.fold_scratch, &levels) || levels > (UINT64_MAX >> 4) ||
				list > (UINT64_MAX >> 4))
			return LW_ERR_CAPACITY;
		part_bytes = (size_t)list * sizeof(double), levels_bytes = (size_t)levels * sizeof(double), thr_bytes = n_rows * ch * sizeof(float);
	}
	HIP_TRY(hipSetDevice(v->device));
	hipStream_t st = (hipStream_t)hip_stream;
	if (n_rows == 0 || span.span == 0) { // no byte of the mask to write: every threshold is energy_threshold, by one workgroup
		int total = 0;
		if (d_thr && n_rows) {
			if (!lw_hip_ok(lw_launch_vad_fill(d_thr, (uint64_t)n_rows * ch, v->p.energy_threshold, st), "lw_launch_vad_fill"))
				return LW_ERR_DEVICE;
			total = 1;
		}
		v->last_launches = total;
		return LW_OK;
	}
	// ---- queue: the records, then the launches
	if (int rc = v->ring.acquire(n_rows))
		return rc;
	LwStageBuf &buf = v->scratch[v->ring.next];
	if (split) {
		if (int rc = buf.reserve(part_bytes + levels_bytes + thr_bytes))
			return rc;
		a.part = (double *)buf.p, a.scratch = (double *)((char *)buf.p + part_bytes), a.thr = (float *)((char *)buf.p + part_bytes + levels_bytes);
	}
	a.thr_out = !split;
	LwStageGuard staged = v->ring.guard(st);
	if (int rc = v->ring.upload(v->rows, st))
		return rc;
	a.rows = v->ring.dev();
	int total = 0;
	// (the launches of the next 65535 rows are queued behind these on the stream; the lists of all rows are apart)
	const int launches = lw_stage_launch(n_rows, "lw_launch_vad", [&](uint32_t row0, uint32_t n) {
		a.row0 = row0;
		if (split) {
			hipError_t e = lw_launch_vad_sum(a, n, st);
			if (e != hipSuccess)
				return e;
			total++;
			e = lw_launch_vad_fold(a, n, st);
			if (e != hipSuccess)
				return e;
			total++;
		}
		total++;
		return sums && !split ? lw_launch_vad(a, n, st) : lw_launch_vad_decide(a, n, st);
	});
	if (launches < 0)
		return LW_ERR_DEVICE;
	if (int rc = staged.commit())
		return rc;
	v->last_launches = total;
	return LW_OK;
}

} // extern "C"
