// Frame selection (lw_select_*, lw_select_rows; include/lewton_amd.h "frame decisions and frame selection"): Kaldi's
// select-voiced-frames for any mask over f32 [row][ch][F][frame_capacity] rows -- the kept frames of every line moved to the
// line's front by bit copies, the rest of the line zeroed, the counts left on the device.  Everything about a call is decided here
// on the host before anything is queued; k_select_count and k_select (lw_kernels_select.hip) do the work in two launches per 65535
// rows.  The call's per-row records are staged as lw_stage.hpp describes, the tile counts go through scratch of the same
// rotation.  Nothing else in the library calls into this file.
#include "lw_stage.hpp"
#include "lw_select.hpp"

struct lw_select {
	int device = 0;
	uint32_t tile = LW_SE_TILE;
	LwStageRing<LwSelectRow> ring;
	LwStageBuf scratch[LW_STAGE_SLOTS]; // the tile counts of the call that holds the slot
	int last_launches = -1;
	std::vector<LwSelectRow> rows;
};

extern "C" {

lw_select *lw_select_create(int device, int *err)
{
	int dummy;
	if (!err)
		err = &dummy;
	*err = LW_OK;
	int lds_limit = 0;
	if (lw_stage_device(device) ||
			!lw_hip_ok(hipDeviceGetAttribute(&lds_limit, hipDeviceAttributeMaxSharedMemoryPerBlock, device), "hipDeviceGetAttribute(LDS per workgroup)") ||
			lds_limit < (int)LW_SE_LDS) { // k_select's workgroup does not fit this device
		*err = LW_ERR_DEVICE;
		return nullptr;
	}
	auto se = std::make_unique<lw_select>();
	se->device = device;
	if (!se->ring.create("hipEventCreate(select rows)")) {
		*err = LW_ERR_DEVICE;
		lw_select_destroy(se.release());
		return nullptr;
	}
	return se.release();
}

void lw_select_destroy(lw_select *se)
{
	if (!se)
		return;
	(void)hipSetDevice(se->device);
	(void)hipDeviceSynchronize();
	se->ring.destroy();
	for (auto &b : se->scratch)
		b.release();
	delete se;
}

uint32_t lw_select_tile_frames(const lw_select *se)
{
	return se ? se->tile : 0u;
}

int lw_select_set_tile_frames(lw_select *se, uint32_t tile)
{
	if (!se)
		return LW_ERR_NULL_ARG;
	if (!lw_select_tile_ok(tile))
		return LW_ERR_UNSUPPORTED;
	se->tile = tile;
	return LW_OK;
}

int lw_select_last_launches(const lw_select *se)
{
	return se ? se->last_launches : -1;
}

int lw_select_rows(lw_select *se, uint32_t ch, uint32_t F, const void *d_src, const uint8_t *d_mask, void *d_dst, uint64_t *d_counts, size_t n_rows,
		size_t frame_capacity, const uint64_t *n_frames, const uint64_t *fill_to, void *hip_stream)
{
	if (!se || (!n_frames && n_rows))
		return LW_ERR_NULL_ARG;
	if (ch == 0 || ch > 255 || F == 0 || F > 65535u || n_rows > UINT32_MAX)
		return LW_ERR_CAPACITY;
	if (!lw_rows_bytes_ok((uint64_t)ch * F, frame_capacity, n_rows))
		return LW_ERR_CAPACITY;
	// ---- plan: every row is checked before anything is queued, so a refused call has written nothing
	se->rows.clear();
	LwFillSpan span;
	if (int rc = lw_stage_fill_rows(n_rows, n_frames, fill_to, frame_capacity, d_src, d_dst, span, [&](uint64_t n, uint64_t fill_end) {
			se->rows.push_back(LwSelectRow{n, fill_end});
			return LW_OK;
		}))
		return rc;
	if (span.most && !d_mask)
		return LW_ERR_NULL_ARG;
	const uint32_t groups = (F + LW_SE_LINES - 1u) / LW_SE_LINES;
	const uint64_t tiles = (span.span + se->tile - 1u) / se->tile;
	uint64_t list = 0; // entries of the tile counts: [min(n_rows, 65535)][ch][tiles]
	if (tiles * groups > LW_SE_MAX_TILES || __builtin_mul_overflow(std::min<uint64_t>(n_rows, LW_STAGE_ROWS) * ch, tiles, &list) || list > (UINT64_MAX >> 3))
		return LW_ERR_CAPACITY; // what a grid of 256-lane workgroups can count in its first dimension
	HIP_TRY(hipSetDevice(se->device));
	hipStream_t st = (hipStream_t)hip_stream;
	if (n_rows == 0 || span.span == 0) { // nothing to write but the counts, which are all 0
		if (d_counts && n_rows)
			HIP_TRY(hipMemsetAsync(d_counts, 0, n_rows * ch * sizeof(uint64_t), st));
		se->last_launches = 0;
		return LW_OK;
	}
	// ---- queue: the records, then the launches
	if (int rc = se->ring.acquire(n_rows))
		return rc;
	LwStageBuf &buf = se->scratch[se->ring.next];
	if (int rc = buf.reserve((size_t)list * sizeof(uint32_t)))
		return rc;
	LwStageGuard staged = se->ring.guard(st);
	if (int rc = se->ring.upload(se->rows, st))
		return rc;
	LwSelectArgs a{};
	a.rows = se->ring.dev(), a.tile_counts = (uint32_t *)buf.p, a.d_counts = d_counts, a.line_el = frame_capacity, a.ch = ch, a.F = F;
	a.tile = se->tile, a.tiles = (uint32_t)tiles, a.groups = groups;
	int total = 0;
	// (the rows of one launch pair share the scratch list: the pair of the next 65535 rows is queued behind it on the stream)
	const int launches = lw_stage_launch(n_rows, "lw_launch_select", [&](uint32_t row0, uint32_t n) {
		a.row0 = row0;
		if (span.most) {
			const hipError_t e = lw_launch_select_count(a, d_mask, n, st);
			if (e != hipSuccess)
				return e;
			total++;
		}
		total++;
		return lw_launch_select(a, (const uint32_t *)d_src, d_mask, (uint32_t *)d_dst, n, st);
	});
	if (launches < 0)
		return LW_ERR_DEVICE;
	if (int rc = staged.commit())
		return rc;
	se->last_launches = total;
	return LW_OK;
}

} // extern "C"
