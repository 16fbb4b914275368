// Speech segments from a frame mask (lw_segment_*, lw_segment_rows; include/lewton_amd.h "segments of a frame mask"): pyannote's
// Binarize on a uint8 mask [row][ch][frame_capacity] -- pad, fill short gaps, drop short runs -- into the spans of every row and
// channel, their count and the smoothed mask, all left on the device.  Everything about a call is decided here on the host before
// anything is queued; k_segment_count and k_segment (lw_kernels_segment.hip) do the work in two launches per 65535 rows.  The call's
// per-row records are staged as lw_stage.hpp describes, the tile counts go through scratch of the same rotation.  Nothing else in
// the library calls into this file.
#include "lw_stage.hpp"
#include "lw_segment.hpp"

static_assert(LW_SG_MAX_SPAN == LW_SEG_MAX_SPAN, "the kernels' limit is the header's");

struct lw_segment {
	int device = 0;
	lw_segment_params p{};
	uint32_t tile = LW_SG_TILE;
	LwStageRing<LwSegmentRow> ring;
	LwStageBuf scratch[LW_STAGE_SLOTS]; // the tile counts of the call that holds the slot
	int last_launches = -1;
	std::vector<LwSegmentRow> rows;
};

extern "C" {

lw_segment *lw_segment_create(int device, const lw_segment_params *p, int *err)
{
	int dummy;
	if (!err)
		err = &dummy;
	*err = LW_OK;
	if (!p) {
		*err = LW_ERR_NULL_ARG;
		return nullptr;
	}
	if (p->pad_onset > LW_SEG_MAX_SPAN || p->pad_offset > LW_SEG_MAX_SPAN || p->min_off > LW_SEG_MAX_SPAN || p->min_on > LW_SEG_MAX_SPAN || p->reserved != 0) {
		*err = LW_ERR_UNSUPPORTED;
		return nullptr;
	}
	int lds_limit = 0;
	if (lw_stage_device(device) ||
			!lw_hip_ok(hipDeviceGetAttribute(&lds_limit, hipDeviceAttributeMaxSharedMemoryPerBlock, device), "hipDeviceGetAttribute(LDS per workgroup)") ||
			lds_limit < (int)LW_SG_LDS) { // k_segment's workgroup does not fit this device
		*err = LW_ERR_DEVICE;
		return nullptr;
	}
	auto sg = std::make_unique<lw_segment>();
	sg->device = device, sg->p = *p;
	if (!sg->ring.create("hipEventCreate(segment rows)")) {
		*err = LW_ERR_DEVICE;
		lw_segment_destroy(sg.release());
		return nullptr;
	}
	return sg.release();
}

void lw_segment_destroy(lw_segment *sg)
{
	if (!sg)
		return;
	(void)hipSetDevice(sg->device);
	(void)hipDeviceSynchronize();
	sg->ring.destroy();
	for (auto &b : sg->scratch)
		b.release();
	delete sg;
}

uint32_t lw_segment_tile_frames(const lw_segment *sg)
{
	return sg ? sg->tile : 0u;
}

int lw_segment_set_tile_frames(lw_segment *sg, uint32_t tile)
{
	if (!sg)
		return LW_ERR_NULL_ARG;
	if (!lw_segment_tile_ok(tile))
		return LW_ERR_UNSUPPORTED;
	sg->tile = tile;
	return LW_OK;
}

int lw_segment_last_launches(const lw_segment *sg)
{
	return sg ? sg->last_launches : -1;
}

int lw_segment_rows(lw_segment *sg, uint32_t ch, const uint8_t *d_mask, uint64_t *d_spans, uint64_t *d_counts, uint8_t *d_smooth, size_t n_rows,
		size_t frame_capacity, size_t seg_capacity, const uint64_t *n_frames, const uint64_t *fill_to, void *hip_stream)
{
	if (!sg || (!n_frames && n_rows))
		return LW_ERR_NULL_ARG;
	if (ch == 0 || ch > 255 || n_rows > UINT32_MAX || (d_spans && seg_capacity == 0))
		return LW_ERR_CAPACITY;
	if (!lw_rows_bytes_ok(ch, frame_capacity, n_rows, 1) || (d_spans && !lw_rows_bytes_ok((uint64_t)ch * 2u, seg_capacity, n_rows, 8)))
		return LW_ERR_CAPACITY;
	// ---- plan: every row is checked before anything is queued, so a refused call has written nothing
	sg->rows.clear();
	uint64_t most = 0, span = 0; // the largest T; the largest frame a workgroup has something to do for
	for (size_t i = 0; i < n_rows; i++) {
		const uint64_t fill = fill_to ? fill_to[i] : 0;
		if (n_frames[i] > frame_capacity || fill > frame_capacity)
			return LW_ERR_CAPACITY;
		const uint64_t fill_end = std::max<uint64_t>(n_frames[i], fill);
		sg->rows.push_back(LwSegmentRow{n_frames[i], fill_end});
		most = std::max<uint64_t>(most, n_frames[i]);
		span = std::max(span, d_smooth ? fill_end : n_frames[i]);
	}
	if (most && !d_mask)
		return LW_ERR_NULL_ARG;
	const uint64_t tiles = (span + sg->tile - 1u) / sg->tile;
	uint64_t list = 0; // entries of the tile counts: [min(n_rows, 65535)][ch][tiles]
	if (tiles > LW_SG_MAX_TILES || __builtin_mul_overflow(std::min<uint64_t>(n_rows, LW_STAGE_ROWS) * ch, tiles, &list) || list > (UINT64_MAX >> 3))
		return LW_ERR_CAPACITY; // what a grid of 256-lane workgroups can count in its first dimension
	HIP_TRY(hipSetDevice(sg->device));
	hipStream_t st = (hipStream_t)hip_stream;
	if (n_rows == 0 || tiles == 0 || (!d_spans && !d_counts && !d_smooth)) { // nothing to write but the counts, which are all 0
		if (d_counts && n_rows)
			HIP_TRY(hipMemsetAsync(d_counts, 0, n_rows * ch * sizeof(uint64_t), st));
		sg->last_launches = 0;
		return LW_OK;
	}
	// ---- queue: the records, then the launches
	if (int rc = sg->ring.acquire(n_rows))
		return rc;
	LwStageBuf &buf = sg->scratch[sg->ring.next];
	if (int rc = buf.reserve((size_t)list * sizeof(uint32_t)))
		return rc;
	LwStageGuard staged = sg->ring.guard(st);
	if (int rc = sg->ring.upload(sg->rows, st))
		return rc;
	LwSegmentArgs a{};
	a.rows = sg->ring.dev(), a.mask = d_mask, a.tile_counts = (uint32_t *)buf.p, a.d_spans = d_spans, a.d_counts = d_counts, a.d_smooth = d_smooth;
	a.line_el = frame_capacity, a.seg_capacity = seg_capacity, a.ch = ch, a.tile = sg->tile, a.tiles = (uint32_t)tiles;
	a.pad_onset = sg->p.pad_onset, a.pad_offset = sg->p.pad_offset, a.min_off = sg->p.min_off, a.min_on = sg->p.min_on;
	int total = 0;
	// (the rows of one launch pair share the scratch list: the pair of the next 65535 rows is queued behind it on the stream)
	const int launches = lw_stage_launch(n_rows, "lw_launch_segment", [&](uint32_t row0, uint32_t n) {
		a.row0 = row0;
		if (most && (d_spans || d_counts)) {
			const hipError_t e = lw_launch_segment_count(a, n, st);
			if (e != hipSuccess)
				return e;
			total++;
		}
		total++;
		return lw_launch_segment(a, n, st);
	});
	if (launches < 0)
		return LW_ERR_DEVICE;
	if (int rc = staged.commit())
		return rc;
	sg->last_launches = total;
	return LW_OK;
}

} // extern "C"
