// Segment rows (lw_cut_*, lw_cut_rows; include/lewton_amd.h "cutting rows into segment rows"): one output row [ch][F][out_capacity]
// per job (row, start, end) over rows [row][ch][F][capacity] of 2- or 4-byte elements -- the waveform or the features of every
// speech segment as a row of its own, by bit copies, the rest of the line zeroed.  Everything about a call is decided here on the
// host before anything is queued; k_cut (lw_kernels_cut.hip) does the work in one launch per 65535 jobs.  The call's per-job
// records are staged as lw_stage.hpp describes.  Nothing else in the library calls into this file.
#include "lw_stage.hpp"
#include "lw_cut.hpp"

struct lw_cut {
	int device = 0;
	LwStageRing<LwCutJob> ring;
	int last_launches = -1;
	std::vector<LwCutJob> jobs;
};

extern "C" {

lw_cut *lw_cut_create(int device, int *err)
{
	int dummy;
	if (!err)
		err = &dummy;
	*err = LW_OK;
	if (lw_stage_device(device)) {
		*err = LW_ERR_DEVICE;
		return nullptr;
	}
	auto c = std::make_unique<lw_cut>();
	c->device = device;
	if (!c->ring.create("hipEventCreate(cut jobs)")) {
		*err = LW_ERR_DEVICE;
		lw_cut_destroy(c.release());
		return nullptr;
	}
	return c.release();
}

void lw_cut_destroy(lw_cut *c)
{
	if (!c)
		return;
	(void)hipSetDevice(c->device);
	(void)hipDeviceSynchronize();
	c->ring.destroy();
	delete c;
}

int lw_cut_last_launches(const lw_cut *c)
{
	return c ? c->last_launches : -1;
}

int lw_cut_rows(lw_cut *c, uint32_t ch, uint32_t F, uint32_t elem_bytes, const void *d_src, size_t n_rows, size_t capacity, const uint64_t *n_frames,
		const uint64_t *jobs, size_t n_out, void *d_dst, size_t out_capacity, const uint64_t *fill_to, void *hip_stream)
{
	if (!c || (!n_frames && n_rows) || (!jobs && n_out))
		return LW_ERR_NULL_ARG;
	if (elem_bytes != 2u && elem_bytes != 4u)
		return LW_ERR_UNSUPPORTED;
	if (ch == 0 || ch > 255 || F == 0 || F > 65535u || n_rows > UINT32_MAX || n_out > UINT32_MAX)
		return LW_ERR_CAPACITY;
	if (!lw_rows_bytes_ok((uint64_t)ch * F, capacity, n_rows, elem_bytes) || !lw_rows_bytes_ok((uint64_t)ch * F, out_capacity, n_out, elem_bytes))
		return LW_ERR_CAPACITY;
	// ---- plan: every job is checked before anything is queued, so a refused call has written nothing
	c->jobs.clear();
	uint64_t most = 0, span = 0; // the largest len, the largest fill_end
	for (size_t i = 0; i < n_out; i++) {
		const uint64_t row = jobs[3 * i], start = jobs[3 * i + 1], end = jobs[3 * i + 2], fill = fill_to ? fill_to[i] : 0;
		if (row >= n_rows || start > end || end > n_frames[row] || n_frames[row] > capacity || end - start > out_capacity || fill > out_capacity)
			return LW_ERR_CAPACITY;
		const uint64_t len = end - start, fill_end = std::max(len, fill);
		c->jobs.push_back(LwCutJob{row * ch * F * capacity + start, len, fill_end});
		most = std::max(most, len), span = std::max(span, fill_end);
	}
	if ((most && !d_src) || (span && !d_dst))
		return LW_ERR_NULL_ARG;
	const uint64_t tiles = (span * elem_bytes + LW_CT_TILE - 1u) / LW_CT_TILE;
	if (tiles * F > LW_CT_MAX_TILES)
		return LW_ERR_CAPACITY; // what a grid of 256-lane workgroups can count in its first dimension
	HIP_TRY(hipSetDevice(c->device));
	hipStream_t st = (hipStream_t)hip_stream;
	if (n_out == 0 || span == 0) { // nothing to write
		c->last_launches = 0;
		return LW_OK;
	}
	// ---- queue: the records, then the launches
	if (int rc = c->ring.acquire(n_out))
		return rc;
	LwStageGuard staged = c->ring.guard(st);
	if (int rc = c->ring.upload(c->jobs, st))
		return rc;
	LwCutArgs a{};
	a.jobs = c->ring.dev(), a.src = (const uint8_t *)d_src, a.dst = (uint8_t *)d_dst, a.src_line = capacity, a.dst_line = out_capacity;
	a.ch = ch, a.F = F, a.elem = elem_bytes, a.tiles = (uint32_t)tiles;
	const int launches = lw_stage_launch(n_out, "lw_launch_cut", [&](uint32_t job0, uint32_t n) {
		a.job0 = job0;
		return lw_launch_cut(a, n, st);
	});
	if (launches < 0)
		return LW_ERR_DEVICE;
	if (int rc = staged.commit())
		return rc;
	c->last_launches = launches;
	return LW_OK;
}

} // extern "C"
