// SpecAugment masks (lw_specaug_*, lw_specaug_rows; include/lewton_amd.h "masking feature rows"): time and frequency masks over f32
// [row][ch][F][frame_capacity] rows, each a pure function of (seed, utterance id, group, kind, number) by the rule of lw_specaug.hpp
// -- a contract on bits.  Everything about a call is decided here on the host before anything is queued (the refusals, whether
// there is anything to write at all); k_specaug of lw_kernels_specaug.hip does the work in one launch per 65535 rows.  The call's
// per-row records (T, fill_end, id) are staged as lw_stage.hpp describes.  Nothing else in the library calls into this file.
#include "lw_stage.hpp"
#include "lw_specaug.hpp"

static_assert(LW_SA_MAX_MASKS == LW_SPECAUG_MAX_MASKS && LW_SA_MAX_WIDTH == LW_SPECAUG_MAX_WIDTH, "the kernel's limits are the header's");

struct lw_specaug {
	int device = 0;
	lw_specaug_params p{};
	LwSaRule rule{};
	uint32_t fill_bits = 0;
	uint32_t tile = LW_SA_TILE;
	LwStageRing<LwSaRow> ring;
	int last_launches = -1;
	std::vector<LwSaRow> rows;
};

extern "C" {

lw_specaug *lw_specaug_create(int device, const lw_specaug_params *p, int *err)
{
	int dummy;
	if (!err)
		err = &dummy;
	*err = LW_OK;
	if (!p) {
		*err = LW_ERR_NULL_ARG;
		return nullptr;
	}
	if (p->min_t > p->max_t || p->min_f > p->max_f || p->num_t > LW_SPECAUG_MAX_MASKS || p->num_f > LW_SPECAUG_MAX_MASKS || p->max_t > LW_SPECAUG_MAX_WIDTH ||
			p->max_f > LW_SPECAUG_MAX_WIDTH || p->ratio_num > p->ratio_den || p->ratio_den > 65535u || p->per_channel > 1u || p->reserved != 0) {
		*err = LW_ERR_UNSUPPORTED;
		return nullptr;
	}
	if (lw_stage_device(device)) {
		*err = LW_ERR_DEVICE;
		return nullptr;
	}
	auto sa = std::make_unique<lw_specaug>();
	sa->device = device, sa->p = *p;
	sa->rule = LwSaRule{p->seed, p->num_t, p->min_t, p->max_t, p->ratio_num, p->ratio_den, p->num_f, p->min_f, p->max_f};
	std::memcpy(&sa->fill_bits, &p->fill, 4); // fill's own bits: a NaN's payload, the sign of a zero
	if (!sa->ring.create("hipEventCreate(specaug rows)")) {
		*err = LW_ERR_DEVICE;
		lw_specaug_destroy(sa.release());
		return nullptr;
	}
	return sa.release();
}

void lw_specaug_destroy(lw_specaug *sa)
{
	if (!sa)
		return;
	(void)hipSetDevice(sa->device);
	(void)hipDeviceSynchronize();
	sa->ring.destroy();
	delete sa;
}

int lw_specaug_plan(const lw_specaug *sa, uint64_t id, uint32_t group, uint64_t T, uint32_t F, int64_t *spans)
{
	if (!sa || !spans)
		return LW_ERR_NULL_ARG;
	if (group > 65535u || F > 65535u || T > (uint64_t)INT64_MAX)
		return LW_ERR_CAPACITY;
	for (uint32_t i = 0; i < sa->rule.num_t + sa->rule.num_f; i++) {
		const bool time = i < sa->rule.num_t;
		uint64_t start, end;
		lw_sa_span(sa->rule, id, group, time ? LW_SA_TIME : LW_SA_FREQ, time ? i : i - sa->rule.num_t, time ? T : (uint64_t)F, start, end);
		spans[2 * i] = (int64_t)start, spans[2 * i + 1] = (int64_t)end;
	}
	return LW_OK;
}

uint32_t lw_specaug_tile_frames(const lw_specaug *sa)
{
	return sa ? sa->tile : 0u;
}

int lw_specaug_set_tile_frames(lw_specaug *sa, uint32_t tile)
{
	if (!sa)
		return LW_ERR_NULL_ARG;
	if (!lw_sa_tile_ok(tile))
		return LW_ERR_UNSUPPORTED;
	sa->tile = tile;
	return LW_OK;
}

int lw_specaug_last_launches(const lw_specaug *sa)
{
	return sa ? sa->last_launches : -1;
}

int lw_specaug_rows(lw_specaug *sa, uint32_t ch, uint32_t F, const void *d_src, void *d_dst, size_t n_rows, size_t frame_capacity, const uint64_t *n_frames,
		const uint64_t *fill_to, const uint64_t *ids, int64_t *d_spans, void *hip_stream)
{
	if (!sa || (!n_frames && n_rows))
		return LW_ERR_NULL_ARG;
	if (ch == 0 || ch > 255 || F == 0 || F > 65535u || n_rows > UINT32_MAX)
		return LW_ERR_CAPACITY;
	if (!lw_rows_bytes_ok((uint64_t)ch * F, frame_capacity, n_rows))
		return LW_ERR_CAPACITY;
	// ---- plan: every row is checked before anything is queued, so a refused call has written nothing
	sa->rows.clear();
	LwFillSpan span;
	bool fills = false; // some row has a fill span
	if (int rc = lw_stage_fill_rows(n_rows, n_frames, fill_to, frame_capacity, d_src, d_dst, span, [&](uint64_t n, uint64_t fill_end) {
			const uint64_t row = sa->rows.size();
			sa->rows.push_back(LwSaRow{n, fill_end, ids ? ids[row] : row, 0u});
			fills = fills || fill_end > n;
			return LW_OK;
		}))
		return rc;
	const uint32_t masks = sa->rule.num_t + sa->rule.num_f;
	const bool owes = d_spans && masks && n_rows;
	const bool in_place = d_src == d_dst;
	// what can be written: out of place every element below fill_end; in place the masked frames and the fill spans
	const bool writes = in_place ? fills || (masks && span.most) : span.span != 0;
	uint64_t tiles = (span.span + sa->tile - 1u) / sa->tile;
	if (owes && tiles == 0)
		tiles = 1; // tile 0 of line 0 stores a group's spans
	if (tiles * F > LW_SA_MAX_TILES)
		return LW_ERR_CAPACITY; // what a grid of 256-lane workgroups can count in its first dimension
	HIP_TRY(hipSetDevice(sa->device));
	hipStream_t st = (hipStream_t)hip_stream;
	if (!writes && !owes) {
		sa->last_launches = 0;
		return LW_OK;
	}
	LwSaArgs a{};
	a.src = (const uint32_t *)d_src, a.dst = (uint32_t *)d_dst, a.spans = owes ? d_spans : nullptr, a.line_el = frame_capacity, a.rule = sa->rule;
	a.ch = ch, a.F = F, a.tile = sa->tile, a.tiles = (uint32_t)tiles, a.per_channel = sa->p.per_channel, a.fill = sa->fill_bits;
	// ---- queue: the records, then the launches
	if (int rc = sa->ring.acquire(n_rows))
		return rc;
	LwStageGuard staged = sa->ring.guard(st);
	if (int rc = sa->ring.upload(sa->rows, st))
		return rc;
	a.rows = sa->ring.dev();
	const int launches = lw_stage_launch(n_rows, "lw_launch_specaug", [&](uint32_t row0, uint32_t n) {
		a.row0 = row0;
		return lw_launch_specaug(a, n, st);
	});
	if (launches < 0)
		return LW_ERR_DEVICE;
	if (int rc = staged.commit())
		return rc;
	sa->last_launches = launches;
	return LW_OK;
}

} // extern "C"
