// Cepstra and deltas of feature rows (lw_cep_*, lw_cep_rows; include/lewton_amd.h "cepstra and deltas of feature rows"): a matrix
// across the feature lines of f32 [row][ch][n_in][capacity] rows (MFCC: a DCT of log-mel lines) and regression deltas along the
// frames, a contract on bits.  Everything about a call is decided here on the host before anything is queued (the refusals, the
// tile plan); k_cep (lw_kernels_cep.hip) does the work in one launch per 65535 rows.  The call's per-row records are staged as
// lw_stage.hpp describes.  Nothing else in the library calls into this file.
#include "lw_stage.hpp"
#include "lw_cep.hpp"

struct lw_cep {
	int device = 0;
	uint32_t n_in = 0, n_out = 0, order = 0, width = 0;
	bool identity = false;
	LwCepPlan plan{};
	uint32_t mt_stride = 0;
	std::vector<float> matrix; // [n_out][n_in], the caller's (empty for the identity)
	float *d_mt = nullptr;     // [n_in][mt_stride], transposed and padded with +0.0
	float w[LW_CP_MAX_WIDTH] = {};
	LwStageRing<LwCepRow> ring;
	int last_launches = -1;
	std::vector<LwCepRow> rows;
};

extern "C" {

lw_cep *lw_cep_create(int device, uint32_t n_in, uint32_t n_out, const float *matrix, uint32_t order, uint32_t width, int *err)
{
	int dummy;
	if (!err)
		err = &dummy;
	*err = LW_OK;
	if (n_in < 1 || n_in > LW_CEP_MAX_IN || n_out < 1 || n_out > LW_CEP_MAX_OUT || order > 2 || (order == 0 ? width != 0 : (width < 1 || width > LW_CEP_MAX_WIDTH))) {
		*err = LW_ERR_UNSUPPORTED;
		return nullptr;
	}
	if (!matrix && n_out != n_in) {
		*err = LW_ERR_NULL_ARG;
		return nullptr;
	}
	const LwCepPlan plan = lw_cep_plan(n_out, order, width);
	int lds_limit = 0;
	if (lw_stage_device(device) ||
			!lw_hip_ok(hipDeviceGetAttribute(&lds_limit, hipDeviceAttributeMaxSharedMemoryPerBlock, device), "hipDeviceGetAttribute(LDS per workgroup)") ||
			(size_t)lds_limit < plan.lds) { // k_cep's workgroup does not fit this device
		*err = LW_ERR_DEVICE;
		return nullptr;
	}
	auto cp = std::make_unique<lw_cep>();
	cp->device = device, cp->n_in = n_in, cp->n_out = n_out, cp->order = order, cp->width = width, cp->identity = !matrix, cp->plan = plan;
	cp->mt_stride = (n_out + LW_CP_GROUP - 1u) & ~(LW_CP_GROUP - 1u);
	lw_cep_weights(width, cp->w);
	bool ok = cp->ring.create("hipEventCreate(cep rows)");
	if (ok && matrix) {
		cp->matrix.assign(matrix, matrix + (size_t)n_out * n_in);
		std::vector<float> mt((size_t)n_in * cp->mt_stride, 0.0f);
		for (uint32_t q = 0; q < n_out; q++)
			for (uint32_t f = 0; f < n_in; f++)
				mt[(size_t)f * cp->mt_stride + q] = matrix[(size_t)q * n_in + f];
		ok = lw_hip_ok(hipMalloc((void **)&cp->d_mt, mt.size() * sizeof(float)), "hipMalloc(cep matrix)") &&
			lw_hip_ok(hipMemcpy(cp->d_mt, mt.data(), mt.size() * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy(cep matrix)");
	}
	if (!ok) {
		*err = LW_ERR_DEVICE;
		lw_cep_destroy(cp.release());
		return nullptr;
	}
	return cp.release();
}

void lw_cep_destroy(lw_cep *cp)
{
	if (!cp)
		return;
	(void)hipSetDevice(cp->device);
	(void)hipDeviceSynchronize();
	cp->ring.destroy();
	if (cp->d_mt)
		(void)hipFree(cp->d_mt);
	delete cp;
}

uint32_t lw_cep_features(const lw_cep *cp)
{
	return cp ? cp->n_out * (1u + cp->order) : 0u;
}

size_t lw_cep_matrix(const lw_cep *cp, float *dst)
{
	if (!cp)
		return 0;
	if (dst && !cp->matrix.empty())
		std::memcpy(dst, cp->matrix.data(), cp->matrix.size() * sizeof(float));
	return cp->matrix.size();
}

uint32_t lw_cep_delta_weights(const lw_cep *cp, float *dst)
{
	if (!cp)
		return 0;
	if (dst)
		std::memcpy(dst, cp->w, cp->width * sizeof(float));
	return cp->width;
}

uint32_t lw_cep_tile_frames(const lw_cep *cp)
{
	return cp ? cp->plan.tile : 0u;
}

int lw_cep_last_launches(const lw_cep *cp)
{
	return cp ? cp->last_launches : -1;
}

int lw_cep_rows(lw_cep *cp, uint32_t ch, const void *d_src, void *d_dst, size_t n_rows, size_t frame_capacity, const uint64_t *n_frames,
		const uint64_t *fill_to, void *hip_stream)
{
	if (!cp || (!n_frames && n_rows))
		return LW_ERR_NULL_ARG;
	if (ch == 0 || ch > 255 || n_rows > UINT32_MAX)
		return LW_ERR_CAPACITY;
	const uint64_t lines = (uint64_t)ch * std::max(cp->n_in, cp->n_out * (1u + cp->order)); // the larger of the two buffers
	if (!lw_rows_bytes_ok(lines, frame_capacity, n_rows)) // each must be addressable in 64 bits of BYTES
		return LW_ERR_CAPACITY;
	// ---- plan: every row is checked before anything is queued, so a refused call has written nothing
	cp->rows.clear();
	LwFillSpan m;
	if (int rc = lw_stage_fill_rows(n_rows, n_frames, fill_to, frame_capacity, d_src, d_dst, m, [&](uint64_t n, uint64_t fill_end) {
		    cp->rows.push_back(LwCepRow{n, fill_end});
		    return LW_OK;
	    }))
		return rc;
	const uint64_t tiles = (m.span + cp->plan.tile - 1u) / cp->plan.tile;
	if (tiles > LW_CP_MAX_TILES) // what a grid of 256-lane workgroups can count in its first dimension
		return LW_ERR_CAPACITY;
	if (n_rows == 0 || m.span == 0) {
		cp->last_launches = 0;
		return LW_OK;
	}
	// ---- queue: the records, then the launches
	HIP_TRY(hipSetDevice(cp->device));
	hipStream_t st = (hipStream_t)hip_stream;
	if (int rc = cp->ring.acquire(n_rows))
		return rc;
	LwStageGuard staged = cp->ring.guard(st);
	if (int rc = cp->ring.upload(cp->rows, st))
		return rc;
	LwCepArgs a{};
	a.rows = cp->ring.dev(), a.line_el = frame_capacity;
	a.ch = ch, a.n_in = cp->n_in, a.n_out = cp->n_out, a.order = cp->order, a.width = cp->width;
	a.identity = cp->identity, a.mt_stride = cp->mt_stride, a.plan = cp->plan;
	std::memcpy(a.w, cp->w, sizeof(a.w));
	const int launches = lw_stage_launch(n_rows, "lw_launch_cep", [&](uint32_t row0, uint32_t n) {
		a.row0 = row0;
		return lw_launch_cep(a, cp->d_mt, (const float *)d_src, (float *)d_dst, (uint32_t)tiles, n, st);
	});
	if (launches < 0)
		return LW_ERR_DEVICE;
	if (int rc = staged.commit())
		return rc;
	cp->last_launches = launches;
	return LW_OK;
}

} // extern "C"
