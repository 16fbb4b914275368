// Frame-major model input (lw_pack_*, lw_pack_rows; include/lewton_amd.h "frame-major model input"): f32
// [row][ch][F][frame_capacity] feature rows into [row][ch][out_capacity][W * F] frames of f32, bf16 or f16 -- transpose, context
// splice, stride, shift and scale, one rounding, padding and the mask -- a contract on bits.  Everything about a call is decided
// here on the host before anything is queued (the refusals, the tile plan, whether the 16-byte stores apply); k_pack
// (lw_kernels_pack.hip) does the work in one launch per 65535 rows.  The call's per-row records are staged as lw_stage.hpp
// describes.  Nothing else in the library calls into this file.
#include "lw_stage.hpp"
#include "lw_pack.hpp"

#include <cmath>

struct lw_pack {
	int device = 0;
	lw_pack_params p{};
	uint32_t W = 0, D = 0, esize = 4, pad_bits = 0;
	LwPackPlan plan{};
	float *d_shift = nullptr, *d_scale = nullptr; // D floats each, or NULL
	LwStageRing<LwPackRow> ring;
	int last_launches = -1;
	std::vector<LwPackRow> rows;
};

static uint32_t bits_of(float v)
{
	uint32_t u;
	std::memcpy(&u, &v, 4);
	return u;
}

extern "C" {

lw_pack *lw_pack_create(int device, const lw_pack_params *p, const float *shift, const float *scale, int *err)
{
	int dummy;
	if (!err)
		err = &dummy;
	*err = LW_OK;
	if (!p) {
		*err = LW_ERR_NULL_ARG;
		return nullptr;
	}
	if (p->F < 1 || p->F > 65535u || p->left > LW_PACK_MAX_CONTEXT || p->right > LW_PACK_MAX_CONTEXT || p->stride < 1 || p->stride > LW_PACK_MAX_STRIDE ||
			(p->edge != LW_PACK_EDGE_REPLICATE && p->edge != LW_PACK_EDGE_VALID) || p->dtype < LW_PACK_F32 || p->dtype > LW_PACK_F16 ||
			std::isnan(p->pad) || p->reserved != 0) {
		*err = LW_ERR_UNSUPPORTED;
		return nullptr;
	}
	const uint32_t W = p->left + p->right + 1u;
	const LwPackPlan plan = lw_pack_plan(p->F, W, p->stride);
	int lds_limit = 0;
	if (lw_stage_device(device) ||
			!lw_hip_ok(hipDeviceGetAttribute(&lds_limit, hipDeviceAttributeMaxSharedMemoryPerBlock, device), "hipDeviceGetAttribute(LDS per workgroup)") ||
			(size_t)lds_limit < plan.lds) { // k_pack's workgroup does not fit this device
		*err = LW_ERR_DEVICE;
		return nullptr;
	}
	auto pk = std::make_unique<lw_pack>();
	pk->device = device, pk->p = *p, pk->W = W, pk->D = W * p->F, pk->plan = plan;
	pk->esize = p->dtype == LW_PACK_F32 ? 4u : 2u;
	pk->pad_bits = lw_pack_cvt(p->dtype, bits_of(p->pad));
	bool ok = pk->ring.create("hipEventCreate(pack rows)");
	const size_t bytes = (size_t)pk->D * sizeof(float);
	if (ok && shift)
		ok = lw_hip_ok(hipMalloc((void **)&pk->d_shift, bytes), "hipMalloc(pack shift)") &&
			lw_hip_ok(hipMemcpy(pk->d_shift, shift, bytes, hipMemcpyHostToDevice), "hipMemcpy(pack shift)");
	if (ok && scale)
		ok = lw_hip_ok(hipMalloc((void **)&pk->d_scale, bytes), "hipMalloc(pack scale)") &&
			lw_hip_ok(hipMemcpy(pk->d_scale, scale, bytes, hipMemcpyHostToDevice), "hipMemcpy(pack scale)");
	if (!ok) {
		*err = LW_ERR_DEVICE;
		lw_pack_destroy(pk.release());
		return nullptr;
	}
	return pk.release();
}

void lw_pack_destroy(lw_pack *pk)
{
	if (!pk)
		return;
	(void)hipSetDevice(pk->device);
	(void)hipDeviceSynchronize();
	pk->ring.destroy();
	if (pk->d_shift)
		(void)hipFree(pk->d_shift);
	if (pk->d_scale)
		(void)hipFree(pk->d_scale);
	delete pk;
}

uint32_t lw_pack_width(const lw_pack *pk)
{
	return pk ? pk->D : 0u;
}

uint32_t lw_pack_tile_frames(const lw_pack *pk)
{
	return pk ? pk->plan.tile : 0u;
}

uint64_t lw_pack_frames(const lw_pack *pk, uint64_t T)
{
	return pk ? lw_pack_out_frames(pk->p.edge, pk->W, pk->p.stride, T) : 0u;
}

uint32_t lw_pack_convert(const lw_pack *pk, float v)
{
	return pk ? lw_pack_cvt(pk->p.dtype, bits_of(v)) : 0u;
}

int lw_pack_last_launches(const lw_pack *pk)
{
	return pk ? pk->last_launches : -1;
}

int lw_pack_rows(lw_pack *pk, uint32_t ch, const void *d_src, void *d_dst, size_t n_rows, size_t frame_capacity, size_t out_capacity,
		const uint64_t *n_frames, const uint64_t *fill_to, uint8_t *d_mask, void *hip_stream)
{
	if (!pk || (!n_frames && n_rows))
		return LW_ERR_NULL_ARG;
	if (ch == 0 || ch > 255 || n_rows > UINT32_MAX)
		return LW_ERR_CAPACITY;
	if (!lw_rows_bytes_ok((uint64_t)ch * pk->p.F, frame_capacity, n_rows) || !lw_rows_bytes_ok((uint64_t)ch * pk->D, out_capacity, n_rows, pk->esize))
		return LW_ERR_CAPACITY; // each must be addressable in 64 bits of BYTES (the mask is smaller than either)
	// ---- plan: every row is checked before anything is queued, so a refused call has written nothing.  (Not one of
	// lw_stage.hpp's two loops: a row is held against two capacities, the second through a count derived from the first.)
	pk->rows.clear();
	uint64_t most = 0, span = 0; // the largest n of a row that is read, the largest fill_end
	for (size_t i = 0; i < n_rows; i++) {
		const uint64_t fill = fill_to ? fill_to[i] : 0;
		if (n_frames[i] > frame_capacity)
			return LW_ERR_CAPACITY;
		const uint64_t n_out = lw_pack_out_frames(pk->p.edge, pk->W, pk->p.stride, n_frames[i]);
		if (n_out > out_capacity || fill > out_capacity)
			return LW_ERR_CAPACITY;
		const uint64_t fill_end = std::max(n_out, fill);
		pk->rows.push_back(LwPackRow{n_frames[i], n_out, fill_end});
		if (n_out)
			most = std::max(most, n_frames[i]);
		span = std::max(span, fill_end);
	}
	if ((most && !d_src) || (span && !d_dst))
		return LW_ERR_NULL_ARG;
	const uint64_t tiles = (span + pk->plan.tile - 1u) / pk->plan.tile;
	if (tiles > LW_PK_MAX_TILES) // what a grid of 256-lane workgroups can count in its first dimension
		return LW_ERR_CAPACITY;
	if (n_rows == 0 || span == 0) {
		pk->last_launches = 0;
		return LW_OK;
	}
	// ---- queue: the records, then the launches
	HIP_TRY(hipSetDevice(pk->device));
	hipStream_t st = (hipStream_t)hip_stream;
	if (int rc = pk->ring.acquire(n_rows))
		return rc;
	LwStageGuard staged = pk->ring.guard(st);
	if (int rc = pk->ring.upload(pk->rows, st))
		return rc;
	LwPackArgs a{};
	a.rows = pk->ring.dev(), a.shift = pk->d_shift, a.scale = pk->d_scale, a.line_el = frame_capacity, a.out_cap = out_capacity;
	a.ch = ch, a.F = pk->p.F, a.left = pk->p.left, a.stride = pk->p.stride, a.W = pk->W, a.D = pk->D;
	a.edge = pk->p.edge, a.dtype = pk->p.dtype, a.pad_bits = pk->pad_bits, a.plan = pk->plan;
	a.vec = pk->p.F % (16u / pk->esize) == 0 && ((uintptr_t)d_dst & 15u) == 0; // an optimisation where addresses allow, never a precondition
	const int launches = lw_stage_launch(n_rows, "lw_launch_pack", [&](uint32_t row0, uint32_t n) {
		a.row0 = row0;
		return lw_launch_pack(a, (const float *)d_src, d_dst, d_mask, (uint32_t)tiles, n, st);
	});
	if (launches < 0)
		return LW_ERR_DEVICE;
	if (int rc = staged.commit())
		return rc;
	pk->last_launches = launches;
	return LW_OK;
}

} // extern "C"
