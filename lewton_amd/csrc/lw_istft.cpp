// Inverse spectral frames of rows (lw_istft_*, lw_istft_rows; include/lewton_amd.h "inverse spectral frames of rows"): complex
// spectral frames [row][ch][2 B][frame] in device memory (lw_spec_rows' LW_SPEC_OUT_COMPLEX layout) turned back into rows of f32
// PCM by a windowed inverse DFT, an overlap-add and a division by the window envelope whose table and fold orders are a contract
// on bits.  The table is evaluated here in double and rounded once; everything about a call is decided here on the host before
// anything is queued (the refusals, the lengths, the launch geometry); k_istft (lw_kernels_istft.hip) does the folds.  The
// call's per-row records are staged as lw_stage.hpp describes.  Nothing else in the library calls into this file.
#include "lw_stage.hpp"
#include "lw_istft.hpp"
#include "lw_window.hpp"

#include <cmath>

struct lw_istft {
	int device = 0;
	uint32_t n_fft = 0, win_length = 0, hop = 0;
	bool center = false;
	LwIstftPlan plan{};
	uint32_t m = 0;            // the tile plan's, or what lw_istft_set_tile_frames put in its place
	std::vector<float> table;  // [2 B][win_length], the public order
	std::vector<double> w2;    // [win_length]
	float *d_table = nullptr;  // the kernel's order (lw_istft.hpp)
	double *d_w2 = nullptr;
	LwStageRing<LwIstftRow> ring;
	int route = LW_IS_ROUTE_MFMA, last_route = -1;
	std::vector<LwIstftRow> rows;
	std::vector<uint64_t> taken;
};

static uint64_t lw_is_natural(const lw_istft *is, uint64_t T)
{
	if (T == 0)
		return 0;
	const uint64_t P = (uint64_t)is->n_fft + (T - 1) * is->hop, pad2 = is->center ? 2u * (uint64_t)(is->n_fft / 2u) : 0u;
	return P > pad2 ? P - pad2 : 0; // (odd n_fft and one frame: P - 2 pad = 1)
}

extern "C" {

lw_istft *lw_istft_create(int device, const lw_istft_params *prm, int *err)
{
	int dummy;
	if (!err)
		err = &dummy;
	*err = LW_OK;
	if (!prm) {
		*err = LW_ERR_NULL_ARG;
		return nullptr;
	}
	const uint32_t n_fft = prm->n_fft, win_length = prm->win_length, hop = prm->hop;
	const int window = prm->window;
	const bool symmetric = lw_sp_window_symmetric(window);
	if (n_fft < 2 || n_fft > LW_SPEC_MAX_FFT || win_length < 1 || win_length > n_fft || hop < 1 || hop > 65535 ||
			(window != LW_SPEC_HANN && window != LW_SPEC_RECT && !symmetric) || (symmetric && win_length < 2) || (prm->center != 0 && prm->center != 1) ||
			prm->reserved != 0 || hop > win_length /* gaps no frame covers */ ||
			(win_length + hop - 1u) / hop > LW_ISTFT_MAX_OVERLAP /* a tile must own at least half of what it computes */) {
		*err = LW_ERR_UNSUPPORTED;
		return nullptr;
	}
	int lds_limit = 0;
	if (lw_stage_device(device) ||
			!lw_hip_ok(hipDeviceGetAttribute(&lds_limit, hipDeviceAttributeMaxSharedMemoryPerBlock, device), "hipDeviceGetAttribute(LDS per workgroup)") ||
			(size_t)lds_limit < LW_IS_LDS_FLOATS * sizeof(float)) { // k_istft's workgroup does not fit this device
		*err = LW_ERR_DEVICE;
		return nullptr;
	}
	auto is = std::make_unique<lw_istft>();
	is->device = device;
	is->n_fft = n_fft, is->win_length = win_length, is->hop = hop, is->center = prm->center != 0;
	is->plan = lw_istft_plan(n_fft, win_length, hop);
	is->m = is->plan.m;
	const LwIstftPlan p = is->plan;
	const uint32_t B = p.bins;
	// ---- the tables, in double, each entry rounded once
	is->table.resize((size_t)p.lines * win_length);
	is->w2.resize(win_length);
	std::vector<float> dev((size_t)p.passes * p.l_pad * LW_IS_COLS, 0.0f);
	for (uint32_t k = 0; k < win_length; k++) {
		const double w = lw_sp_window(window, k, win_length);
		is->w2[k] = w * w;
		for (uint32_t j = 0; j < B; j++) {
			const bool real_only = j == 0 || (n_fft % 2u == 0 && j == n_fft / 2u); // irfft ignores the imaginary part of these bins
			const double c = real_only ? 1.0 : 2.0;
			const double ang = 2.0 * M_PI * (double)(((uint64_t)k + p.offset) * j % n_fft) / (double)n_fft;
			const float gc = (float)(w * c * std::cos(ang) / (double)n_fft);
			const float gs = real_only ? 0.0f : (float)(-(w * c * std::sin(ang)) / (double)n_fft);
			is->table[(size_t)j * win_length + k] = gc, is->table[((size_t)B + j) * win_length + k] = gs;
			dev[lw_istft_table_at(p, j, k)] = gc, dev[lw_istft_table_at(p, B + j, k)] = gs;
		}
	}
	const bool ok = lw_hip_ok(hipMalloc((void **)&is->d_table, dev.size() * sizeof(float)), "hipMalloc(istft table)") &&
		lw_hip_ok(hipMemcpy(is->d_table, dev.data(), dev.size() * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy(istft table)") &&
		lw_hip_ok(hipMalloc((void **)&is->d_w2, is->w2.size() * sizeof(double)), "hipMalloc(istft envelope)") &&
		lw_hip_ok(hipMemcpy(is->d_w2, is->w2.data(), is->w2.size() * sizeof(double), hipMemcpyHostToDevice), "hipMemcpy(istft envelope)");
	if (!ok || !is->ring.create("hipEventCreate(istft rows)")) {
		*err = LW_ERR_DEVICE;
		lw_istft_destroy(is.release());
		return nullptr;
	}
	return is.release();
}

void lw_istft_destroy(lw_istft *is)
{
	if (!is)
		return;
	(void)hipSetDevice(is->device);
	(void)hipDeviceSynchronize();
	is->ring.destroy();
	if (is->d_table)
		(void)hipFree(is->d_table);
	if (is->d_w2)
		(void)hipFree(is->d_w2);
	delete is;
}

uint32_t lw_istft_bins(const lw_istft *is)
{
	return is ? is->plan.bins : 0;
}

uint64_t lw_istft_out_len(const lw_istft *is, uint64_t frames)
{
	return is ? lw_is_natural(is, frames) : 0;
}

size_t lw_istft_basis(const lw_istft *is, float *dst)
{
	if (!is)
		return 0;
	if (dst)
		std::memcpy(dst, is->table.data(), is->table.size() * sizeof(float));
	return is->table.size();
}

size_t lw_istft_window2(const lw_istft *is, double *dst)
{
	if (!is)
		return 0;
	if (dst)
		std::memcpy(dst, is->w2.data(), is->w2.size() * sizeof(double));
	return is->w2.size();
}

uint32_t lw_istft_tile_frames(const lw_istft *is)
{
	return is ? is->m : 0;
}

int lw_istft_set_tile_frames(lw_istft *is, uint32_t m)
{
	if (!is)
		return LW_ERR_NULL_ARG;
	if (m < 1 || m > is->plan.m) // (the plan's m is the most the tile's frames and LDS hold)
		return LW_ERR_UNSUPPORTED;
	is->m = m;
	return LW_OK;
}

int lw_istft_last_route(const lw_istft *is)
{
	return is ? is->last_route : -1;
}

int lw_istft_set_route(lw_istft *is, int route)
{
	if (!is)
		return LW_ERR_NULL_ARG;
	if (route != LW_IS_ROUTE_MFMA && route != LW_IS_ROUTE_FMA)
		return LW_ERR_UNSUPPORTED;
	is->route = route;
	return LW_OK;
}

int lw_istft_rows(lw_istft *is, uint32_t ch, const void *d_src, size_t n_src_rows, size_t frame_capacity, const uint64_t *frames, const uint32_t *dst_row,
		const uint64_t *out_len, int fmt, void *d_dst, size_t n_dst_rows, size_t dst_capacity, void *hip_stream)
{
	if (!is || (!frames && n_src_rows))
		return LW_ERR_NULL_ARG;
	if (fmt != LW_FMT_F32_PLANAR && fmt != LW_FMT_F32_INTERLEAVED)
		return LW_ERR_UNSUPPORTED;
	if (ch == 0 || ch > 255 || n_src_rows > UINT32_MAX)
		return LW_ERR_CAPACITY;
	const LwIstftPlan &p = is->plan;
	// both buffers must be addressable in 64 bits of BYTES
	if (!lw_rows_bytes_ok((uint64_t)ch * p.lines, frame_capacity, n_src_rows) || !lw_rows_bytes_ok(ch, dst_capacity, n_dst_rows))
		return LW_ERR_CAPACITY;
	// ---- plan: every row is checked before anything is queued, so a refused call has written nothing
	is->rows.clear();
	const uint64_t pad = is->center ? is->n_fft / 2u : 0u;
	uint64_t most = 0, most_frames = 0;
	size_t i = 0;
	if (int rc = lw_stage_mapped_rows(is->taken, n_src_rows, frames, dst_row, frame_capacity, n_dst_rows, [&](uint64_t T, uint64_t row) {
		    const uint64_t n = out_len ? out_len[i] : lw_is_natural(is, T);
		    i++;
		    if (n > dst_capacity)
			    return LW_ERR_CAPACITY;
		    is->rows.push_back(LwIstftRow{T, n, row});
		    most = std::max(most, n);
		    if (n)
			    most_frames = std::max(most_frames, T);
		    return LW_OK;
	    }))
		return rc;
	if ((most && !d_dst) || (most_frames && !d_src)) // (a row without frames is written as zeros and reads nothing)
		return LW_ERR_NULL_ARG;
	if (most == 0)
		return LW_OK;
	const uint64_t span = (uint64_t)is->m * is->hop, tiles = (pad + most + span - 1) / span; // (most <= a capacity: no overflow)
	if (tiles > INT32_MAX)
		return LW_ERR_CAPACITY;
	// ---- queue: the records, then the launches
	HIP_TRY(hipSetDevice(is->device));
	hipStream_t st = (hipStream_t)hip_stream;
	if (int rc = is->ring.acquire(n_src_rows))
		return rc;
	LwStageGuard staged = is->ring.guard(st);
	if (int rc = is->ring.upload(is->rows, st))
		return rc;
	const bool itl = fmt == LW_FMT_F32_INTERLEAVED;
	LwIstftArgs a{};
	a.src = (const float *)d_src, a.dst = (float *)d_dst, a.table = is->d_table, a.w2 = is->d_w2, a.rows = is->ring.dev();
	a.d = itl ? LwIstftLayout{(uint64_t)dst_capacity * ch, 1, ch} : LwIstftLayout{(uint64_t)dst_capacity * ch, dst_capacity, 1};
	a.s_line = frame_capacity, a.s_ch = (uint64_t)p.lines * frame_capacity, a.s_row = a.s_ch * ch;
	a.pad = pad;
	a.n_fft = is->n_fft, a.hop = is->hop, a.win_length = is->win_length, a.offset = p.offset, a.lines = p.lines, a.l_pad = p.l_pad, a.passes = p.passes;
	a.m = is->m;
	if (lw_stage_launch(n_src_rows, "lw_launch_istft", [&](uint32_t row0, uint32_t n) {
		    a.row0 = row0;
		    for (uint64_t t0 = 0; t0 < tiles; t0 += LW_IS_MAX_TILES) { // (a grid dimension holds fewer than 2^32 lanes)
			    a.tile0 = (uint32_t)t0;
			    const hipError_t e = lw_launch_istft(a, is->route, (uint32_t)std::min<uint64_t>(tiles - t0, LW_IS_MAX_TILES), ch, n, st);
			    if (e != hipSuccess)
				    return e;
		    }
		    return hipSuccess;
	    }) < 0)
		return LW_ERR_DEVICE;
	if (int rc = staged.commit())
		return rc;
	is->last_route = is->route;
	return LW_OK;
}

} // extern "C"
