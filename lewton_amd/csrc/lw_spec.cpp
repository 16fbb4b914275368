// Spectral frames of rows (lw_spec_*, lw_spec_rows; include/lewton_amd.h "spectral frames of rows"): finished rows of f32 PCM
// ([row][ch][sample] or [row][sample][ch] in device memory) cut into overlapping frames and turned into a power spectrum or mel
// features, [row][ch][F][frame], by a windowed DFT whose basis and fold order are a contract on bits.  The basis is evaluated
// here in double and rounded once; everything about a call is decided here on the host before anything is queued (the refusals,
// the frame counts, the launch geometry); k_spec (lw_kernels_spec.hip) does the folds.  The call's per-row records are staged as
// lw_stage.hpp describes.  Nothing else in the library calls into this file.
#include "lw_stage.hpp"
#include "lw_spec.hpp"
#include "lw_window.hpp"

#include <cmath>

struct lw_spec {
	int device = 0;
	uint32_t n_fft = 0, win_length = 0, hop = 0, n_mels = 0;
	bool center = false;
	int pad_mode = LW_SPEC_PAD_ZERO;
	int framing = LW_SPEC_FRAMES_STFT;
	bool remove_dc = false, energy = false;
	int output = LW_SPEC_OUT_POWER;
	double scale = 1.0;
	LwSpecPlan plan{};
	std::vector<float> basis;                  // [2][win_length][B], the public order
	float *d_basis = nullptr, *d_fb = nullptr; // the kernel's orders (lw_spec.hpp)
	LwStageRing<LwSpecRow> ring;
	int route = LW_SP_ROUTE_MFMA, last_route = -1;
	std::vector<LwSpecRow> rows;
	std::vector<uint64_t> taken;
};

extern "C" {

lw_spec *lw_spec_create(int device, uint32_t n_fft, uint32_t win_length, uint32_t hop, int window, int center, uint32_t n_mels, const float *fb,
		int *err)
{
	if (window != LW_SPEC_HANN && window != LW_SPEC_RECT) { // this entry point keeps its two windows; the others come with lw_spec_create_ex
		if (err)
			*err = LW_ERR_UNSUPPORTED;
		return nullptr;
	}
	lw_spec_params p{};
	p.n_fft = n_fft, p.win_length = win_length, p.hop = hop, p.n_mels = n_mels, p.fb = fb;
	p.window = window, p.center = center, p.framing = LW_SPEC_FRAMES_STFT;
	p.preemphasis = 0.0, p.scale = 1.0;
	return lw_spec_create_ex(device, &p, err);
}

lw_spec *lw_spec_create_ex(int device, const lw_spec_params *prm, int *err)
{
	int dummy;
	if (!err)
		err = &dummy;
	*err = LW_OK;
	if (!prm) {
		*err = LW_ERR_NULL_ARG;
		return nullptr;
	}
	const uint32_t n_fft = prm->n_fft, win_length = prm->win_length, hop = prm->hop, n_mels = prm->n_mels;
	const int window = prm->window, center = prm->center;
	const float *fb = prm->fb;
	const bool kaldi = prm->framing == LW_SPEC_FRAMES_KALDI_SNIP || prm->framing == LW_SPEC_FRAMES_KALDI_EDGES;
	const bool symmetric = lw_sp_window_symmetric(window);
	if (n_fft < 2 || n_fft > LW_SPEC_MAX_FFT || win_length < 1 || win_length > n_fft || hop < 1 || hop > 65535 || n_mels > LW_SPEC_MAX_MELS ||
			(window != LW_SPEC_HANN && window != LW_SPEC_RECT && !symmetric) || (symmetric && win_length < 2) ||
			(prm->framing != LW_SPEC_FRAMES_STFT && !kaldi) || (kaldi && center) || (prm->remove_dc != 0 && prm->remove_dc != 1) ||
			(prm->energy != 0 && prm->energy != 1) || !(prm->preemphasis >= 0.0 && prm->preemphasis <= 1.0) ||
			!(prm->scale > 0.0 && std::isfinite(prm->scale)) || prm->reserved != 0 ||
			(prm->output != LW_SPEC_OUT_POWER && prm->output != LW_SPEC_OUT_COMPLEX) ||
			(prm->output == LW_SPEC_OUT_COMPLEX && (n_mels != 0 || prm->remove_dc != 0 || prm->energy != 0))) { // (the complex lines are the chains themselves)
		*err = LW_ERR_UNSUPPORTED;
		return nullptr;
	}
	if (n_mels && !fb) {
		*err = LW_ERR_NULL_ARG;
		return nullptr;
	}
	int lds_limit = 0;
	if (lw_stage_device(device) ||
			!lw_hip_ok(hipDeviceGetAttribute(&lds_limit, hipDeviceAttributeMaxSharedMemoryPerBlock, device), "hipDeviceGetAttribute(LDS per workgroup)") ||
			(size_t)lds_limit < LW_SP_LDS_FLOATS * sizeof(float)) { // k_spec's workgroup does not fit this device
		*err = LW_ERR_DEVICE;
		return nullptr;
	}
	auto sp = std::make_unique<lw_spec>();
	sp->device = device;
	sp->n_fft = n_fft, sp->win_length = win_length, sp->hop = hop, sp->n_mels = n_mels, sp->center = center != 0;
	sp->framing = prm->framing, sp->remove_dc = prm->remove_dc != 0, sp->energy = prm->energy != 0, sp->scale = prm->scale;
	sp->output = prm->output;
	if (prm->framing == LW_SPEC_FRAMES_KALDI_EDGES)
		sp->pad_mode = LW_SPEC_PAD_SYMMETRIC;
	sp->plan = lw_spec_plan(n_fft, win_length, n_mels);
	if (kaldi)
		sp->plan.offset = 0; // the window starts at sample 0 of the frame
	const LwSpecPlan p = sp->plan;
	const uint32_t B = p.bins;
	// ---- the tables, in double, each rounded once: pre-emphasis, window and scale folded in (c = 0 and scale = 1: g itself)
	sp->basis.resize((size_t)2 * win_length * B);
	std::vector<float> dev((size_t)p.passes * p.k_pad * 2 * LW_SP_COLS, 0.0f);
	const double c = prm->preemphasis, scale = prm->scale;
	std::vector<double> win(win_length);
	for (uint32_t i = 0; i < win_length; i++)
		win[i] = lw_sp_window(window, i, win_length);
	auto g = [&](uint32_t i, uint32_t j, bool sine) { // g_i of bin j; g_W = 0
		if (i >= win_length)
			return 0.0;
		const double w = win[i];
		const uint64_t k = (uint64_t)i + p.offset;
		const double ang = 2.0 * M_PI * (double)(k * j % n_fft) / (double)n_fft;
		return sine ? -w * std::sin(ang) : w * std::cos(ang);
	};
	for (uint32_t i = 0; i < win_length; i++)
		for (uint32_t j = 0; j < B; j++)
			for (uint32_t sine = 0; sine < 2u; sine++) {
				double v = g(i, j, sine != 0);
				if (c != 0.0)
					v = (i == 0 ? 1.0 - c : 1.0) * v - c * g(i + 1u, j, sine != 0);
				if (scale != 1.0)
					v = scale * v;
				const float r = (float)v;
				sp->basis[((size_t)sine * win_length + i) * B + j] = r;
				dev[lw_spec_basis_at(p, i, sine, j)] = r;
			}
	bool ok = lw_hip_ok(hipMalloc((void **)&sp->d_basis, dev.size() * sizeof(float)), "hipMalloc(spec basis)") &&
		lw_hip_ok(hipMemcpy(sp->d_basis, dev.data(), dev.size() * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy(spec basis)");
	if (ok && n_mels) {
		std::vector<float> m((size_t)p.j_pad * p.mel_pad, 0.0f);
		for (uint32_t q = 0; q < n_mels; q++)
			for (uint32_t j = 0; j < B; j++)
				m[(size_t)j * p.mel_pad + q] = fb[(size_t)q * B + j];
		ok = lw_hip_ok(hipMalloc((void **)&sp->d_fb, m.size() * sizeof(float)), "hipMalloc(spec mel matrix)") &&
			lw_hip_ok(hipMemcpy(sp->d_fb, m.data(), m.size() * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy(spec mel matrix)");
	}
	if (!ok || !sp->ring.create("hipEventCreate(spec rows)")) {
		*err = LW_ERR_DEVICE;
		lw_spec_destroy(sp.release());
		return nullptr;
	}
	return sp.release();
}

void lw_spec_destroy(lw_spec *sp)
{
	if (!sp)
		return;
	(void)hipSetDevice(sp->device);
	(void)hipDeviceSynchronize();
	sp->ring.destroy();
	if (sp->d_basis)
		(void)hipFree(sp->d_basis);
	if (sp->d_fb)
		(void)hipFree(sp->d_fb);
	delete sp;
}

uint32_t lw_spec_bins(const lw_spec *sp)
{
	return sp ? sp->plan.bins : 0;
}

uint32_t lw_spec_features(const lw_spec *sp)
{
	if (sp && sp->output == LW_SPEC_OUT_COMPLEX)
		return 2u * sp->plan.bins; // re[j] on line j, im[j] on line B + j
	return sp ? (sp->n_mels ? sp->n_mels : sp->plan.bins) + (sp->energy ? 1u : 0u) : 0;
}

uint64_t lw_spec_frames(const lw_spec *sp, uint64_t len)
{
	if (!sp)
		return 0;
	if (sp->framing != LW_SPEC_FRAMES_STFT)
		return lw_spec_kaldi_frames(len, sp->win_length, sp->hop, sp->framing == LW_SPEC_FRAMES_KALDI_SNIP);
	return lw_spec_n_frames(len, sp->n_fft, sp->hop, sp->center);
}

size_t lw_spec_basis(const lw_spec *sp, float *dst)
{
	if (!sp)
		return 0;
	if (dst)
		std::memcpy(dst, sp->basis.data(), sp->basis.size() * sizeof(float));
	return sp->basis.size();
}

uint32_t lw_spec_tile_frames(const lw_spec *sp)
{
	return sp ? LW_SP_TF : 0;
}

int lw_spec_last_route(const lw_spec *sp)
{
	return sp ? sp->last_route : -1;
}

int lw_spec_set_route(lw_spec *sp, int route)
{
	if (!sp)
		return LW_ERR_NULL_ARG;
	if (route != LW_SP_ROUTE_MFMA && route != LW_SP_ROUTE_FMA)
		return LW_ERR_UNSUPPORTED;
	sp->route = route;
	return LW_OK;
}

int lw_spec_pad_mode(const lw_spec *sp)
{
	return sp ? sp->pad_mode : -1;
}

int lw_spec_set_pad_mode(lw_spec *sp, int mode)
{
	if (!sp)
		return LW_ERR_NULL_ARG;
	if ((mode != LW_SPEC_PAD_ZERO && mode != LW_SPEC_PAD_REFLECT) || (mode == LW_SPEC_PAD_REFLECT && !sp->center) ||
			sp->framing != LW_SPEC_FRAMES_STFT) // (a Kaldi framing has its own)
		return LW_ERR_UNSUPPORTED;
	sp->pad_mode = mode;
	return LW_OK;
}

int lw_spec_rows(lw_spec *sp, int fmt, uint32_t ch, const void *d_src, size_t n_src_rows, size_t src_capacity, const uint64_t *len,
		const uint32_t *dst_row, void *d_dst, size_t n_dst_rows, size_t frame_capacity, void *hip_stream)
{
	if (!sp || (!len && n_src_rows))
		return LW_ERR_NULL_ARG;
	if (fmt != LW_FMT_F32_PLANAR && fmt != LW_FMT_F32_INTERLEAVED)
		return LW_ERR_UNSUPPORTED;
	if (ch == 0 || ch > 255 || n_src_rows > UINT32_MAX)
		return LW_ERR_CAPACITY;
	const uint64_t F = lw_spec_features(sp); // (the energy line counts)
	const bool kaldi = sp->framing != LW_SPEC_FRAMES_STFT;
	const int64_t lead = kaldi ? lw_spec_kaldi_lead(sp->win_length, sp->hop, sp->framing == LW_SPEC_FRAMES_KALDI_SNIP)
	                           : (int64_t)sp->plan.offset - (int64_t)(sp->center ? sp->n_fft / 2 : 0);
	// both buffers must be addressable in 64 bits of BYTES
	if (!lw_rows_bytes_ok(ch, src_capacity, n_src_rows) || !lw_rows_bytes_ok((uint64_t)ch * F, frame_capacity, n_dst_rows))
		return LW_ERR_CAPACITY;
	// ---- plan: every row is checked before anything is queued, so a refused call has written nothing
	sp->rows.clear();
	uint64_t most = 0;
	if (int rc = lw_stage_mapped_rows(sp->taken, n_src_rows, len, dst_row, src_capacity, n_dst_rows, [&](uint64_t len_i, uint64_t row) {
		    if (sp->pad_mode == LW_SPEC_PAD_REFLECT && len_i != 0 && len_i < lw_spec_reflect_min_len(sp->n_fft))
			    return LW_ERR_CAPACITY; // one reflection does not reach every support sample
		    const uint64_t frames = lw_spec_frames(sp, len_i);
		    if (frames > frame_capacity)
			    return LW_ERR_CAPACITY;
		    if (sp->pad_mode == LW_SPEC_PAD_SYMMETRIC && frames) {
			    // the first and the last index the row's frames touch (len <= the capacity of a buffer: no overflow); one reflection
			    // reaches [-len, 2 len - 1]
			    const int64_t first = lead, last = (int64_t)((frames - 1) * sp->hop) + lead + (int64_t)sp->win_length - 1, n = (int64_t)len_i;
			    if (first < -n || last > 2 * n - 1)
				    return LW_ERR_CAPACITY;
		    }
		    sp->rows.push_back(LwSpecRow{len_i, frames, row});
		    most = std::max(most, frames);
		    return LW_OK;
	    }))
		return rc;
	if (most && (!d_src || !d_dst)) // (a row with a frame has a sample)
		return LW_ERR_NULL_ARG;
	const uint64_t tiles = (most + LW_SP_TF - 1) / LW_SP_TF;
	if (tiles > INT32_MAX)
		return LW_ERR_CAPACITY;
	if (most == 0)
		return LW_OK;
	// ---- queue: the records, then the launches
	HIP_TRY(hipSetDevice(sp->device));
	hipStream_t st = (hipStream_t)hip_stream;
	if (int rc = sp->ring.acquire(n_src_rows))
		return rc;
	LwStageGuard staged = sp->ring.guard(st);
	if (int rc = sp->ring.upload(sp->rows, st))
		return rc;
	const bool itl = fmt == LW_FMT_F32_INTERLEAVED;
	const LwSpecPlan &p = sp->plan;
	LwSpecArgs a{};
	a.src = (const float *)d_src, a.dst = (float *)d_dst, a.basis = sp->d_basis, a.fb = sp->d_fb, a.rows = sp->ring.dev();
	a.s = itl ? LwSpecLayout{(uint64_t)src_capacity * ch, 1, ch} : LwSpecLayout{(uint64_t)src_capacity * ch, src_capacity, 1};
	a.d_line = frame_capacity, a.d_ch = F * frame_capacity, a.d_row = a.d_ch * ch;
	a.lead = lead;
	if (sp->remove_dc || sp->energy) {
		a.remove_dc = sp->remove_dc, a.energy = sp->energy, a.escale = sp->scale * sp->scale;
		a.span = lw_spec_span_fits(sp->hop, sp->win_length) ? (LW_SP_TF - 1u) * sp->hop + sp->win_length : 0u;
	}
	a.hop = sp->hop, a.win_length = sp->win_length, a.k_pad = p.k_pad, a.bins = p.bins, a.passes = p.passes, a.n_mels = sp->n_mels, a.mel_pad = p.mel_pad;
	a.pad_mode = (uint32_t)sp->pad_mode;
	a.output = (uint32_t)sp->output;
	if (lw_stage_launch(n_src_rows, "lw_launch_spec", [&](uint32_t row0, uint32_t n) {
		    a.row0 = row0;
		    for (uint64_t t0 = 0; t0 < tiles; t0 += LW_SP_MAX_TILES) { // (a grid dimension holds fewer than 2^32 lanes)
			    a.tile0 = (uint32_t)t0;
			    const hipError_t e = lw_launch_spec(a, sp->route, (uint32_t)std::min<uint64_t>(tiles - t0, LW_SP_MAX_TILES), ch, n, st);
			    if (e != hipSuccess)
				    return e;
		    }
		    return hipSuccess;
	    }) < 0)
		return LW_ERR_DEVICE;
	if (int rc = staged.commit())
		return rc;
	sp->last_route = sp->route;
	return LW_OK;
}

} // extern "C"
