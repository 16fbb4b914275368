// Row resampler (lw_resampler_*, lw_resample_rows; include/lewton_amd.h "resampling rows"): finished rows of f32 PCM
// ([row][ch][sample] or [row][sample][ch] in device memory) resampled by a rational ratio into another rows buffer, by a windowed-
// sinc polyphase filter whose taps and fold order are a contract on bits.  The taps are evaluated here in double and rounded once;
// everything about a call is decided here on the host before anything is queued (the refusals, the output lengths, the launch
// geometry); k_resample (lw_kernels_resample.hip) does the fold.  The call's per-row records are staged as lw_stage.hpp
// describes.  Nothing else in the library calls into this file.
#include "lw_stage.hpp"
#include "lw_resample.hpp"

#include <cmath>
#include <numeric>

struct lw_resampler {
	int device = 0;
	uint32_t orig = 0, new_ = 0, half_width = 0, k_taps = 0;
	std::vector<float> taps; // [new][K], the public order
	float *d_taps = nullptr; // [K][new] by n mod new, the kernel's order (lw_resample.hpp)
	LwStageRing<LwResampleRow> ring;
	bool taps_in_lds = true;
	int last_route = -1;
	std::vector<LwResampleRow> plan;
	std::vector<uint64_t> taken;
};

// I0 by its power series, sum of ((x / 2)^m / m!)^2, until a term no longer changes the sum
static double bessel_i0(double x)
{
	const double q = x * x / 4;
	double sum = 1, term = 1;
	for (double m = 1;; m += 1) {
		term *= q / (m * m);
		const double next = sum + term;
		if (next == sum)
			return sum;
		sum = next;
	}
}

static double tap_value(double s, double zeros, int window, double beta, double i0_beta, double t)
{
	const double u = s * t;
	if (!(std::fabs(u) < zeros))
		return 0;
	const double pu = M_PI * u;
	const double sinc = u == 0 ? 1.0 : std::sin(pu) / pu;
	double w;
	if (window == LW_RESAMPLE_HANN) {
		const double c = std::cos(pu / (2 * zeros));
		w = c * c;
	} else {
		const double r = u / zeros;
		w = bessel_i0(beta * std::sqrt(1 - r * r)) / i0_beta;
	}
	return s * sinc * w;
}

static uint64_t out_len_of(const lw_resampler *rs, uint64_t len)
{
	const unsigned __int128 p = (unsigned __int128)len * rs->new_ + (rs->orig - 1);
	const unsigned __int128 q = p / rs->orig;
	return q > UINT64_MAX ? UINT64_MAX : (uint64_t)q;
}

extern "C" {

lw_resampler *lw_resampler_create(int device, uint32_t in_rate, uint32_t out_rate, uint32_t zeros, double rolloff, int window, double beta,
		int *err)
{
	int dummy;
	if (!err)
		err = &dummy;
	*err = LW_OK;
	if (in_rate == 0 || out_rate == 0 || zeros == 0 || !(rolloff > 0 && rolloff <= 1) ||
			(window != LW_RESAMPLE_HANN && window != LW_RESAMPLE_KAISER) || (window == LW_RESAMPLE_KAISER && !(beta >= 0 && beta < 700))) {
		*err = LW_ERR_UNSUPPORTED;
		return nullptr;
	}
	const uint32_t g = std::gcd(in_rate, out_rate), orig = in_rate / g, new_ = out_rate / g;
	const double s = rolloff * (new_ < orig ? (double)new_ / (double)orig : 1.0);
	const double wd = std::ceil((double)zeros / s);
	if (!(wd >= 1) || (2 * wd + 2) * new_ > (double)LW_RESAMPLE_MAX_TAPS) {
		*err = LW_ERR_UNSUPPORTED;
		return nullptr;
	}
	if (lw_stage_device(device)) {
		*err = LW_ERR_DEVICE;
		return nullptr;
	}
	auto rs = std::make_unique<lw_resampler>();
	rs->device = device;
	rs->orig = orig, rs->new_ = new_;
	rs->half_width = (uint32_t)wd;
	rs->k_taps = 2 * rs->half_width + 2;
	const uint32_t W = rs->half_width, K = rs->k_taps;
	const double i0_beta = window == LW_RESAMPLE_KAISER ? bessel_i0(beta) : 1;
	rs->taps.resize((size_t)new_ * K);
	for (uint32_t ph = 0; ph < new_; ph++)
		for (uint32_t k = 0; k < K; k++) {
			const double t = ((double)k - (double)W) - (double)ph / (double)new_;
			rs->taps[(size_t)ph * K + k] = (float)tap_value(s, (double)zeros, window, beta, i0_beta, t); // the one rounding
		}
	std::vector<float> dev(((size_t)new_ * K + 3) & ~(size_t)3, 0.0f); // (padded: the kernel stages it 16 bytes at a time)
	for (uint32_t i = 0; i < new_; i++) {
		const uint32_t ph = (uint32_t)((uint64_t)i * orig % new_);
		for (uint32_t k = 0; k < K; k++)
			dev[(size_t)k * new_ + i] = rs->taps[(size_t)ph * K + k];
	}
	bool ok = lw_hip_ok(hipMalloc((void **)&rs->d_taps, dev.size() * sizeof(float)), "hipMalloc(resampler taps)") &&
		lw_hip_ok(hipMemcpy(rs->d_taps, dev.data(), dev.size() * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy(resampler taps)");
	if (!ok || !rs->ring.create("hipEventCreate(resampler rows)")) {
		*err = LW_ERR_DEVICE;
		lw_resampler_destroy(rs.release());
		return nullptr;
	}
	return rs.release();
}

void lw_resampler_destroy(lw_resampler *rs)
{
	if (!rs)
		return;
	(void)hipSetDevice(rs->device);
	(void)hipDeviceSynchronize();
	rs->ring.destroy();
	if (rs->d_taps)
		(void)hipFree(rs->d_taps);
	delete rs;
}

void lw_resampler_geometry(const lw_resampler *rs, uint32_t *orig, uint32_t *new_, uint32_t *half_width, uint32_t *taps_per_phase)
{
	if (orig)
		*orig = rs ? rs->orig : 0;
	if (new_)
		*new_ = rs ? rs->new_ : 0;
	if (half_width)
		*half_width = rs ? rs->half_width : 0;
	if (taps_per_phase)
		*taps_per_phase = rs ? rs->k_taps : 0;
}

size_t lw_resampler_taps(const lw_resampler *rs, float *dst)
{
	if (!rs)
		return 0;
	if (dst)
		std::memcpy(dst, rs->taps.data(), rs->taps.size() * sizeof(float));
	return rs->taps.size();
}

uint64_t lw_resampler_out_len(const lw_resampler *rs, uint64_t len)
{
	return rs ? out_len_of(rs, len) : 0;
}

int lw_resampler_set_taps_in_lds(lw_resampler *rs, int on)
{
	if (!rs)
		return LW_ERR_NULL_ARG;
	rs->taps_in_lds = on != 0;
	return LW_OK;
}

int lw_resampler_last_route(const lw_resampler *rs)
{
	return rs ? rs->last_route : -1;
}

int lw_resample_rows(lw_resampler *rs, int fmt, uint32_t ch, const void *d_src, size_t n_src_rows, size_t src_capacity, const uint64_t *len,
		const uint32_t *dst_row, void *d_dst, size_t n_dst_rows, size_t dst_capacity, void *hip_stream)
{
	if (!rs || (!len && n_src_rows))
		return LW_ERR_NULL_ARG;
	if (fmt != LW_FMT_F32_PLANAR && fmt != LW_FMT_F32_INTERLEAVED)
		return LW_ERR_UNSUPPORTED;
	if (ch == 0 || ch > 255 || n_src_rows > UINT32_MAX)
		return LW_ERR_CAPACITY;
	// both buffers must be addressable in 64 bits of BYTES
	if (!lw_rows_bytes_ok(ch, src_capacity, n_src_rows) || !lw_rows_bytes_ok(ch, dst_capacity, n_dst_rows))
		return LW_ERR_CAPACITY;
	// ---- plan: every row is checked before anything is queued, so a refused call has written nothing
	rs->plan.clear();
	uint64_t longest = 0;
	bool any_in = false;
	if (int rc = lw_stage_mapped_rows(rs->taken, n_src_rows, len, dst_row, src_capacity, n_dst_rows, [&](uint64_t len_i, uint64_t row) {
		    const uint64_t out = out_len_of(rs, len_i);
		    if (out > dst_capacity)
			    return LW_ERR_CAPACITY;
		    rs->plan.push_back(LwResampleRow{len_i, out, row});
		    longest = std::max(longest, out);
		    any_in = any_in || len_i != 0;
		    return LW_OK;
	    }))
		return rc;
	if ((any_in && !d_src) || (longest && !d_dst))
		return LW_ERR_NULL_ARG;
	const LwResamplePlan p = lw_resample_plan(rs->orig, rs->new_, rs->k_taps, rs->taps_in_lds);
	const uint64_t tiles = (longest + p.tile - 1) / p.tile;
	if (tiles > INT32_MAX)
		return LW_ERR_CAPACITY;
	if (longest == 0)
		return LW_OK;
	// ---- queue: the records, then the launches
	HIP_TRY(hipSetDevice(rs->device));
	hipStream_t st = (hipStream_t)hip_stream;
	if (int rc = rs->ring.acquire(n_src_rows))
		return rc;
	LwStageGuard staged = rs->ring.guard(st);
	if (int rc = rs->ring.upload(rs->plan, st))
		return rc;
	const bool itl = fmt == LW_FMT_F32_INTERLEAVED;
	LwResampleArgs a{};
	a.src = (const float *)d_src, a.dst = (float *)d_dst, a.taps = rs->d_taps, a.rows = rs->ring.dev();
	a.s = itl ? LwResampleLayout{(uint64_t)src_capacity * ch, 1, ch} : LwResampleLayout{(uint64_t)src_capacity * ch, src_capacity, 1};
	a.d = itl ? LwResampleLayout{(uint64_t)dst_capacity * ch, 1, ch} : LwResampleLayout{(uint64_t)dst_capacity * ch, dst_capacity, 1};
	a.orig = rs->orig, a.new_ = rs->new_, a.half_width = rs->half_width, a.k_taps = rs->k_taps, a.blocks = p.blocks;
	if (lw_stage_launch(n_src_rows, "lw_launch_resample", [&](uint32_t row0, uint32_t n) {
		    a.row0 = row0;
		    for (uint64_t t0 = 0; t0 < tiles; t0 += LW_RS_MAX_TILES) { // (a grid dimension holds fewer than 2^32 lanes)
			    a.tile0 = (uint32_t)t0;
			    const hipError_t e = lw_launch_resample(a, p, (uint32_t)std::min<uint64_t>(tiles - t0, LW_RS_MAX_TILES), ch, n, st);
			    if (e != hipSuccess)
				    return e;
		    }
		    return hipSuccess;
	    }) < 0)
		return LW_ERR_DEVICE;
	if (int rc = staged.commit())
		return rc;
	rs->last_route = p.route;
	return LW_OK;
}

} // extern "C"
