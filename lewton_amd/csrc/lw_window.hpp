// The analysis windows of lw_spec (include/lewton_amd.h, "spectral frames of rows"), in double: one evaluation for lw_spec.cpp's
// basis and for lw_istft.cpp's synthesis table and envelope, so that the two sides of a round trip hold the same w[i] to the bit.
// Host only.
#pragma once
#include "../../include/lewton_amd.h"

#include <cmath>

// w[i] of a window of W samples, in double
static inline double lw_sp_window(int window, uint32_t i, uint32_t W)
{
	if (window == LW_SPEC_RECT)
		return 1.0;
	if (window == LW_SPEC_HANN)
		return 0.5 - 0.5 * std::cos(2.0 * M_PI * (double)i / (double)W);
	const double a = 2.0 * M_PI * (double)i / (double)(W - 1u);
	if (window == LW_SPEC_HAMMING)
		return 0.54 - 0.46 * std::cos(a);
	if (window == LW_SPEC_HANN_SYM)
		return 0.5 - 0.5 * std::cos(a);
	if (window == LW_SPEC_POVEY)
		return std::pow(0.5 - 0.5 * std::cos(a), 0.85);
	return 0.42 - 0.5 * std::cos(a) + 0.08 * std::cos(2.0 * a); // LW_SPEC_BLACKMAN
}

static inline bool lw_sp_window_symmetric(int window)
{
	return window == LW_SPEC_POVEY || window == LW_SPEC_HAMMING || window == LW_SPEC_HANN_SYM || window == LW_SPEC_BLACKMAN;
}
