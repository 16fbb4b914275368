// The public sample formats (LW_FMT_* in include/lewton_amd.h): the one place that says which exist and how they are laid out.
// Host code only, no HIP: included by lw_internal.hpp and by the translation units that work on the public ABI alone.
#pragma once

#include "../../include/lewton_amd.h"

#include <stddef.h>

inline bool lw_fmt_valid(int fmt)
{
	return fmt >= LW_FMT_I16_PLANAR && fmt <= LW_FMT_F32_INTERLEAVED;
}
inline size_t lw_elem_size(int fmt)
{
	return fmt == LW_FMT_F32_PLANAR || fmt == LW_FMT_F32_INTERLEAVED ? 4 : 2;
}
// per packet [m][ch] (InterleavedSamples<S>) rather than [ch][m]
inline bool lw_fmt_interleaved(int fmt)
{
	return fmt == LW_FMT_I16_INTERLEAVED || fmt == LW_FMT_F32_INTERLEAVED;
}
