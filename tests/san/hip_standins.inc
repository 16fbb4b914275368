// Stand-ins for the HIP runtime and the kernel launchers, for GPU-less harnesses of the product's HOST code: device memory =
// calloc, copies = memcpy, kernels = no-ops, so everything the host decides (statuses, sample counts, offsets, staging records,
// container logic) is real and every sample value is zero.  Included by tools/micro/batch_host_bench.cpp and by every program of
// tests/san/ that links product sources which call HIP (all but stage_host.cpp, which keeps books of its own stand-ins, and the
// programs without HIP code: dev_entropy_host, host_fuzz, ogg_fuzz).  The programs that run a KERNEL source on the CPU supply
// that pass's launcher themselves and put kernel_host.hpp on top of this file.  Test infrastructure only -- never linked into
// liblewton_amd.so.
#include "../../lewton_amd/csrc/lw_fast.hpp"
#include "../../lewton_amd/csrc/lw_kernels.hpp"

#include <atomic>
#include <cstdlib>
#include <cstring>

// failure injection: n > 0 makes the n-th synthesis launch from now (any of the launchers below) fail, once
std::atomic<int> lw_standin_fail_launch{0};
static hipError_t standin_launch()
{
	if (lw_standin_fail_launch.load() > 0 && lw_standin_fail_launch.fetch_sub(1) == 1)
		return hipErrorLaunchFailure;
	return hipSuccess;
}

extern "C" {
hipError_t hipGetDeviceCount(int *n) { *n = 1; return hipSuccess; }
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipGetDevice(int *d) { *d = 0; return hipSuccess; }
hipError_t hipDeviceGetAttribute(int *v, hipDeviceAttribute_t a, int)
{
	*v = a == hipDeviceAttributeMultiprocessorCount ? 256 : 160 * 1024;
	return hipSuccess;
}
hipError_t hipDeviceSynchronize(void) { return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
hipError_t hipGetLastError(void) { return hipSuccess; }
const char *hipGetErrorString(hipError_t) { return "stub"; }
hipError_t hipMalloc(void **p, size_t n) { *p = calloc(1, n ? n : 1); return *p ? hipSuccess : hipErrorOutOfMemory; }
hipError_t hipFree(void *p) { free(p); return hipSuccess; }
hipError_t hipHostMalloc(void **p, size_t n, unsigned) { *p = calloc(1, n ? n : 1); return *p ? hipSuccess : hipErrorOutOfMemory; }
hipError_t hipHostFree(void *p) { free(p); return hipSuccess; }
hipError_t hipHostGetDevicePointer(void **d, void *h, unsigned) { *d = h; return hipSuccess; }
hipError_t hipMemset(void *d, int v, size_t n) { if (n) memset(d, v, n); return hipSuccess; }
hipError_t hipMemcpy(void *d, const void *s, size_t n, hipMemcpyKind) { if (n) memcpy(d, s, n); return hipSuccess; }
hipError_t hipMemcpyAsync(void *d, const void *s, size_t n, hipMemcpyKind, hipStream_t) { if (n) memcpy(d, s, n); return hipSuccess; }
hipError_t hipMemsetAsync(void *d, int v, size_t n, hipStream_t) { if (n) memset(d, v, n); return hipSuccess; }
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned) { *s = (hipStream_t)calloc(1, 8); return hipSuccess; }
hipError_t hipExtStreamCreateWithCUMask(hipStream_t *s, uint32_t, const uint32_t *) { *s = (hipStream_t)calloc(1, 8); return hipSuccess; }
hipError_t hipStreamDestroy(hipStream_t s) { free((void *)s); return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { *e = (hipEvent_t)calloc(1, 8); return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t e) { free((void *)e); return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t) { return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t, unsigned) { return hipSuccess; }
hipError_t hipGetDeviceProperties(hipDeviceProp_t *p, int) // (the header maps the name onto the versioned symbol)
{
	memset(p, 0, sizeof(*p));
	strcpy(p->gcnArchName, "gfx950:sramecc+:xnack-");
	p->multiProcessorCount = 256;
	return hipSuccess;
}
hipError_t hipMemcpy2D(void *d, size_t dp, const void *s, size_t sp, size_t w, size_t h, hipMemcpyKind)
{
	for (size_t i = 0; i < h; i++)
		memcpy((char *)d + i * dp, (const char *)s + i * sp, w);
	return hipSuccess;
}
}
hipError_t lw_launch_generic_imdct(const LwDevTables &, const LwBatchDev &, float *, hipStream_t, uint32_t, bool, bool) { return standin_launch(); }
hipError_t lw_launch_entropy(const LwEntTables &, const LwEntPacket *, const LwPacketRec *, const uint32_t *, uint16_t *, float *, uint32_t,
		hipStream_t) { return hipSuccess; }
void lw_launch_generic_ola(const LwDevTables &, const LwBatchDev &, void *, int, hipStream_t, bool) {}
hipError_t lw_launch_prep(const LwDevTables &, const LwBatchDev &, const uint32_t *, uint32_t, const uint8_t *, uint16_t *, hipStream_t) { return standin_launch(); }
hipError_t lw_launch_long(const LwDevTables &, const LwBatchDev &, const LwFastLaunch &, void *, int, hipStream_t) { return standin_launch(); }
hipError_t lw_launch_long10(const LwDevTables &, const LwBatchDev &, const LwFastLaunch &, void *, int, hipStream_t) { return standin_launch(); }
hipError_t lw_launch_long12(const LwDevTables &, const LwBatchDev &, const LwFastLaunch &, void *, int, hipStream_t) { return standin_launch(); }
hipError_t lw_launch_short(const LwDevTables &, const LwBatchDev &, const LwShortLaunch &, void *, int, hipStream_t) { return hipSuccess; }
hipError_t lw_launch_big(const LwDevTables &, const LwBatchDev &, const LwShortLaunch &, void *, int, hipStream_t) { return standin_launch(); }
bool lw_mix_applicable(const LwFastLaunch &, const LwShortLaunch &, int) { return false; }
bool lw_mix10_applicable(const LwFastLaunch &, const LwShortLaunch &, int) { return false; }
hipError_t lw_launch_mix10(const LwDevTables &, const LwBatchDev &, const LwFastLaunch &, const LwShortLaunch &, uint32_t *, uint32_t *, uint32_t, bool,
		void *, int, hipStream_t) { return standin_launch(); }
hipError_t lw_launch_mix(const LwDevTables &, const LwBatchDev &, const LwFastLaunch &, const LwShortLaunch &, uint32_t *, uint32_t *, uint32_t, bool,
		void *, int, hipStream_t) { return standin_launch(); }

