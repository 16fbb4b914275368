// The staged records of the row-chain entry points (lewton_amd/csrc/lw_stage.hpp) WITHOUT a GPU, with a model of what is in
// flight: lw_resample.cpp, lw_spec.cpp, lw_feat.cpp, lw_norm.cpp and lw_cep.cpp linked against the stand-ins below, which do no
// work but keep books.  hipMemcpyAsync copies at once and notes its source and its destination as ranges in flight, each
// launcher notes the records (and the scratch) it was handed, hipEventRecord stores the sequence number reached in the event,
// and the three synchronising calls retire every range up to theirs.  Starting a hipMemcpyAsync whose source or destination
// overlaps a range in flight, or freeing memory that holds one, ends the program with a message that names the call.
// Only the public entry points are driven, at the smallest shapes: 1 channel, 2 feature lines, a capacity of 8.
// Built with -fsanitize=address,undefined; tests/test_host_stage_ring.py drives it.
//   stage_host ENTRY CASE      ENTRY: resample | spec | feat | norm | cep
//     rotate   four calls back to back: slots 0, 1, 2, 0, and ONE hipEventSynchronize, before the fourth upload, on the first
//              call's event
//     fail     a call whose last launch fails (feat, norm: the second pass's, so that the first pass is in flight): LW_ERR_DEVICE;
//              then calls of 1, 65, 66, 67 and 68 rows (every slot regrown, once with nothing in between): LW_OK each
//     many     65 536 rows of length 1: per pass two launches, of rows 0 .. 65534 and of row 65535
//     norecord hipEventRecord fails at the end of a call: LW_ERR_DEVICE, the stream synchronised, nothing left in flight, and
//              the object takes the next calls
//   prints "OK" and exits 0, or a message and exits 1
#include "../../include/lewton_amd.h"

#include "../../lewton_amd/csrc/lw_cep.hpp"
#include "../../lewton_amd/csrc/lw_feat.hpp"
#include "../../lewton_amd/csrc/lw_norm.hpp"
#include "../../lewton_amd/csrc/lw_resample.hpp"
#include "../../lewton_amd/csrc/lw_spec.hpp"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <string>
#include <vector>

// ---- the books

struct Range {
	const char *lo, *hi;
	uint64_t seq;
	const char *what;
};
struct Event {
	uint64_t seq = 0;
};
struct Launch {
	const void *rows; // the records of the CALL (a.rows), row0 not added
	uint32_t row0, n_rows;
};

static std::vector<Range> g_flight;
static uint64_t g_seq = 0;
static std::map<const char *, size_t> g_alloc; // device and pinned memory: start -> bytes
static std::vector<Launch> g_launches;
static std::vector<uint64_t> g_upload_at;                  // g_seq of every hipMemcpyAsync
static std::vector<std::pair<Event *, uint64_t>> g_waited; // hipEventSynchronize: the event, g_seq at the time
static std::vector<Event *> g_recorded;
static int g_stream_syncs = 0;
static int g_fail_launch = 0, g_fail_record = 0; // n > 0: the n-th from now fails, once
static const char *g_entry = "";

[[noreturn]] static void fail(const char *fmt, ...)
{
	va_list ap;
	va_start(ap, fmt);
	printf("stage_host: lw_%s_rows: ", g_entry);
	vprintf(fmt, ap);
	printf("\n");
	va_end(ap);
	exit(1);
}

static bool countdown(int &n)
{
	return n > 0 && --n == 0;
}

static void note(const void *p, size_t bytes, const char *what)
{
	g_flight.push_back(Range{(const char *)p, (const char *)p + bytes, ++g_seq, what});
}

static void retire(uint64_t upto)
{
	size_t k = 0;
	for (const Range &r : g_flight)
		if (r.seq > upto)
			g_flight[k++] = r;
	g_flight.resize(k);
}

static void must_be_idle(const char *call, const char *role, const void *p, size_t bytes)
{
	for (const Range &r : g_flight)
		if ((const char *)p < r.hi && r.lo < (const char *)p + bytes)
			fail("%s: %s overlaps %s, which is still in flight", call, role, r.what);
}

static hipError_t allocate(void **p, size_t n)
{
	*p = malloc(n ? n : 1);
	if (!*p)
		return hipErrorOutOfMemory;
	g_alloc[(const char *)*p] = n ? n : 1;
	return hipSuccess;
}

static hipError_t release(const char *call, void *p)
{
	const auto it = g_alloc.find((const char *)p);
	if (it == g_alloc.end())
		fail("%s of memory that is not allocated", call);
	must_be_idle(call, "the memory", p, it->second);
	g_alloc.erase(it);
	free(p);
	return hipSuccess;
}

bool lw_hip_ok(hipError_t e, const char *) // (lw_runtime.cpp's, without its thread-local text)
{
	return e == hipSuccess;
}

extern "C" {
hipError_t hipGetDeviceCount(int *n) { *n = 1; return hipSuccess; }
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipDeviceGetAttribute(int *v, hipDeviceAttribute_t, int) { *v = 160 * 1024; return hipSuccess; }
hipError_t hipMalloc(void **p, size_t n) { return allocate(p, n); }
hipError_t hipHostMalloc(void **p, size_t n, unsigned) { return allocate(p, n); }
hipError_t hipFree(void *p) { return release("hipFree", p); }
hipError_t hipHostFree(void *p) { return release("hipHostFree", p); }
hipError_t hipMemcpy(void *d, const void *s, size_t n, hipMemcpyKind) // (the tables of a create: synchronous)
{
	if (n)
		memcpy(d, s, n);
	return hipSuccess;
}
hipError_t hipMemcpyAsync(void *d, const void *s, size_t n, hipMemcpyKind, hipStream_t)
{
	must_be_idle("hipMemcpyAsync", "the source", s, n);
	must_be_idle("hipMemcpyAsync", "the destination", d, n);
	memcpy(d, s, n);
	note(s, n, "the source of an upload");
	note(d, n, "the destination of an upload");
	g_upload_at.push_back(g_seq);
	return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { *e = (hipEvent_t) new Event; return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t e) { delete (Event *)e; return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t)
{
	if (countdown(g_fail_record))
		return hipErrorInvalidValue;
	((Event *)e)->seq = g_seq;
	g_recorded.push_back((Event *)e);
	return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t e)
{
	g_waited.emplace_back((Event *)e, g_seq);
	retire(((Event *)e)->seq);
	return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t) { g_stream_syncs++; retire(g_seq); return hipSuccess; }
hipError_t hipDeviceSynchronize(void) { retire(g_seq); return hipSuccess; }
}

// a launch: what it will read and write is in flight from now on -- unless it is the one that fails, which queues nothing
static hipError_t launched(const void *rows, size_t rec, uint32_t row0, uint32_t n_rows, std::initializer_list<const void *> scratch = {})
{
	if (!rows || n_rows == 0 || n_rows > 65535u)
		fail("a launch of %u rows from %p", n_rows, rows);
	if (countdown(g_fail_launch))
		return hipErrorLaunchFailure;
	g_launches.push_back(Launch{rows, row0, n_rows});
	note((const char *)rows + (size_t)row0 * rec, (size_t)n_rows * rec, "the records of a launch");
	for (const void *p : scratch)
		if (p)
			note(p, 1, "the scratch of a launch");
	return hipSuccess;
}

hipError_t lw_launch_resample(const LwResampleArgs &a, const LwResamplePlan &, uint32_t, uint32_t, uint32_t n_rows, hipStream_t)
{
	return launched(a.rows, sizeof(LwResampleRow), a.row0, n_rows);
}
hipError_t lw_launch_spec(const LwSpecArgs &a, int, uint32_t, uint32_t, uint32_t n_rows, hipStream_t)
{
	return launched(a.rows, sizeof(LwSpecRow), a.row0, n_rows);
}
hipError_t lw_launch_feat_log(const LwFeatArgs &a, uint32_t n_rows, hipStream_t) { return launched(a.rows, sizeof(LwFeatRow), a.row0, n_rows, {a.part}); }
hipError_t lw_launch_feat_fin(const LwFeatArgs &a, uint32_t n_rows, hipStream_t) { return launched(a.rows, sizeof(LwFeatRow), a.row0, n_rows, {a.part}); }
hipError_t lw_launch_norm_sum(const LwNormArgs &a, uint32_t n_rows, hipStream_t)
{
	return launched(a.rows, sizeof(LwNormRow), a.row0, n_rows, {a.part, a.scratch, a.sc});
}
hipError_t lw_launch_norm_fold(const LwNormArgs &a, uint32_t n_rows, hipStream_t)
{
	return launched(a.rows, sizeof(LwNormRow), a.row0, n_rows, {a.part, a.scratch, a.sc});
}
hipError_t lw_launch_norm_apply(const LwNormArgs &a, uint32_t n_rows, hipStream_t)
{
	return launched(a.rows, sizeof(LwNormRow), a.row0, n_rows, {a.part, a.scratch, a.sc});
}
hipError_t lw_launch_cep(const LwCepArgs &a, const float *, const float *, float *, uint32_t, uint32_t n_rows, hipStream_t)
{
	return launched(a.rows, sizeof(LwCepRow), a.row0, n_rows);
}

// ---- the five entry points, each as "a call of n_rows rows of length 1"

struct Entry {
	std::function<int(size_t)> call;
	std::function<void()> destroy;
	int passes = 1;    // launches of a call of up to 65535 rows
	int fail_pass = 1; // the pass whose launch fails in "fail"
};

static float g_buf[1]; // the rows buffers: never dereferenced, the launchers do no work

static Entry make(const std::string &name)
{
	int err = 0;
	Entry e;
	static std::vector<uint64_t> ones;
	auto len = [](size_t n) {
		ones.assign(n, 1);
		return ones.data();
	};
	if (name == "resample") {
		lw_resampler *rs = lw_resampler_create(0, 2, 1, 2, 0.9, LW_RESAMPLE_HANN, 0.0, &err);
		e.call = [=](size_t n) { return lw_resample_rows(rs, LW_FMT_F32_PLANAR, 1, g_buf, n, 8, len(n), nullptr, g_buf, n, 8, nullptr); };
		e.destroy = [=] { lw_resampler_destroy(rs); };
	} else if (name == "spec") {
		lw_spec *sp = lw_spec_create(0, 2, 2, 1, LW_SPEC_HANN, 1, 0, nullptr, &err); // 2 bins; a row of 1 sample has 2 frames
		e.call = [=](size_t n) { return lw_spec_rows(sp, LW_FMT_F32_PLANAR, 1, g_buf, n, 8, len(n), nullptr, g_buf, n, 8, nullptr); };
		e.destroy = [=] { lw_spec_destroy(sp); };
	} else if (name == "feat") {
		const lw_feat_params p{LW_FEAT_LOG_LOG10, LW_FEAT_SCOPE_ROW, 1e-10f, 8.0f, 0.0f, 1.0f}; // a finite top: two passes
		lw_feat *ft = lw_feat_create(0, &p, &err);
		e.call = [=](size_t n) { return lw_feat_rows(ft, 1, 2, g_buf, g_buf, n, 8, len(n), nullptr, nullptr, nullptr); };
		e.destroy = [=] { lw_feat_destroy(ft); };
		e.passes = e.fail_pass = 2;
	} else if (name == "norm") {
		const lw_norm_params p{1, LW_NORM_SCALE_STD, LW_NORM_SCOPE_CHANNEL, 0, 1e-7, 1.0}; // centred: sums, fold, apply
		lw_norm *nm = lw_norm_create(0, &p, &err);
		e.call = [=](size_t n) { return lw_norm_rows(nm, 1, 2, g_buf, g_buf, n, 8, len(n), nullptr, nullptr, nullptr); };
		e.destroy = [=] { lw_norm_destroy(nm); };
		e.passes = 3, e.fail_pass = 2;
	} else if (name == "cep") {
		lw_cep *cp = lw_cep_create(0, 2, 2, nullptr, 0, 0, &err);
		e.call = [=](size_t n) { return lw_cep_rows(cp, 1, g_buf, g_buf, n, 8, len(n), nullptr, nullptr); };
		e.destroy = [=] { lw_cep_destroy(cp); };
	}
	if (!e.call || err != LW_OK)
		fail("no such entry point, or its create failed (%d)", err);
	return e;
}

#define EXPECT(cond, ...)         \
	do {                          \
		if (!(cond))              \
			fail(__VA_ARGS__);    \
	} while (0)

int main(int argc, char **argv)
{
	if (argc != 3)
		return 2;
	const std::string mode = argv[2];
	g_entry = argv[1];
	Entry e = make(argv[1]);
	const size_t P = (size_t)e.passes;
	if (mode == "rotate") {
		for (int i = 0; i < 4; i++) {
			EXPECT(e.call(2) == LW_OK, "call %d is refused", i);
			EXPECT(g_waited.size() == (i == 3 ? 1u : 0u), "%zu waits for an event after call %d", g_waited.size(), i);
		}
		EXPECT(g_launches.size() == 4 * P && g_upload_at.size() == 4 && g_recorded.size() == 4, "4 calls made %zu launches, %zu uploads, %zu records",
				g_launches.size(), g_upload_at.size(), g_recorded.size());
		const void *slot[4];
		for (int i = 0; i < 4; i++) {
			slot[i] = g_launches[i * P].rows;
			for (size_t k = 1; k < P; k++)
				EXPECT(g_launches[i * P + k].rows == slot[i], "the passes of call %d read different records", i);
		}
		EXPECT(slot[0] != slot[1] && slot[1] != slot[2] && slot[0] != slot[2] && slot[3] == slot[0], "the slots are not 0, 1, 2, 0");
		EXPECT(g_waited[0].first == g_recorded[0], "the wait is not for the first call's event");
		EXPECT(g_waited[0].second < g_upload_at[3] && g_waited[0].second >= g_upload_at[2], "the wait is not between the third and the fourth upload");
		EXPECT(g_stream_syncs == 0, "the stream was synchronised");
	} else if (mode == "fail") {
		EXPECT(e.call(2) == LW_OK, "the first call is refused"); // (so that the failing call is not the object's first)
		g_fail_launch = e.fail_pass;
		EXPECT(e.call(2) == LW_ERR_DEVICE, "a call whose launch failed does not say so");
		EXPECT(g_launches.size() == P + (size_t)e.fail_pass - 1, "%zu launches", g_launches.size());
		for (size_t n : {1, 65, 66, 67, 68})
			EXPECT(e.call(n) == LW_OK, "the call of %zu rows after the failed one is refused", n);
		EXPECT(g_stream_syncs == 0, "the stream was synchronised");
	} else if (mode == "many") {
		EXPECT(e.call(65536) == LW_OK, "the call is refused");
		EXPECT(g_launches.size() == 2 * P, "%zu launches", g_launches.size());
		for (size_t k = 0; k < 2 * P; k++) {
			const Launch &l = g_launches[k];
			EXPECT(l.row0 == (k % 2 ? 65535u : 0u) && l.n_rows == (k % 2 ? 1u : 65535u), "launch %zu is of %u rows from row %u", k, l.n_rows, l.row0);
		}
	} else if (mode == "norecord") {
		EXPECT(e.call(2) == LW_OK, "the first call is refused");
		g_fail_record = 1;
		EXPECT(e.call(2) == LW_ERR_DEVICE, "a call whose event was not recorded does not say so");
		EXPECT(g_launches.size() == 2 * P, "%zu launches", g_launches.size());
		EXPECT(g_stream_syncs == 1, "the stream was synchronised %d times", g_stream_syncs);
		EXPECT(g_flight.empty(), "%zu ranges are in flight behind the synchronised stream", g_flight.size());
		for (size_t n : {1, 65, 66, 67, 68})
			EXPECT(e.call(n) == LW_OK, "the call of %zu rows after the failed one is refused", n);
		EXPECT(g_stream_syncs == 1 && g_recorded.size() == 6, "%d stream synchronisations, %zu records", g_stream_syncs, g_recorded.size());
	} else {
		return 2;
	}
	e.destroy();
	EXPECT(g_alloc.empty(), "%zu allocations are left", g_alloc.size());
	printf("OK\n");
	return 0;
}
