// What every host program that runs a KERNEL source on the CPU shares (cep, fbank, feat, istft, lanes, norm, pack, resample, select, slide,
// spec, spec_complex, spec_reflect), included behind hip_standins.inc: the lw_hip_ok stand-in, the launch log, guarded buffers,
// sentinel fills, files that are read and written whole or not at all, and the exit codes.  rows_host, rows_mix_host and fmt_host
// take the file helpers alone.  tests/san/kernel_host_selftest.cpp holds the guarded buffer against ASan itself.  Test
// infrastructure only.
//
// Exit codes of these programs: 0 = ran (what it printed is the test's to judge), 2 = usage or I/O, 3 = the harness itself found
// something wrong and has said so in a "BAD ..." line.  Anything else is a sanitizer's report.
#pragma once

#include <sanitizer/asan_interface.h>

#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

[[noreturn]] static inline void bad(const char *fmt, ...) // "BAD <text>", exit 3
{
	va_list ap;
	va_start(ap, fmt);
	printf("BAD ");
	vprintf(fmt, ap);
	printf("\n");
	va_end(ap);
	exit(3);
}

#ifndef KERNEL_HOST_NO_HIP_OK // (defined by a program that links lw_runtime.cpp, which has the real one, or no HIP code at all)
bool lw_hip_ok(hipError_t e, const char *) // (lw_runtime.cpp's, without its thread-local text)
{
	return e == hipSuccess;
}
#endif

// ---- the launch log: what a pass's stand-in launchers were given, for the modes that queue without running ("two", "refuse")
template <class Row>
struct LaunchLog {
	int launches = 0;
	bool run = true; // false: the launchers check their arguments and return
	std::vector<std::pair<const Row *, uint32_t>> rows; // the records of each launch that has some, looked at again at the end

	void launch() { launches++; }
	void launch(const Row *r, uint32_t n) { launches++, rows.emplace_back(r, n); }

	// "ROWS ..." per launch, one(record) printing a record, then "LAUNCHES n".  Queued work reads its records later: they must
	// still be there after the calls behind it
	template <class One>
	void print(One one) const
	{
		for (const auto &g : rows) {
			printf("ROWS");
			for (uint32_t i = 0; i < g.second; i++)
				one(g.first[i]);
			printf("\n");
		}
		printf("LAUNCHES %d\n", launches);
	}
};

// ---- guarded buffers
// A buffer of exactly `bytes` bytes that starts OFF bytes behind a 16-byte boundary.  Its END is the allocation's end: one byte
// beyond it is an ASan report.  In FRONT of it lie 32 + OFF bytes of the same allocation (malloc returns 16-byte boundaries): they
// hold the sentinel and are poisoned by hand down to the last 8-byte granule ASan can express, so a 16-byte access that began
// before the first line -- the head group of a line that starts off a boundary -- is a report as well, and guard_intact() finds a
// store into what poisoning cannot cover
struct Guarded {
	char *base = nullptr, *at = nullptr;
	template <class T>
	T *as() const
	{
		return (T *)at;
	}
};

static const unsigned char GUARD_FRONT = 0x5a;

static inline Guarded shifted(size_t bytes, unsigned off)
{
	Guarded g;
	const size_t front = 32 + (size_t)(off & 15u);
	g.base = (char *)malloc(front + bytes);
	if (!g.base || ((uintptr_t)g.base & 15u))
		exit(2);
	g.at = g.base + front;
	memset(g.base, GUARD_FRONT, front);
	ASAN_POISON_MEMORY_REGION(g.base, front & ~(size_t)7);
	return g;
}

static inline bool guard_intact(const Guarded &g) // (unpoisons the front: the last look at a buffer, before its free)
{
	const size_t front = (size_t)(g.at - g.base);
	ASAN_UNPOISON_MEMORY_REGION(g.base, front);
	for (size_t i = 0; i < front; i++)
		if ((unsigned char)g.base[i] != GUARD_FRONT)
			return false;
	return true;
}

// ---- sentinels: NaNs with a payload, and the bf16 / f16 NaN of the packed destinations
static const uint32_t SENT_DEAD = 0x7fc0deadu, SENT_ABC = 0x7fc00abcu;
static const uint16_t SENT_HALF = 0x7fadu;

static inline void fill32(void *p, size_t n, uint32_t v) // n elements; p need not be aligned
{
	for (size_t i = 0; i < n; i++)
		memcpy((char *)p + 4 * i, &v, 4);
}

static inline void fill16(void *p, size_t n, uint16_t v)
{
	for (size_t i = 0; i < n; i++)
		memcpy((char *)p + 2 * i, &v, 2);
}

// ---- files: every read and write is whole, or the program ends with 2
struct File {
	FILE *f;
	File(const char *path, const char *mode) : f(fopen(path, mode))
	{
		if (!f)
			exit(2);
	}
	File(const File &) = delete;
	~File() { close(); }
	void read_exact(void *p, size_t bytes)
	{
		if (bytes && fread(p, 1, bytes, f) != bytes)
			exit(2);
	}
	void write_exact(const void *p, size_t bytes)
	{
		if (bytes && fwrite(p, 1, bytes, f) != bytes)
			exit(2);
	}
	template <class T>
	void get(T *p, size_t n) // n elements
	{
		read_exact(p, n * sizeof(T));
	}
	template <class T>
	void put(const T *p, size_t n)
	{
		write_exact(p, n * sizeof(T));
	}
	void close() // (a write can fail as late as here)
	{
		if (f && fclose(f) != 0)
			exit(2);
		f = nullptr;
	}
};

static inline std::vector<uint8_t> slurp(const char *path)
{
	File in(path, "rb");
	if (fseek(in.f, 0, SEEK_END) != 0)
		exit(2);
	const long n = ftell(in.f);
	if (n < 0 || fseek(in.f, 0, SEEK_SET) != 0)
		exit(2);
	std::vector<uint8_t> b((size_t)n);
	in.read_exact(b.data(), b.size());
	return b;
}

static inline std::vector<float> slurp_f32(const char *path) // the whole floats of a file
{
	const std::vector<uint8_t> raw = slurp(path);
	std::vector<float> v(raw.size() / 4);
	if (!v.empty())
		memcpy(v.data(), raw.data(), v.size() * 4);
	return v;
}
