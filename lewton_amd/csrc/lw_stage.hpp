// What the row-chain entry points (lw_resample_rows, lw_spec_rows, lw_feat_rows, lw_norm_rows, lw_cep_rows; lw_rows_synth and
// lw_rows_synth_mix for the guard and the size check) share on the host: choosing the device, the staged records, the size
// check of a rows buffer, the launch loop and the two loops that check a call's rows.  Host only; no .hip file sees it.
//
// THE STAGED RECORDS.  A call's per-row records are complete in a host vector before anything is queued.  They travel to the
// device through one of LW_STAGE_SLOTS slots taken in rotation, so that calls queued back to back do not wait for each other's
// kernels: a slot is a pinned array (the source of the asynchronous copy), a device array (what the launches read) and an
// event recorded behind the last launch of the call that used it.  A call
//   acquires  the next slot: waits for the slot's event if the slot is pending, and grows both arrays to max(n, 64) records
//             (free, then allocate) where they are too small; device scratch of the same rotation (LwStageBuf) grows here too,
//   uploads   its records: memcpy into the pinned array, hipMemcpyAsync behind it on the call's stream,
//   launches, and
//   commits:  records the slot's event on the stream, marks the slot pending and moves the rotation on.
// The commit is a scope guard (LwStageGuard).  From the upload on, EVERY way out of the calling function commits, a failed launch
// in the middle of a call included: what did get queued may still read the slot, so the slot must not look idle to the next
// call.  Where the event cannot be recorded either, the guard waits for the stream instead and leaves the slot idle, which it
// then is.  A slot that may be in flight is never left unmarked.
#pragma once
#include "lw_internal.hpp"

#include <algorithm>
#include <cstring>

#define LW_STAGE_SLOTS 3
#define LW_STAGE_ROWS 65535u // rows of one launch: what a grid counts in its last dimension

// the top of every *_create: LW_OK with `device` current, or LW_ERR_DEVICE
inline int lw_stage_device(int device)
{
	int ndev = 0;
	if (!lw_hip_ok(hipGetDeviceCount(&ndev), "hipGetDeviceCount") || device < 0 || device >= ndev || !lw_hip_ok(hipSetDevice(device), "hipSetDevice"))
		return LW_ERR_DEVICE;
	return LW_OK;
}

// [n_rows][lines][capacity] elements of elem_size bytes are addressable in 64 bits of BYTES
inline bool lw_rows_bytes_ok(uint64_t lines, uint64_t capacity, uint64_t n_rows, uint64_t elem_size = 4)
{
	uint64_t e = 0;
	return !__builtin_mul_overflow(lines, capacity, &e) && !__builtin_mul_overflow(e, n_rows, &e) && e <= UINT64_MAX / elem_size;
}

// launch(row0, count) once per LW_STAGE_ROWS rows: the number of launches, or -1 after one that failed (`what` names it in
// lw_last_device_error)
template <class Launch> inline int lw_stage_launch(size_t n_rows, const char *what, Launch &&launch)
{
	int launches = 0;
	for (size_t r0 = 0; r0 < n_rows; r0 += LW_STAGE_ROWS, launches++)
		if (!lw_hip_ok(launch((uint32_t)r0, (uint32_t)std::min<size_t>(n_rows - r0, LW_STAGE_ROWS)), what))
			return -1;
	return launches;
}

// device scratch that grows on demand and keeps its contents for nobody: free, then allocate
struct LwStageBuf {
	void *p = nullptr;
	size_t bytes = 0;
	int reserve(size_t need)
	{
		if (bytes >= need)
			return LW_OK;
		release();
		HIP_TRY(hipMalloc(&p, need));
		bytes = need;
		return LW_OK;
	}
	void release()
	{
		if (p)
			(void)hipFree(p);
		p = nullptr;
		bytes = 0;
	}
};

// the commit of a slot (above): armed from its construction, which is the moment before the upload is queued
class LwStageGuard {
	hipEvent_t done;
	bool &pending;
	unsigned &next;
	hipStream_t st;
	bool armed = true;

public:
	LwStageGuard(hipEvent_t done, bool &pending, unsigned &next, hipStream_t st) : done(done), pending(pending), next(next), st(st) {}
	LwStageGuard(const LwStageGuard &) = delete;
	LwStageGuard &operator=(const LwStageGuard &) = delete;
	~LwStageGuard() { (void)commit(); }
	// the end of a call that queued everything; LW_ERR_DEVICE where the event could not be recorded
	int commit()
	{
		if (!armed)
			return LW_OK;
		armed = false;
		next = (next + 1) % LW_STAGE_SLOTS;
		if (lw_hip_ok(hipEventRecord(done, st), "hipEventRecord(staged records)")) {
			pending = true;
			return LW_OK;
		}
		(void)lw_hip_ok(hipStreamSynchronize(st), "hipStreamSynchronize(staged records)"); // nothing of the call is in flight after it
		return LW_ERR_DEVICE;
	}
};

template <class Rec> struct LwStageRing {
	struct Slot {
		Rec *h = nullptr, *d = nullptr; // pinned / device, cap records each
		size_t cap = 0;
		hipEvent_t done = nullptr; // recorded behind the last launch that read d, or scratch of this slot
		bool pending = false;
	};
	Slot slot[LW_STAGE_SLOTS];
	unsigned next = 0; // the slot of the call being made; device scratch "of the same rotation" is indexed by it

	bool create(const char *what)
	{
		bool ok = true;
		for (auto &s : slot)
			ok = ok && lw_hip_ok(hipEventCreateWithFlags(&s.done, hipEventDisableTiming), what);
		return ok;
	}
	void destroy() // (the device is idle: the caller has synchronised it)
	{
		for (auto &s : slot) {
			if (s.h)
				(void)hipHostFree(s.h);
			if (s.d)
				(void)hipFree(s.d);
			if (s.done)
				(void)hipEventDestroy(s.done);
			s = Slot{};
		}
	}
	int acquire(size_t n)
	{
		Slot &s = slot[next];
		if (s.pending) { // an earlier call's copy of these records, or its scratch, may still be in use
			HIP_TRY(hipEventSynchronize(s.done));
			s.pending = false;
		}
		if (s.cap < n) {
			if (s.h)
				(void)hipHostFree(s.h);
			if (s.d)
				(void)hipFree(s.d);
			s.h = s.d = nullptr;
			s.cap = 0;
			const size_t cap = std::max<size_t>(n, 64);
			HIP_TRY(hipHostMalloc((void **)&s.h, cap * sizeof(Rec), 0));
			HIP_TRY(hipMalloc((void **)&s.d, cap * sizeof(Rec)));
			s.cap = cap;
		}
		return LW_OK;
	}
	LwStageGuard guard(hipStream_t st)
	{
		Slot &s = slot[next];
		return LwStageGuard(s.done, s.pending, next, st);
	}
	int upload(const std::vector<Rec> &rows, hipStream_t st)
	{
		Slot &s = slot[next];
		std::memcpy(s.h, rows.data(), rows.size() * sizeof(Rec));
		HIP_TRY(hipMemcpyAsync(s.d, s.h, rows.size() * sizeof(Rec), hipMemcpyHostToDevice, st));
		return LW_OK;
	}
	const Rec *dev() const { return slot[next].d; } // what the launches behind the upload read (until the commit moves on)
};

// ---- the rows of a call, checked before anything is queued (a refused call has written nothing)

struct LwFillSpan {
	uint64_t most = 0, span = 0; // the largest n, the largest fill_end = max(n, fill_to)
};

// Rows that are normalised / finished / transformed in place of their own row: n[i] and fill_to[i] (0 without the array) against
// the capacity, then per_row(n, fill_end), which appends the row's record or refuses with a status; at the end the buffers
// that rows with elements need
template <class PerRow>
inline int lw_stage_fill_rows(size_t n_rows, const uint64_t *n, const uint64_t *fill_to, uint64_t capacity, const void *d_src, const void *d_dst,
		LwFillSpan &out, PerRow &&per_row)
{
	out = LwFillSpan{};
	for (size_t i = 0; i < n_rows; i++) {
		const uint64_t fill = fill_to ? fill_to[i] : 0;
		if (n[i] > capacity || fill > capacity)
			return LW_ERR_CAPACITY;
		const uint64_t fill_end = std::max(n[i], fill);
		if (int rc = per_row(n[i], fill_end))
			return rc;
		out.most = std::max(out.most, n[i]);
		out.span = std::max(out.span, fill_end);
	}
	if ((out.most && !d_src) || (out.span && !d_dst))
		return LW_ERR_NULL_ARG;
	return LW_OK;
}

// Rows that go from a source buffer into rows of another: len[i] against the source's capacity and the destination row
// (dst_row[i], or i without the array) against n_dst_rows, then per_row(len, row) as above; at the end no two source rows
// may have one destination row
template <class PerRow>
inline int lw_stage_mapped_rows(std::vector<uint64_t> &taken, size_t n_src_rows, const uint64_t *len, const uint32_t *dst_row, uint64_t src_capacity,
		uint64_t n_dst_rows, PerRow &&per_row)
{
	taken.clear();
	for (size_t i = 0; i < n_src_rows; i++) {
		const uint64_t row = dst_row ? dst_row[i] : i;
		if (len[i] > src_capacity || row >= n_dst_rows)
			return LW_ERR_CAPACITY;
		if (int rc = per_row(len[i], row))
			return rc;
		taken.push_back(row);
	}
	std::sort(taken.begin(), taken.end());
	if (std::adjacent_find(taken.begin(), taken.end()) != taken.end())
		return LW_ERR_CAPACITY;
	return LW_OK;
}
