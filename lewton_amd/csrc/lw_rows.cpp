// Stream-major rows (lw_rows_*, include/lewton_amd.h "stream-major rows"): a batch's packet-major PCM assembled into
// [row][channel][sample] / [row][sample][channel] device buffers.  lw_batch_synth writes the batch's blocks into a staging
// buffer this object owns, and k_rows (lw_kernels_rows.hip) scatters them behind it on the same HIP stream.  Everything is
// decided here on the host, from lw_batch_results, before anything is launched: which samples of which packet go where
// (a leading skip as in skip_samples_linear, inside_ogg.rs:244-283; the last packet's trim, inside_ogg.rs:219-227), the
// refusals, and the cut of segments into pieces of at most LW_ROWS_PIECE elements.
// Built on the public batch calls; no other source of the library calls into this one.
#include "lw_rows_internal.hpp"

#include <algorithm>
#include <cstring>

// pieces one packet can be cut into: a first piece up to the destination's 16-byte boundary, whole pieces, a rest -- per
// channel for the planar formats, once for the interleaved ones
static size_t max_pieces_per_packet(const lw_decoder *d)
{
	const size_t ch = d->T.ch, half1 = d->T.state_chan_stride;
	return ch * (half1 / LW_ROWS_PIECE + 2) + 2;
}

extern "C" {

lw_rows *lw_rows_create(lw_decoder *d, size_t max_packets, int fmt, int *err)
{
	int dummy;
	if (!err)
		err = &dummy;
	*err = LW_OK;
	if (!d || max_packets == 0 || !lw_fmt_valid(fmt)) {
		*err = LW_ERR_NULL_ARG;
		return nullptr;
	}
	if (max_packets > lw_batch_max_packets(d)) { // no batch of the decoder is that large (before anything is allocated)
		*err = LW_ERR_CAPACITY;
		return nullptr;
	}
	if (lw_decoder_set_device(d)) {
		*err = LW_ERR_DEVICE;
		return nullptr;
	}
	auto r = std::make_unique<lw_rows>();
	r->dec = d;
	r->max_packets = max_packets;
	r->fmt = fmt;
	r->stage_elems = max_packets * d->T.ch * d->T.state_chan_stride; // a packet yields at most n1 / 2 samples per channel
	r->seg_cap = max_packets * max_pieces_per_packet(d);
	bool ok = lw_hip_ok(hipMalloc(&r->d_stage, r->stage_elems * lw_elem_size(fmt)), "hipMalloc(rows staging PCM)");
	for (auto &s : r->slot) {
		ok = ok && lw_hip_ok(hipHostMalloc((void **)&s.h_seg, r->seg_cap * sizeof(LwRowSeg), 0), "hipHostMalloc(row segments)") &&
			lw_hip_ok(hipMalloc((void **)&s.d_seg, r->seg_cap * sizeof(LwRowSeg)), "hipMalloc(row segments)") &&
			lw_hip_ok(hipEventCreateWithFlags(&s.done, hipEventDisableTiming), "hipEventCreate(row segments)");
	}
	if (!ok) {
		*err = LW_ERR_DEVICE;
		lw_rows_destroy(r.release());
		return nullptr;
	}
	return r.release();
}

void lw_rows_destroy(lw_rows *r)
{
	if (!r)
		return;
	(void)hipSetDevice(r->dec->device);
	(void)hipDeviceSynchronize();
	for (auto &s : r->slot) {
		if (s.h_seg)
			(void)hipHostFree(s.h_seg);
		if (s.d_seg)
			(void)hipFree(s.d_seg);
		if (s.done)
			(void)hipEventDestroy(s.done);
	}
	for (auto &s : r->mix) { // (made by lw_rows_synth_mix, lw_rows_mix.cpp, on first use)
		if (s.h)
			(void)hipHostFree(s.h);
		if (s.d)
			(void)hipFree(s.d);
		if (s.done)
			(void)hipEventDestroy(s.done);
	}
	if (r->d_stage)
		(void)hipFree(r->d_stage);
	delete r;
}

int lw_rows_synth(lw_rows *r, lw_batch *b, const lw_row_place *place, size_t n, void *d_rows, size_t n_rows, size_t row_capacity,
		void *hip_stream)
{
	if (!r || !b || (!place && n))
		return LW_ERR_NULL_ARG;
	if (b->dec != r->dec || b->fmt != r->fmt)
		return LW_ERR_STATE_MISMATCH;
	if (n != lw_batch_size(b) || n > r->max_packets)
		return LW_ERR_CAPACITY;
	const size_t ch = r->dec->T.ch, es = lw_elem_size(r->fmt);
	const bool itl = lw_fmt_interleaved(r->fmt);
	const size_t out_elems = lw_batch_out_elems(b);
	if (!lw_rows_bytes_ok(ch, row_capacity, n_rows, es) || out_elems > UINT32_MAX)
		return LW_ERR_CAPACITY;
	// ---- plan: every packet is checked and cut before anything is queued, so a refused call has written nothing
	const lw_packet_result *res = lw_batch_results(b);
	r->plan.clear();
	uint64_t copied = 0;
	const size_t align_elems = 16 / es;
	auto cut = [&](uint64_t src, uint64_t dst, uint64_t count) {
		// the first piece ends on a 16-byte boundary of the destination (for a 16-byte aligned buffer), so the later ones start on one
		uint64_t first = LW_ROWS_PIECE - dst % align_elems;
		while (count) {
			const uint64_t c = std::min<uint64_t>(count, first);
			r->plan.push_back(LwRowSeg{(uint32_t)src, (uint32_t)c, dst});
			src += c, dst += c, count -= c;
			first = LW_ROWS_PIECE;
		}
	};
	for (size_t i = 0; i < n; i++) {
		const lw_row_place &p = place[i];
		if (p.row >= n_rows)
			return LW_ERR_CAPACITY;
		if (res[i].status != LW_OK || res[i].n_samples == 0 || p.skip >= res[i].n_samples)
			continue;
		const uint64_t m = res[i].n_samples, kept = std::min<uint64_t>(p.keep, m - p.skip);
		if (p.t0 > row_capacity || kept > row_capacity - p.t0)
			return LW_ERR_CAPACITY;
		if (kept == 0)
			continue;
		if (res[i].out_offset + m * ch > out_elems)
			return LW_ERR_CAPACITY; // (results that do not belong to this batch's PCM: never from lw_batch_entropy)
		if (itl) {
			cut(res[i].out_offset + (uint64_t)p.skip * ch, ((uint64_t)p.row * row_capacity + p.t0) * ch, kept * ch);
		} else {
			for (size_t c = 0; c < ch; c++)
				cut(res[i].out_offset + c * m + p.skip, ((uint64_t)p.row * ch + c) * row_capacity + p.t0, kept);
		}
		copied += kept * ch;
	}
	if (r->plan.size() > r->seg_cap || r->plan.size() > UINT32_MAX)
		return LW_ERR_CAPACITY;
	if (!r->plan.empty() && !d_rows)
		return LW_ERR_NULL_ARG;
	// ---- queue: synthesis into the staging buffer, the descriptors, k_rows
	if (int rc = lw_decoder_set_device(r->dec))
		return rc;
	hipStream_t st = (hipStream_t)hip_stream;
	if (r->last_done && r->last_stream != hip_stream) // another stream than last time: the staging buffer is still that call's
		HIP_TRY(hipStreamWaitEvent(st, r->last_done, 0));
	if (out_elems > r->stage_elems) {
		HIP_TRY(hipDeviceSynchronize());
		(void)hipFree(r->d_stage);
		r->d_stage = nullptr;
		r->stage_elems = 0;
		HIP_TRY(hipMalloc(&r->d_stage, out_elems * es));
		r->stage_elems = out_elems;
	}
	if (int rc = lw_batch_synth(b, r->d_stage, r->stage_elems, hip_stream))
		return rc;
	r->last_segments = r->plan.size();
	r->last_copied = copied;
	if (r->plan.empty())
		return LW_OK;
	lw_rows_slot &s = r->slot[r->next];
	if (s.pending) { // an earlier call's copy of these descriptors may still be on its way
		HIP_TRY(hipEventSynchronize(s.done));
		s.pending = false;
	}
	std::memcpy(s.h_seg, r->plan.data(), r->plan.size() * sizeof(LwRowSeg));
	LwStageGuard staged(s.done, s.pending, r->next, st); // (lw_stage.hpp: a failed launch leaves the slot marked as well)
	r->last_done = s.done;
	r->last_stream = hip_stream;
	HIP_TRY(hipMemcpyAsync(s.d_seg, s.h_seg, r->plan.size() * sizeof(LwRowSeg), hipMemcpyHostToDevice, st));
	HIP_TRY(lw_launch_rows(r->d_stage, d_rows, s.d_seg, (uint32_t)r->plan.size(), (int)es, st));
	return staged.commit();
}

size_t lw_rows_last_segments(const lw_rows *r)
{
	return r ? r->last_segments : 0;
}

uint64_t lw_rows_last_copied_elems(const lw_rows *r)
{
	return r ? r->last_copied : 0;
}

} // extern "C"
