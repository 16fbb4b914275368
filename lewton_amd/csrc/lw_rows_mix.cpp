// Stream-major rows through a channel matrix (lw_rows_synth_mix, include/lewton_amd.h "stream-major rows"): lw_rows_synth with
// out_ch output channels per row, each folded from the decoder's channels by a small matrix (select, reorder, downmix) in the
// assembling kernel itself (k_rows_mix, lw_kernels_rows_mix.hip).  As in lw_rows.cpp everything is decided here on the host, from
// lw_batch_results, before anything is queued: the refusals, which samples of which packet go where, and the cut into pieces.
// A piece is a time range of ONE packet with all its channels (LwRowMixPiece), at most LW_ROWS_MIX_PIECE positions; the first
// piece of a packet ends on a 16-byte boundary of the destination's channel 0, so the later ones start on one.
// The matrix travels behind the call's pieces in the same upload, so calls with different matrices may be queued back to back.
// lw_rows.cpp and the rest of the library reference nothing defined here.
#include "lw_rows_internal.hpp"

#include <algorithm>
#include <cstring>

static_assert(LW_ROWS_MIX_OUT == LW_ROWS_MIX_MAX_OUT, "the kernel's accumulators and the public bound are one number");

// every row holds at most one non-zero coefficient, and that one is 1.0: the output channels are copies of input channels or silence
static bool is_routing(const lw_row_mix *mix)
{
	for (size_t o = 0; o < mix->out_ch; o++) {
		size_t taken = 0;
		for (size_t c = 0; c < mix->in_ch; c++) {
			const float k = mix->coef[o * mix->in_ch + c];
			if (k == 0.0f)
				continue;
			if (!(k == 1.0f) || ++taken > 1)
				return false;
		}
	}
	return true;
}

extern "C" int lw_rows_synth_mix(lw_rows *r, lw_batch *b, const lw_row_place *place, size_t n, const lw_row_mix *mix, void *d_rows,
		size_t n_rows, size_t row_capacity, void *hip_stream)
{
	if (!r || !b || (!place && n) || !mix || !mix->coef)
		return LW_ERR_NULL_ARG;
	if (b->dec != r->dec || b->fmt != r->fmt)
		return LW_ERR_STATE_MISMATCH;
	const size_t ch = r->dec->T.ch, es = lw_elem_size(r->fmt);
	if (mix->in_ch != ch)
		return LW_ERR_STATE_MISMATCH;
	if (n != lw_batch_size(b) || n > r->max_packets || mix->out_ch == 0 || mix->out_ch > LW_ROWS_MIX_MAX_OUT)
		return LW_ERR_CAPACITY;
	const size_t out_ch = mix->out_ch;
	if (es == 2 && !is_routing(mix))
		return LW_ERR_UNSUPPORTED; // the i16 formats route only: nobody wants quantised samples mixed
	const bool itl = lw_fmt_interleaved(r->fmt);
	const size_t out_elems = lw_batch_out_elems(b);
	if (!lw_rows_bytes_ok(out_ch, row_capacity, n_rows, es) || out_elems > UINT32_MAX)
		return LW_ERR_CAPACITY;
	// ---- plan: every packet is checked and cut before anything is queued, so a refused call has written nothing
	const lw_packet_result *res = lw_batch_results(b);
	r->mix_plan.clear();
	uint64_t copied = 0;
	const uint64_t align = 16 / es; // positions of one channel per 16 bytes
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
		// per sample position: source elements, destination elements; channel 0 of the first kept position
		const uint64_t s_step = itl ? ch : 1, d_step = itl ? out_ch : 1;
		uint64_t src = res[i].out_offset + (uint64_t)p.skip * s_step;
		uint64_t dst = itl ? ((uint64_t)p.row * row_capacity + p.t0) * out_ch : (uint64_t)p.row * out_ch * row_capacity + p.t0;
		uint64_t count = kept, first = LW_ROWS_MIX_PIECE - (dst / d_step) % align;
		while (count) {
			const uint64_t c = std::min<uint64_t>(count, first);
			r->mix_plan.push_back(LwRowMixPiece{(uint32_t)src, (uint32_t)(itl ? 1 : m), (uint32_t)c, 0, dst});
			src += c * s_step, dst += c * d_step, count -= c;
			first = LW_ROWS_MIX_PIECE;
		}
		copied += kept * out_ch;
	}
	const size_t half1 = r->dec->T.state_chan_stride; // a packet yields at most this many samples per channel
	const size_t piece_cap = r->max_packets * (half1 / LW_ROWS_MIX_PIECE + 2);
	const size_t n_pieces = r->mix_plan.size(), coef_bytes = out_ch * ch * sizeof(float);
	if (n_pieces > piece_cap || n_pieces > UINT32_MAX)
		return LW_ERR_CAPACITY;
	if (n_pieces && !d_rows)
		return LW_ERR_NULL_ARG;
	// ---- queue: synthesis into the staging buffer, the pieces and the matrix, k_rows_mix
	if (int rc = lw_decoder_set_device(r->dec))
		return rc;
	hipStream_t st = (hipStream_t)hip_stream;
	lw_rows_mix_slot &s = r->mix[r->mix_next];
	if (n_pieces && !s.done) { // first use of this slot: room for any call this object accepts
		const size_t bytes = piece_cap * sizeof(LwRowMixPiece) + LW_ROWS_MIX_MAX_OUT * ch * sizeof(float);
		if (!s.h)
			HIP_TRY(hipHostMalloc(&s.h, bytes, 0));
		if (!s.d)
			HIP_TRY(hipMalloc(&s.d, bytes));
		HIP_TRY(hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
	}
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
	r->last_segments = n_pieces;
	r->last_copied = copied;
	if (n_pieces == 0)
		return LW_OK;
	if (s.pending) { // an earlier call's copy of this slot may still be on its way
		HIP_TRY(hipEventSynchronize(s.done));
		s.pending = false;
	}
	const size_t piece_bytes = n_pieces * sizeof(LwRowMixPiece);
	std::memcpy(s.h, r->mix_plan.data(), piece_bytes);
	std::memcpy((uint8_t *)s.h + piece_bytes, mix->coef, coef_bytes);
	LwStageGuard staged(s.done, s.pending, r->mix_next, st); // (lw_stage.hpp: a failed launch leaves the slot marked as well)
	r->last_done = s.done;
	r->last_stream = hip_stream;
	HIP_TRY(hipMemcpyAsync(s.d, s.h, piece_bytes + coef_bytes, hipMemcpyHostToDevice, st));
	HIP_TRY(lw_launch_rows_mix(r->d_stage, d_rows, (const LwRowMixPiece *)s.d, (uint32_t)n_pieces, (const float *)((const uint8_t *)s.d + piece_bytes),
			(uint32_t)ch, (uint32_t)out_ch, (uint64_t)row_capacity, (int)es, itl, st));
	return staged.commit();
}
