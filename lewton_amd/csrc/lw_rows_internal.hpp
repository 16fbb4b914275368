// struct lw_rows, shared by the two translation units that work on it: lw_rows.cpp (create, destroy, lw_rows_synth) and
// lw_rows_mix.cpp (lw_rows_synth_mix).  lw_rows.cpp references nothing that lw_rows_mix.cpp defines.
#pragma once
#include "lw_stage.hpp"

#define LW_ROWS_SLOTS LW_STAGE_SLOTS // descriptor arrays in rotation (lw_stage.hpp), sized once: at create, and at the first mix use

struct lw_rows_slot {
	LwRowSeg *h_seg = nullptr, *d_seg = nullptr; // pinned / device, seg_cap descriptors each
	hipEvent_t done = nullptr;                  // recorded behind the k_rows launch that read them
	bool pending = false;
};

// lw_rows_synth_mix's counterpart: the call's pieces with its matrix behind them, in one upload
struct lw_rows_mix_slot {
	void *h = nullptr, *d = nullptr; // pinned / device: room for the pieces of max_packets packets and a matrix
	hipEvent_t done = nullptr;       // recorded behind the k_rows_mix launch that read them
	bool pending = false;
};

struct lw_rows {
	lw_decoder *dec = nullptr;
	size_t max_packets = 0;
	int fmt = 0;
	void *d_stage = nullptr; // the batch's packet-major PCM
	size_t stage_elems = 0;
	size_t seg_cap = 0;
	lw_rows_slot slot[LW_ROWS_SLOTS];
	unsigned next = 0;
	lw_rows_mix_slot mix[LW_ROWS_SLOTS];
	unsigned mix_next = 0;
	hipEvent_t last_done = nullptr; // behind the most recent launch of either kind: the staging buffer is its until then
	void *last_stream = nullptr;
	std::vector<LwRowSeg> plan; // the call's pieces, complete before anything is queued
	std::vector<LwRowMixPiece> mix_plan;
	size_t last_segments = 0;
	uint64_t last_copied = 0;
};
