/*
 * lewton_amd.h -- C ABI of the MI355X-native Vorbis audio-packet decode path.
 *
 * This is the drop-in boundary for lewton's `audio` module (src/audio.rs + src/imdct.rs +
 * src/samples.rs, fed by src/header.rs): a Rust/C/Python host binds exactly these symbols
 * (see INTEGRATION.md for the `extern "C"` block a lewton maintainer would add).  Plain pointers
 * and sizes only; no C++/torch types.  All functions are `noexcept` in effect: errors are status
 * codes, nothing unwinds across the boundary.
 *
 * Split of work: the bit-serial entropy stage (packet prologue, floor decode,
 * residue Huffman/VQ decode; audio.rs:921-986) runs on the host inside this library; everything from
 * the residue vectors onward (inverse coupling, floor-1 curve, floor x residue, IMDCT,
 * window/overlap-add, sample conversion; audio.rs:990-1157, imdct.rs:291-659, samples.rs:32-103)
 * runs in hand-written HIP kernels for gfx950.  There is no CPU fallback for the device stage:
 * calls fail with LW_ERR_DEVICE when no GPU is usable.
 *
 * Paths cited below are relative to the reference tree (RustAudio/lewton 0.10.2).
 */
#ifndef LEWTON_AMD_H
#define LEWTON_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ------------------------------------------------------------------------- */
enum {
	LW_OK = 0,
	/* AudioReadError, src/audio.rs:26-41 */
	LW_AUDIO_END_OF_PACKET = 1,
	LW_AUDIO_BAD_FORMAT = 2,
	LW_AUDIO_IS_HEADER = 3,
	LW_AUDIO_BUFFER_NOT_ADDRESSABLE = 4,
	/* HeaderReadError, src/header.rs:35-63 */
	LW_HDR_END_OF_PACKET = 16,
	LW_HDR_NOT_VORBIS = 17,
	LW_HDR_UNSUPPORTED_VERSION = 18,
	LW_HDR_BAD_FORMAT = 19,
	LW_HDR_BAD_TYPE = 20,
	LW_HDR_IS_AUDIO = 21,
	LW_HDR_UTF8 = 22,
	LW_HDR_BUFFER_NOT_ADDRESSABLE = 23,
	/* errors of this library (no counterpart in the reference) */
	LW_ERR_NULL_ARG = 32,      /* like capi.rs:106-108 returning 1; a packet given as (NULL, 0) is not an error but an empty packet */
	LW_ERR_DEVICE = 33,        /* HIP error / no GPU; lw_last_device_error() has the text */
	LW_ERR_CAPACITY = 34,      /* caller-provided buffer or batch too small */
	LW_ERR_STATE_MISMATCH = 35, /* pwr belongs to another decoder (the reference panics, audio.rs:1086) */
	LW_ERR_UNSUPPORTED = 36     /* an optional mode is not available for this stream (see the function's comment) */
};

/* Output sample formats = the `Samples` implementations of src/samples.rs */
enum {
	LW_FMT_I16_PLANAR = 0,      /* Vec<Vec<i16>>: per packet [ch][m]          (samples.rs:20-40, :92-103) */
	LW_FMT_I16_INTERLEAVED = 1, /* InterleavedSamples<i16>: per packet [m][ch] (samples.rs:48-78) */
	LW_FMT_F32_PLANAR = 2,      /* Vec<Vec<f32>>: per packet [ch][m]          (samples.rs:86-90; capi.rs:110) */
	LW_FMT_F32_INTERLEAVED = 3  /* InterleavedSamples<f32>: per packet [m][ch] (samples.rs:48-78, :86-90) */
};

typedef struct lw_ident lw_ident;     /* IdentHeader incl. cached_bs_derived, src/header.rs:188-211 */
typedef struct lw_setup lw_setup;     /* SetupHeader, src/header.rs:471-481 */
typedef struct lw_comment lw_comment; /* CommentHeader, src/header.rs:289-300 */
typedef struct lw_decoder lw_decoder; /* device context: tables of one (ident, setup) pair on one GPU */
typedef struct lw_pwr lw_pwr;         /* PreviousWindowRight, src/audio.rs:847-861 (device resident) */
typedef struct lw_batch lw_batch;     /* pinned staging + device buffers for a batch of packets */

/* ---- headers (host) ----------------------------------------------------------------------- */
typedef struct {
	uint8_t audio_channels;
	uint32_t audio_sample_rate;
	int32_t bitrate_maximum, bitrate_nominal, bitrate_minimum;
	uint8_t blocksize_0, blocksize_1;
} lw_ident_info;

/* read_header_ident, src/header.rs:221-259.  NULL + *err on failure. */
lw_ident *lw_read_header_ident(const uint8_t *packet, size_t len, int *err);
int lw_ident_get_info(const lw_ident *id, lw_ident_info *out);
void lw_ident_free(lw_ident *id);
/* read_header_setup, src/header.rs:1082-1154 */
lw_setup *lw_read_header_setup(const uint8_t *packet, size_t len, uint8_t audio_channels,
		uint8_t blocksize_0, uint8_t blocksize_1, int *err);
void lw_setup_free(lw_setup *s);
/* read_header_comment, src/header.rs:309-355 */
lw_comment *lw_read_header_comment(const uint8_t *packet, size_t len, int *err);
const char *lw_comment_vendor(const lw_comment *c, size_t *len);
size_t lw_comment_count(const lw_comment *c);
int lw_comment_get(const lw_comment *c, size_t i, const char **key, size_t *key_len, const char **val, size_t *val_len);
void lw_comment_free(lw_comment *c);

/* ---- device context ----------------------------------------------------------------------- */
int lw_device_count(void);
/* Uploads the per-blocksize tables (header_cached.rs:34-110, computed on the host with libm exactly
 * like the reference), floor-1 post tables, the inverse-dB table and the mapping/coupling lists. */
lw_decoder *lw_decoder_create(const lw_ident *id, const lw_setup *s, int device, int *err);
void lw_decoder_destroy(lw_decoder *d);
const char *lw_last_device_error(void);

/* ---- PreviousWindowRight (src/audio.rs:847-861) ------------------------------------------- */
/* A handle is a slot of the decoder's state pool, [slot][2 parities][ch][n1 / 2] floats on the device, and three host fields:
 * whether a right part is stored, its length, and which of the slot's two buffers holds it (lw_pwr_state below).  Planning a batch
 * (lw_batch_entropy, lw_ring_stage) advances the host fields at once; the device buffers follow when that batch is launched, and a
 * launch reads one buffer of a slot and writes the OTHER.  Between the two the host fields are AHEAD of the device.  What each call
 * keeps (tests/test_gpu_stream_state.py pins these on every synthesis kernel family):
 *   lw_pwr_clone         copies both buffers of the slot after a device synchronisation, and the host fields as they are.  Batches of
 *                        the stream that were launched need not be collected; a batch that is planned and NOT yet launched makes the
 *                        twin wrong: its host fields name a buffer that batch has still to write.  Launch first, then clone.  Takes a
 *                        slot like lw_pwr_new (below), so it can move the pool.
 *   lw_pwr_copy_to_host  the same condition: it synchronises the device and reads the buffer the host fields name.  Does not move the
 *                        pool, but reads its address: not next to a lw_pwr_new / lw_decoder_reserve_streams on another thread.
 *   lw_pwr_reset         host fields only.  Batches planned before it, launched or not, decode as planned (their records carry slot and
 *                        buffer); the next batch planned for the stream starts from no previous window.  Nothing has to be finished.
 *   lw_pwr_free          host only: the slot goes on top of the decoder's free list and the next lw_pwr_new / lw_pwr_clone takes it
 *                        (most recently freed first).  Batches of the stream still planned or in flight need not be finished, PROVIDED
 *                        the slot's next stream is launched behind them: one ring launches in the order it staged (lw_ring_launch), so
 *                        freeing straight after lw_ring_submit and reusing the slot in that ring's next batches is sound.  Two rings (or
 *                        two HIP streams) of one decoder are NOT ordered against each other: collect the freed stream's last batch
 *                        before a stream of the other ring can take its slot.  The handle itself is gone at once: it must not appear
 *                        in a later lw_packet.
 *   lw_pwr_new, lw_decoder_reserve_streams   the pool MOVES when it grows (64 slots at first, doubled by lw_pwr_new, exactly n by
 *                        lw_decoder_reserve_streams): device synchronisation, allocation, copy of every slot's two buffers, free.
 *                        Everything launched before the call is finished by the synchronisation and every live state arrives in the
 *                        new pool; batches planned and not yet launched are unaffected (a launch reads the pool's address when it is
 *                        issued).  But a launch call reads that address without the decoder's lock: lw_pwr_new, lw_pwr_clone and
 *                        lw_decoder_reserve_streams must not run while ANOTHER thread is inside lw_batch_synth* / lw_ring_launch /
 *                        lw_ring_submit of the same decoder -- a ring's stage thread that opens streams next to its launch thread
 *                        reserves its slots first (lw_decoder_reserve_streams).  lw_sharder_stream_open between lw_sharder_submit and
 *                        the collect is sound: submit returns once the call's launches are issued (tests/test_host_shard.py).
 * None of these calls is synchronised against lw_batch_entropy / lw_ring_stage of a batch that names the same handle. */
lw_pwr *lw_pwr_new(lw_decoder *d);         /* PreviousWindowRight::new */
int lw_pwr_is_empty(const lw_pwr *p);      /* ::is_empty */
lw_pwr *lw_pwr_clone(const lw_pwr *p);     /* #[derive(Clone)] (device copy) */
void lw_pwr_reset(lw_pwr *p);              /* `pwr = PreviousWindowRight::new()`, inside_ogg.rs:307-313 */
void lw_pwr_free(lw_pwr *p);
size_t lw_pwr_len(const lw_pwr *p);        /* per-channel length of the stored right part */
int lw_pwr_copy_to_host(const lw_pwr *p, float *dst /* [ch][len] */);
/* Grows the decoder's state pool to exactly `n` stream slots in ONE allocation (lw_pwr_new doubles the pool when it runs
 * out: a device synchronisation and a device-to-device copy of the whole pool each time).  A no-op when the pool already
 * holds `n` slots; LW_ERR_CAPACITY past the slot limit (see "Limits" below), LW_ERR_DEVICE when the device has no room.
 * From a fresh pool lw_pwr_new hands the slots out in ascending order. */
int lw_decoder_reserve_streams(lw_decoder *d, size_t n);
int lw_debug_pwr_slot(const lw_pwr *p);    /* the state-pool slot of a handle (tests) */

/* ---- one packet (drop-in for audio.rs) ---------------------------------------------------- */
/* get_decoded_sample_count, src/audio.rs:874-909 (header bits only, host only) */
int lw_get_decoded_sample_count(const lw_ident *id, const lw_setup *s, const uint8_t *packet, size_t len,
		size_t *count);
/* read_audio_packet_generic<S>, src/audio.rs:919-1160 (read_audio_packet :1170 is fmt = LW_FMT_I16_PLANAR).
 * `out` is host memory for ch * cap samples; *n_samples = per-channel sample count (0 for the first
 * packet after a reset, audio.rs:1140-1152).  Synchronous: entropy decode, H2D, kernels, D2H. */
int lw_read_audio_packet(lw_decoder *d, const uint8_t *packet, size_t len, lw_pwr *pwr, int fmt,
		void *out, size_t cap_per_channel, size_t *n_samples);

/* ---- host entropy stage on its own (no GPU needed) ---------------------------------------- */
/* The bit-serial half of read_audio_packet_generic (audio.rs:921-986 + floor-1 amplitude unwrap
 * :391-435): decodes one packet into the GPU-stage record.  floor_out: [ch][lw_setup_floor_stride()] u16
 * (ascending-x order; bits 0-7 = final_y*multiplier, bit 15 = active, entry 0 == 0xFFFF = unused floor, entry 0 ==
 * 0xFFFE = floor 0: the curve of audio.rs:160-212 is in floor_curve_out [ch][n/2] f32, which may be NULL for setups
 * without a floor of type 0); residue_out: [ch][n/2] f32 before inverse coupling.  *blocksize_log2, *mode and *flags (bit 0 long, bit 1
 * prev window flag, bit 2 next window flag) describe the packet; *bits_consumed = position of the bit
 * cursor afterwards. */
uint32_t lw_setup_floor_stride(const lw_setup *s);
int lw_entropy_decode_host(const lw_ident *id, const lw_setup *s, const uint8_t *packet, size_t len,
		uint16_t *floor_out, float *residue_out, size_t residue_cap_floats, uint8_t *blocksize_log2, uint8_t *mode,
		uint8_t *flags, uint64_t *bits_consumed, float *floor_curve_out);

/* Introspection for tests and tools: the dense VQ table of a codebook (header.rs:495-531; entries x dims floats,
 * dst may be NULL to query the sizes; returns LW_ERR_UNSUPPORTED for a book without a lookup table). */
int lw_setup_codebook_vq(const lw_setup *s, unsigned book, float *dst, size_t cap_floats, uint32_t *dims, uint32_t *entries);

/* ---- batches ------------------------------------------------------------------------------ */
typedef struct {
	const uint8_t *data;
	size_t len;
	lw_pwr *pwr; /* packets sharing a pwr must be listed in stream order */
} lw_packet;

typedef struct {
	int32_t status;      /* LW_OK or an AudioReadError code; failed packets produce no samples */
	uint32_t n_samples;  /* per channel */
	uint64_t out_offset; /* element offset of this packet's block in the output buffer */
} lw_packet_result;

/* Tap points = the reference's record_*! macros (src/lib.rs:56-94; audio.rs:988,1004,1041,1054) */
enum { LW_TAP_RESIDUE_PRE_INVERSE = 0, LW_TAP_RESIDUE_POST_INVERSE = 1, LW_TAP_PRE_MDCT = 2, LW_TAP_POST_MDCT = 3 };

lw_batch *lw_batch_create(lw_decoder *d, size_t max_packets, int fmt, int *err);
/* The largest max_packets lw_batch_create (and with it lw_ring_create, lw_sharder_create per shard, lw_rows_create and the Ogg
 * stream's read-ahead) accepts for this decoder; a larger one is refused with LW_ERR_CAPACITY before anything is allocated.
 * See "Limits" below. */
size_t lw_batch_max_packets(const lw_decoder *d);
/* ---- Limits ---------------------------------------------------------------------------------
 * Two sizes are bounded by 32-bit fields of the records the kernels read; both are refused with LW_ERR_CAPACITY before
 * anything is allocated, never truncated ("every failure is a status, never wrong samples").
 *
 * Packets per batch.  The records carry per-batch offsets in 32 bits.  With ch channels, block sizes n0 <= n1 and a floor
 * stride of lw_setup_floor_stride() entries, a batch of n packets needs (every packet a long block, the worst case)
 *     n * ch * n1                   floats of time-domain scratch      (2 res_off + c n1 + i; the tightest)
 *     n * ch * (3 n1 - n0) / 4      output elements                    (lw_decoder_max_block_elems per packet)
 *     n * ch * floor stride         floor entries
 *     n * 2 * ch * n0 / 4           raw edge values                    (n0 = 256 or 512: the block sizes with an edge form)
 *     n * 3                         padding words of the device entropy stage's packet pool
 * to be at most 2^32 each, so lw_batch_max_packets = 2^32 / (ch * n1) for every setup in use: 1 048 576 packets for stereo
 * 256/2048, 349 525 for 5.1.  With the entropy stage on the device the packets' own bytes count as well: a batch whose
 * packets, each rounded up to 32-bit words plus three, exceed 2^32 words fails in lw_batch_entropy / lw_ring_stage with
 * LW_ERR_CAPACITY.
 *
 * Streams per decoder.  A state-pool slot travels as int and as int32_t prev = -(slot + 2): slots are 0 .. 2^31 - 2, so
 * lw_decoder_reserve_streams(d, n) and the growth behind lw_pwr_new refuse n > 2^31 - 1 (lw_pwr_new then returns NULL, as on
 * any failed growth).  The pool itself is addressed in size_t by every kernel: its size, 2 * ch * n1 / 2 floats per slot, is
 * bounded by device memory only (2^20 stereo 256/2048 streams are 16 GiB). */
void lw_batch_destroy(lw_batch *b);
/* Host entropy stage for `n` packets on `n_threads` host threads (0 = lw_default_host_threads()): fills the
 * pinned staging buffers with GPU-stage records and decides sample counts, window geometry and error
 * statuses (all host-decidable).  Advances the host-side bookkeeping of every pwr. */
int lw_batch_entropy(lw_batch *b, const lw_packet *pkts, size_t n, int n_threads);
/* hipMemcpyAsync of the staged records to the device (stream = hipStream_t, NULL = default stream) */
int lw_batch_upload(lw_batch *b, void *hip_stream);
/* Launch the synthesis kernels on `hip_stream`; d_out = DEVICE pointer to lw_batch_out_elems() elements
 * of the batch's format.  Asynchronous.  Re-launching the same uploaded batch is idempotent. */
int lw_batch_synth(lw_batch *b, void *d_out, size_t out_capacity_elems, void *hip_stream);
/* Convenience: synth into an internal device buffer, copy to host memory, synchronise. */
int lw_batch_synth_to_host(lw_batch *b, void *h_out, size_t out_capacity_elems, void *hip_stream);
size_t lw_batch_size(const lw_batch *b);
size_t lw_batch_out_elems(const lw_batch *b);
const lw_packet_result *lw_batch_results(const lw_batch *b);
/* bytes the device stage reads+writes for this batch by the SURVEY 8(d) definition */
uint64_t lw_batch_algorithmic_bytes(const lw_batch *b);
/* bytes of PreviousWindowRight that have to cross HBM because of the launch boundary, NOT part of the 8(d) figure: the stored
 * right part of every stream whose first packet of the batch has one (read from the state pool) and the right part every
 * stream's last packet leaves behind (written to it), channels * length * 4 each.  Inside a launch the state passes through LDS. */
uint64_t lw_batch_state_bytes(const lw_batch *b);
/* Debug taps: copy one intermediate of packet `idx` to host after running the generic kernels.
 * dst: [ch][n/2] floats ([ch][n] for LW_TAP_POST_MDCT). */
int lw_batch_tap(lw_batch *b, size_t idx, int tap, float *dst, size_t cap_floats);
/* Force the generic (any block size / window shape) kernels even where a specialised one applies. */
void lw_batch_set_force_generic(lw_batch *b, int on);
/* Test hook: rounds per workgroup of the specialised long-block kernel for this batch's next lw_batch_entropy (1..16;
 * 0 = the planner decides).  Exercises the hand-over of window state across rounds and workgroups on small batches. */
void lw_debug_batch_set_rounds(lw_batch *b, int rounds);
/* Test hook: how the wave-pipeline kernels get the right half of a predecessor that is not the item in front (a chunk of the work
 * list that starts inside a stream): -1 (default) = the predecessor is recomputed inside the launch as an item of its own where
 * that pays, 0 = always by the pre-pass launch (k_long<halo>) */
void lw_debug_batch_set_halo(lw_batch *b, int mode);
/* test hook: 0 = never run a mixed short / long batch as one k_mix launch (two launches: k_long<EDGE>, k_short), -1 = where it applies */
void lw_debug_batch_set_mix(lw_batch *b, int mode);
/* test hook for blocksize_1 = 10 / 12 streams: -1 = k_long10 / k_long12 (long blocks next to short ones in their EDGE form where the
 * short blocks run through k_short<8 / 16>), 1 = k_long10 / k_long12 for the long blocks with two long slopes only (the others
 * through the generic kernels), 0 = the block kernels k_short<32> / k_big<12> instead */
void lw_debug_batch_set_long10(lw_batch *b, int mode);
/* Device-side failures of a batch's launches (audio.rs:27-41: every failure is a status, never wrong samples).  Call once the
 * work lw_batch_synth queued has COMPLETED (after synchronising its stream); lw_batch_synth_to_host and lw_ring_collect call it
 * themselves.  LW_OK, or LW_ERR_DEVICE: a kernel raised the batch's error word (k_mix: a short block's wave never saw the raw
 * edges its long neighbours' waves of the same launch were to write -- the grid was not resident at once, e.g. under a CU mask or
 * next to another process's kernels).  Then every packet's result carries LW_ERR_DEVICE with 0 samples, the PCM written by this
 * batch must not be used, and the window state of the batch's streams is undefined: reset their PreviousWindowRight (or restore
 * a snapshot, lw_pwr_snapshot) before decoding on.  The word and the launch's leftovers are cleared: the batch can run again. */
int lw_batch_device_status(lw_batch *b);
/* test hook: spin != 0 = the long blocks' waves of the next k_mix launches never signal their edges, and the short blocks' waves
 * give up after `spin` polls (lw_batch_device_status then reports LW_ERR_DEVICE); 0 = normal operation */
void lw_debug_batch_break_mix(lw_batch *b, unsigned spin);
/* ... and process-wide, for the batches a ring, a sharder or an Ogg stream reader owns: every batch launched while spin != 0 */
void lw_debug_break_mix(unsigned spin);
/* Entropy stage on the device (csrc/lw_dev_entropy.h, k_entropy): the bit-serial half of read_audio_packet_generic
 * (audio.rs:921-986: floor-1 decode :215-251 + amplitude unwrap :391-435, residue decode :587-760) runs on the GPU, one
 * wave per packet; lw_batch_entropy then only reads the prologues, copies the packets into pinned staging and plans the
 * batch, and the packets themselves (~0.5 KB instead of 8.3 KB of records per stereo long block) cross PCIe.  Records,
 * PCM and statuses are bit-identical to the host stage's.  Eligible streams: floor type 1, residue books with a vector
 * lookup of at most 64 dimensions, at most 16 channels and 16 coupling steps (`why` names the reason otherwise;
 * LW_ERR_UNSUPPORTED from the setters). */
int lw_decoder_supports_device_entropy(const lw_decoder *d, const char **why);
int lw_batch_set_entropy_on_device(lw_batch *b, int on);
/* Runs k_entropy for the records uploaded last (after lw_batch_upload, on the same stream), ahead of lw_batch_synth: the
 * entropy kernel touches no stream state, so a pipeline may queue it before it orders the synthesis kernels behind the
 * previous batch's (the staging ring does).  lw_batch_synth runs it itself when this was not called.  No-op in host mode. */
int lw_batch_device_entropy(lw_batch *b, void *hip_stream);
/* names of the kernels the last lw_batch_synth used, comma separated (introspection for tests/bench) */
const char *lw_batch_last_kernels(const lw_batch *b);

/* ---- stream-major rows ------------------------------------------------------------------------------------------------
 * Everything above hands PCM back packet-major: a batch's output is a run of per-packet blocks ([ch][m] or [m][ch], at
 * lw_packet_result.out_offset) in submission order, the packets of many streams mixed -- lewton's call shape (audio.rs:919).  A
 * caller that decodes many WHOLE streams and goes on working on the GPU wants each stream's waveform as one contiguous array that
 * stays there: d_rows = n_rows rows of ch * row_capacity elements in DEVICE memory,
 *   [row][ch][row_capacity] for the planar formats, [row][row_capacity][ch] for the interleaved ones.
 * lw_rows_synth = lw_batch_synth of `b` (entropy stage done and uploaded; same decoder and fmt as `r`) into a staging PCM buffer
 * that `r` owns, then one more kernel on the same stream (k_rows, a segmented copy) that moves, for packet i of the batch
 * (n == lw_batch_size(b)), the samples [skip, skip + kept) of every channel of its block to the positions [t0, t0 + kept) of row
 * place[i].row, kept = min(keep, n_samples - skip).  `skip` is the leading part a seek drops (skip_samples_linear,
 * inside_ogg.rs:244-283), `keep` the truncation of a stream's last packet to its final granule position (inside_ogg.rs:219-227);
 * the caller keeps the per-row cursor (inside_ogg.rs:209-229 is its bookkeeping for one stream).  A packet whose status is not
 * LW_OK, that has no samples (the first of a stream, audio.rs:1140-1152) or whose skip >= n_samples contributes nothing.
 * Only the destination ranges are written: padding and other rows keep what the caller put there.  Destinations of different
 * packets that overlap are the caller's business (the result is then one of them, unspecified which).
 * Everything is decided on the host from lw_batch_results BEFORE anything is queued, so a refused call has written nothing:
 *   LW_ERR_NULL_ARG        r or b NULL, place NULL with n > 0, d_rows NULL when anything would be copied
 *   LW_ERR_STATE_MISMATCH  b belongs to another decoder or has another fmt than r
 *   LW_ERR_CAPACITY        n != lw_batch_size(b), n > max_packets, a place with row >= n_rows (any packet) or
 *                          t0 + kept > row_capacity
 * Asynchronous, and idempotent like lw_batch_synth.  Calls on one object may be queued back to back without synchronising
 * (on another stream than the call before, the new call's work is ordered behind it).  Device errors: lw_batch_device_status(b)
 * keeps its contract -- after LW_ERR_DEVICE the row ranges the call wrote are void along with the batch's PCM.
 * All destination offsets are 64-bit: a rows buffer may hold more than 2^32 elements. */
typedef struct lw_rows lw_rows;
typedef struct {
	uint32_t row;   /* destination row */
	uint32_t skip;  /* samples per channel dropped from the front of this packet's block */
	uint32_t keep;  /* samples per channel kept behind skip; UINT32_MAX = all that remain */
	uint32_t pad_;
	uint64_t t0;    /* sample position in the row that receives the first kept sample */
} lw_row_place;
lw_rows *lw_rows_create(lw_decoder *d, size_t max_packets, int fmt, int *err);
void lw_rows_destroy(lw_rows *r);
int lw_rows_synth(lw_rows *r, lw_batch *b, const lw_row_place *place, size_t n, void *d_rows, size_t n_rows, size_t row_capacity,
		void *hip_stream);
/* introspection: the pieces (segments cut to at most 2048 elements, one GPU wave each) of the last call, and the elements they moved */
size_t lw_rows_last_segments(const lw_rows *r);
uint64_t lw_rows_last_copied_elems(const lw_rows *r);
/* lw_rows_synth through a channel matrix: select, reorder, downmix.  The rows buffer has mix->out_ch channels per row,
 *   [row][out_ch][row_capacity] for the planar formats, [row][row_capacity][out_ch] for the interleaved ones,
 * and destination sample t of output channel o is folded from the source samples x_c of the same packet position -- bit for bit:
 *   - the input channels c are taken in ascending order; every c whose coef[o][c] compares equal to 0 (either sign) is skipped;
 *   - a coefficient equal to 1.0f contributes x_c itself, with no multiply: a lone 1.0 is a bit copy, NaN payloads included;
 *   - any other coefficient contributes coef * x_c: one f32 multiply, rounded;
 *   - the first contribution is the accumulator, every later one is added with one rounded f32 add -- no fused multiply-add,
 *     no reassociation, subnormals are kept;
 *   - with no non-zero coefficient the result is +0.0 (i16 formats: 0).
 * Every destination position [t0, t0 + kept) of all out_ch channels is written, nothing else.
 * The f32 formats accept any matrix; the i16 formats accept routing matrices only (every row holds at most one non-zero
 * coefficient, and that one equals 1.0): mixing quantised samples is not what anybody wants.
 * Refusals, decided on the host before anything is queued like lw_rows_synth's, which all apply unchanged:
 *   LW_ERR_NULL_ARG        mix or mix->coef NULL
 *   LW_ERR_CAPACITY        out_ch == 0 or > LW_ROWS_MIX_MAX_OUT (t0 + kept > row_capacity as before)
 *   LW_ERR_STATE_MISMATCH  in_ch is not the decoder's channel count
 *   LW_ERR_UNSUPPORTED     a matrix that is not a routing matrix with an i16 format
 * The coefficients are copied during the call.  Calls with different matrices may be queued back to back on one lw_rows, and may
 * be mixed with lw_rows_synth calls.  lw_rows_last_copied_elems reports kept * out_ch summed over the call, lw_rows_last_segments
 * the pieces (time ranges of one packet with all its channels, at most 512 positions, one GPU wave each).  Idempotence, device
 * errors and 64-bit destination offsets as for lw_rows_synth. */
#define LW_ROWS_MIX_MAX_OUT 8
typedef struct {
	uint32_t out_ch;    /* channels of the rows buffer, 1..LW_ROWS_MIX_MAX_OUT */
	uint32_t in_ch;     /* must equal the decoder's channel count */
	const float *coef;  /* out_ch * in_ch host floats, coef[o * in_ch + c] */
} lw_row_mix;
int lw_rows_synth_mix(lw_rows *r, lw_batch *b, const lw_row_place *place, size_t n, const lw_row_mix *mix,
		void *d_rows, size_t n_rows, size_t row_capacity, void *hip_stream);

/* ---- resampling rows ---------------------------------------------------------------------------------------------------
 * Finished rows at one sample rate -> rows at another, on the GPU, as a pass of its own (k_resample): the synthesis kernels and
 * the assemblers above are not involved.  Source and destination are rows buffers of the two f32 formats, `ch` channels each,
 *   [row][ch][capacity] (LW_FMT_F32_PLANAR) or [row][capacity][ch] (LW_FMT_F32_INTERLEAVED),
 * with their own capacities.  The filter is a windowed sinc in polyphase form, and it is a contract on BITS:
 *
 * A resampler is made from (in_rate, out_rate, zeros, rolloff, window, beta).  g = gcd(in_rate, out_rate), orig = in_rate / g,
 * new = out_rate / g.
 *   s = rolloff * min(1, new / orig)      the cut-off as a fraction of the input Nyquist
 *   W = ceil(zeros / s)                   the half width in input samples
 *   K = 2 W + 2                           taps per phase; there are `new` phases
 * Tap k of phase ph, evaluated in double and rounded ONCE to f32:
 *   t = (k - W) - ph / new,  u = s * t,  h[ph][k] = s * sinc(u) * w(u) for |u| < zeros, else 0
 *   sinc(u) = sin(pi u) / (pi u), sinc(0) = 1
 *   w(u) = cos^2(pi u / (2 zeros))                               LW_RESAMPLE_HANN
 *   w(u) = I0(beta * sqrt(1 - (u / zeros)^2)) / I0(beta)         LW_RESAMPLE_KAISER; I0 by its power series in double until a
 *                                                                term no longer changes the sum (0 <= beta < 700)
 * The parameters most users know from other toolkits: hann, zeros 6, rolloff 0.99.  A good-quality choice: kaiser, zeros 16,
 * beta 14.769656459379492, rolloff 0.99.
 * A row of len input samples yields out_len = ceil(len * new / orig) output samples.  Output sample n of a row and channel:
 *   base = floor(n * orig / new), ph = (n * orig) mod new      (64-bit integers)
 *   y[n] = the fold over k = 0 .. K - 1 in ascending order of h[ph][k] * x[base - W + k]: every term one rounded f32 multiply;
 *   the first term is the accumulator, every later one is added with one rounded f32 add.  No fused multiply-add, subnormals kept.
 *   x[i] = +0.0 for i < 0 and for i >= len -- len, not the capacity: what the source holds between len and its capacity never
 *   reaches the output, and no byte beyond the capacity is read.  Terms with x = +0.0 take part like any other, so the sign of a
 *   zero result is defined.
 * Nothing outside [0, out_len) of a destination row and channel is written.  orig == new is a copy of the bits of [0, len).
 *
 * lw_resample_rows: source row i (len[i] samples per channel) goes to destination row dst_row[i] (NULL: row i).  len and dst_row
 * are HOST arrays, copied during the call.  Asynchronous on hip_stream; calls on one object may be queued back to back.
 * Overlapping source and destination buffers are the caller's error (the result is then unspecified).  Refusals, decided on
 * the host before anything is queued, so a refused call has written nothing:
 *   LW_ERR_NULL_ARG     rs NULL, len NULL with rows, d_src / d_dst NULL with samples to read / to write
 *   LW_ERR_UNSUPPORTED  (create) a rate of 0, zeros == 0, rolloff outside (0, 1], an unknown window, a kaiser beta outside
 *                       [0, 700), new * K > LW_RESAMPLE_MAX_TAPS;  (rows) an i16 format
 *   LW_ERR_CAPACITY     len[i] > src_capacity, out_len(len[i]) > dst_capacity, dst_row[i] >= n_dst_rows, two source rows for
 *                       one destination row, ch == 0 or > 255
 * (Of the standard rates from 8 to 192 kHz every pair fits LW_RESAMPLE_MAX_TAPS with hann / 6 -- at most 40 960 taps -- and
 * with kaiser / 16 every pair but 11 025 <-> 192 000 Hz; the pairs of 8, 16, 22.05, 32, 44.1 and 48 kHz need 23 040 at most.) */
typedef struct lw_resampler lw_resampler;
enum { LW_RESAMPLE_HANN = 0, LW_RESAMPLE_KAISER = 1 };
#define LW_RESAMPLE_MAX_TAPS 65536
lw_resampler *lw_resampler_create(int device, uint32_t in_rate, uint32_t out_rate, uint32_t zeros, double rolloff, int window, double beta,
		int *err);
void lw_resampler_destroy(lw_resampler *rs);
void lw_resampler_geometry(const lw_resampler *rs, uint32_t *orig, uint32_t *new_, uint32_t *half_width, uint32_t *taps_per_phase);
size_t lw_resampler_taps(const lw_resampler *rs, float *dst); /* [new][K]; returns new * K, dst NULL = size query */
uint64_t lw_resampler_out_len(const lw_resampler *rs, uint64_t len);
int lw_resample_rows(lw_resampler *rs, int fmt, uint32_t ch, const void *d_src, size_t n_src_rows, size_t src_capacity,
		const uint64_t *len, const uint32_t *dst_row, void *d_dst, size_t n_dst_rows, size_t dst_capacity, void *hip_stream);
/* introspection: where the last queued call read taps and samples from -- 0 = table and input span in LDS, 1 = taps from
 * global memory (the table does not fit the workgroup's LDS), 2 = both from global memory, 3 = orig == new, the copy; -1 = no
 * call yet.  lw_resampler_set_taps_in_lds(rs, 0) sends a table that would fit through route 1 (same bits; for tests). */
int lw_resampler_last_route(const lw_resampler *rs);
int lw_resampler_set_taps_in_lds(lw_resampler *rs, int on);

/* ---- spectral frames of rows ---------------------------------------------------------------------------------------------
 * Finished rows -> overlapping frames -> power spectrum or mel features, on the GPU, as a pass of its own (k_spec): what a speech
 * or audio model does first with a [stream][1][samples] tensor.  The source is a rows buffer of either f32 format, `ch` channels,
 *   [row][ch][capacity] (LW_FMT_F32_PLANAR) or [row][capacity][ch] (LW_FMT_F32_INTERLEAVED);
 * the destination is f32 [row][ch][F][frame_capacity], F = n_mels when n_mels > 0, else F = B (the power spectrum).  The
 * transform is a dense windowed DFT, and it is a contract on BITS:
 *
 * A lw_spec is made from (n_fft, win_length, hop, window, center, n_mels, fb).  2 <= n_fft <= LW_SPEC_MAX_FFT,
 * 1 <= win_length <= n_fft, 1 <= hop <= 65535, n_mels <= LW_SPEC_MAX_MELS.  B = n_fft / 2 + 1 bins (integer division).
 *   window  w[i], 0 <= i < win_length:  0.5 - 0.5 cos(2 pi i / win_length)  LW_SPEC_HANN (periodic);  1  LW_SPEC_RECT.
 *           Within a frame it sits at offset o = (n_fft - win_length) / 2 (integer division); the SUPPORT is k in
 *           [o, o + win_length).
 *   basis   the window folded in, evaluated in double and rounded ONCE to f32, for k in the support and 0 <= j < B:
 *           a = 2 pi ((k * j) mod n_fft) / n_fft (reduced in integers before the angle is formed),
 *           C[k][j] = w[k - o] * cos(a),  S[k][j] = -w[k - o] * sin(a)
 *   frames  pad = center ? n_fft / 2 : 0.  n_frames(len), in 64-bit integers: 0 for len == 0; 1 + len / hop when centred;
 *           otherwise len < n_fft ? 0 : 1 + (len - n_fft) / hop.  Sample k of frame t is x[t * hop - pad + k] (signed 64-bit
 *           index); x[i] = +0.0 for i < 0 and for i >= len -- len, not the capacity: what the source holds between len and its
 *           capacity never reaches the output, and no byte beyond the capacity is read.
 *   reflect   With LW_SPEC_PAD_REFLECT (centred objects only; LW_SPEC_PAD_ZERO, the rule above, is what a new object has):
 *           x[i] = x[-i] for i < 0 and x[i] = x[2 (len - 1) - i] for i >= len, one reflection that does not repeat the edge sample,
 *           as numpy.pad(mode="reflect"); the indices are 64-bit integers.  Frame counts, basis, chains and what is written are
 *           unchanged.  One reflection must reach every support sample of every frame, so a row with
 *           0 < len < n_fft - n_fft / 2 + 1 (integer division) is refused; len == 0 still yields no frames.  For even n_fft that
 *           is len > n_fft / 2, torch.stft's own condition.  For odd n_fft it is one sample stricter than torch's, and n_frames
 *           stays 1 + len / hop: torch.stft yields one frame fewer when hop divides len (its padded row is one sample short
 *           of that frame), the frames both compute are the same.
 *   spectrum  re[j]: acc = +0.0; for k ascending over the support acc = fmaf(x_k, C[k][j], acc).  im[j]: the same with S.
 *           P[j] = fmaf(im, im, re * re), the product re * re one rounded f32 multiply.
 *   mel     (n_mels > 0) fb is the caller's matrix, n_mels x B host floats, fb[q * B + j], copied at creation.
 *           m[q]: acc = +0.0; for j = 0 .. B - 1 ascending acc = fmaf(P[j], fb[q][j], acc).  Dense: a weight of 0 takes part
 *           like any other.
 *   bits    no reassociation, no chain split over k or over j, subnormals kept.  Two things are NOT part of the contract: the
 *           sign of a zero result (a zero-padded tail of a matrix tile can turn -0 into +0, and a spectrum is squared anyway)
 *           and which NaN a NaN result is.  Every other bit is.
 * Exactly [0, n_frames(len)) of each of the F lines of a destination row and channel is written, nothing else.
 *
 * lw_spec_create_ex takes a lw_spec_params and adds what a Kaldi-compatible front end (torchaudio.compliance.kaldi.fbank,
 * kaldi-native-fbank) needs; lw_spec_create is lw_spec_create_ex with framing = LW_SPEC_FRAMES_STFT, remove_dc = energy = 0,
 * preemphasis = 0.0, scale = 1.0, and its tables and results keep every bit; it takes LW_SPEC_HANN and LW_SPEC_RECT only, as
 * before.  All options are orthogonal to each other.
 *   windows   with a = 2 pi i / (win_length - 1), symmetric (these four need win_length >= 2):
 *           LW_SPEC_HAMMING 0.54 - 0.46 cos a;  LW_SPEC_HANN_SYM 0.5 - 0.5 cos a;  LW_SPEC_POVEY pow(0.5 - 0.5 cos a, 0.85);
 *           LW_SPEC_BLACKMAN 0.42 - 0.5 cos a + 0.08 cos 2a.
 *   framing   LW_SPEC_FRAMES_STFT: the rule above; `center` applies only here.  The Kaldi framings count frames by the WINDOW,
 *           which starts at sample 0 of the frame: o = 0, the support is k in [0, win_length) of an n_fft-point transform.
 *           LW_SPEC_FRAMES_KALDI_SNIP (snip_edges): n_frames = len < win_length ? 0 : 1 + (len - win_length) / hop; frame t
 *           starts at t * hop; nothing is padded.
 *           LW_SPEC_FRAMES_KALDI_EDGES: n_frames = (len + hop / 2) / hop; frame t starts at t * hop + hop / 2 - win_length / 2
 *           (integer divisions of the positive quantities, a signed 64-bit result).  x[i] = x[-i - 1] for i < 0 and
 *           x[2 len - 1 - i] for i >= len: one reflection that repeats the edge sample, LW_SPEC_PAD_SYMMETRIC, the pad mode such
 *           an object is in.  A row is refused (LW_ERR_CAPACITY) when the first index any of its frames touches is < -len or
 *           the last is > 2 len - 1: a second reflection is not offered.  lw_spec_set_pad_mode on a Kaldi-framed object is
 *           LW_ERR_UNSUPPORTED.  lw_spec_frames answers by the object's framing.
 *   folded    pre-emphasis (coefficient c = preemphasis in [0, 1]), window and scale (finite, > 0; Kaldi callers pass 32768) are
 *           linear in the frame and live in the table.  With g_k = w[k] * cos(2 pi (((k + o) * j) mod n_fft) / n_fft) in double
 *           and g_W = 0:  C[k][j] = (float)(scale * ((k == 0 ? 1.0 - c : 1.0) * g_k - c * g_{k+1})), S the same with -sin --
 *           Kaldi's y_0 = x_0 - c x_0, y_k = x_k - c x_{k-1}, then the window.  c = 0 and scale = 1 give g_k itself.
 *           lw_spec_basis returns this table.
 *   per frame (remove_dc, energy) over a frame's W = win_length support samples x_k, after padding:
 *           S1 = the fold of (double)x_k for k ascending from +0.0, sequential; S2 = the same fold of (double)x_k * (double)x_k
 *           (exact in double).  mu = (float)(S1 / (double)W).  x'_k = x_k - mu with remove_dc (one rounded f32 subtraction),
 *           else x_k; the spectrum chains run over x'_k.  Ed = remove_dc ? S2 - (S1 * S1) / (double)W : S2, every operation
 *           one rounding; Ed = 0 if !(Ed > 0);  E = (float)(Ed * (scale * scale)).  With energy, E is line 0 of the
 *           destination and the spectrum or mel lines follow from line 1: F = lw_spec_features counts it.  (Kaldi's
 *           raw_energy = true and column order without htk_compat; the logarithm is lw_feat_rows' business.)
 *   output    LW_SPEC_OUT_POWER (0): the rule above.  LW_SPEC_OUT_COMPLEX: F = 2 B; line j < B is re[j] and line B + j is im[j],
 *           the two chains of "spectrum" themselves, stored without forming P -- what torch.stft returns, split into planes,
 *           and what lw_istft_rows reads.  Not with n_mels > 0, remove_dc or energy (LW_ERR_UNSUPPORTED); pre-emphasis, scale,
 *           every window, framing and pad mode stay (they live in the table or in x).  The sign of a zero and which NaN a NaN
 *           is stay outside the contract, every other bit is inside it.
 *
 * lw_spec_rows: source row i (len[i] samples per channel) goes to destination row dst_row[i] (NULL: row i).  len and dst_row
 * are HOST arrays, copied during the call.  Asynchronous on hip_stream; calls on one object may be queued back to back.
 * Refusals, decided on the host before anything is queued, so a refused call has written nothing:
 *   LW_ERR_NULL_ARG     sp NULL, len NULL with rows, d_src / d_dst NULL with frames to compute; (create) fb NULL with n_mels > 0
 *   LW_ERR_UNSUPPORTED  (create) a parameter outside the limits above, an unknown window or framing, center with a Kaldi framing,
 *                       a symmetric window with win_length < 2, preemphasis outside [0, 1] or NaN, scale not finite or <= 0,
 *                       remove_dc or energy other than 0 or 1, reserved != 0, an unknown output, LW_SPEC_OUT_COMPLEX with
 *                       n_mels > 0, remove_dc or energy;  (rows) an i16 format;
 *                       (set_pad_mode) an unknown mode, reflect on an object that is not centred, any mode on a Kaldi-framed object
 *   LW_ERR_DEVICE       (create) no such device, or its LDS per workgroup is below the 67 648 bytes k_spec needs (asked of the
 *                       device, not assumed)
 *   LW_ERR_CAPACITY     len[i] > src_capacity, n_frames(len[i]) > frame_capacity, dst_row[i] >= n_dst_rows, two source rows for
 *                       one destination row, ch == 0 or > 255, a row too short for one reflection under LW_SPEC_PAD_REFLECT or
 *                       LW_SPEC_PAD_SYMMETRIC */
typedef struct lw_spec lw_spec;
enum { LW_SPEC_HANN = 0, LW_SPEC_RECT = 1, LW_SPEC_POVEY = 2, LW_SPEC_HAMMING = 3, LW_SPEC_HANN_SYM = 4, LW_SPEC_BLACKMAN = 5 };
enum { LW_SPEC_FRAMES_STFT = 0, LW_SPEC_FRAMES_KALDI_SNIP = 1, LW_SPEC_FRAMES_KALDI_EDGES = 2 };
enum { LW_SPEC_OUT_POWER = 0, LW_SPEC_OUT_COMPLEX = 1 };
#define LW_SPEC_MAX_FFT 2048
#define LW_SPEC_MAX_MELS 256
typedef struct lw_spec_params {
	uint32_t n_fft, win_length, hop, n_mels;
	const float *fb;    /* n_mels x B host floats, copied at creation; NULL with n_mels == 0 */
	int32_t window;     /* LW_SPEC_HANN ... LW_SPEC_BLACKMAN */
	int32_t center;     /* LW_SPEC_FRAMES_STFT only */
	int32_t framing;    /* LW_SPEC_FRAMES_* */
	int32_t remove_dc;  /* 0 or 1 */
	int32_t energy;     /* 0 or 1 */
	uint32_t reserved;  /* must be 0 */
	double preemphasis; /* in [0, 1] */
	double scale;       /* finite, > 0 */
	int32_t output;     /* LW_SPEC_OUT_*; 0 (a zeroed struct, and every struct written before the field existed) is the power */
} lw_spec_params;
lw_spec *lw_spec_create(int device, uint32_t n_fft, uint32_t win_length, uint32_t hop, int window, int center, uint32_t n_mels,
		const float *fb, int *err);
lw_spec *lw_spec_create_ex(int device, const lw_spec_params *p, int *err);
void lw_spec_destroy(lw_spec *sp);
uint32_t lw_spec_bins(const lw_spec *sp);                /* B */
uint32_t lw_spec_features(const lw_spec *sp);            /* F */
uint64_t lw_spec_frames(const lw_spec *sp, uint64_t len); /* n_frames(len) */
size_t lw_spec_basis(const lw_spec *sp, float *dst);     /* [2][win_length][B], C then S; returns the count, dst NULL = size query */
uint32_t lw_spec_tile_frames(const lw_spec *sp);         /* the frames one workgroup takes */
int lw_spec_rows(lw_spec *sp, int fmt, uint32_t ch, const void *d_src, size_t n_src_rows, size_t src_capacity, const uint64_t *len,
		const uint32_t *dst_row, void *d_dst, size_t n_dst_rows, size_t frame_capacity, void *hip_stream);
/* routes: 0 = the DFT fold on the matrix cores (v_mfma_f32_32x32x2_f32, whose result is a k-ordered fmaf chain), 1 = the same
 * kernel body with per-lane fmaf chains -- the fall-back and the second witness for the bits.  Both give the same bits.
 * lw_spec_last_route: the route of the last queued call, -1 = no call yet.  lw_spec_set_route: LW_ERR_UNSUPPORTED for a route the
 * build does not have. */
int lw_spec_last_route(const lw_spec *sp);
int lw_spec_set_route(lw_spec *sp, int route);
/* what x[i] is outside [0, len) for the calls that follow ("reflect" above); lw_spec_pad_mode: the mode, -1 for NULL */
enum { LW_SPEC_PAD_ZERO = 0, LW_SPEC_PAD_REFLECT = 1, LW_SPEC_PAD_SYMMETRIC = 2 /* LW_SPEC_FRAMES_KALDI_EDGES' own, never set */ };
int lw_spec_set_pad_mode(lw_spec *sp, int mode);
int lw_spec_pad_mode(const lw_spec *sp);

/* ---- inverse spectral frames of rows -------------------------------------------------------------------------------------
 * Complex spectral frames -> rows of f32 PCM, on the GPU, as a pass of its own (k_istft): the way back from a model that works
 * on the complex STFT (enhancement, separation, vocoder front ends), torch.istft.  The source is f32 [row][ch][2 B][frame_capacity],
 * what lw_spec_rows writes under LW_SPEC_OUT_COMPLEX (line j < B is re[j], line B + j is im[j]); the destination is a rows buffer
 * of either f32 format.  A contract on BITS.
 *
 * A lw_istft is made from the n_fft, win_length, hop, window and center of a lw_istft_params: STFT framing, the ranges and windows of
 * lw_spec, and hop <= win_length (else there are gaps no frame covers) and ov = ceil(win_length / hop) <= LW_ISTFT_MAX_OVERLAP.
 * With B = n_fft / 2 + 1, o = (n_fft - win_length) / 2, pad = center ? n_fft / 2 : 0 (integer divisions), T the row's frame
 * count and P = T == 0 ? 0 : n_fft + (T - 1) * hop:
 *   table   G[l][k], 0 <= l < 2 B, 0 <= k < win_length, evaluated in double and rounded ONCE to f32; w as lw_spec evaluates it.
 *           a = 2 pi (((k + o) * j) mod n_fft) / n_fft (reduced in integers first); c_j = 1 for j == 0 and, when n_fft is even,
 *           for j == n_fft / 2, else 2.  Line l = j < B: G = w[k] * c_j * cos(a) / n_fft.  Line l = B + j: G = -(w[k] * c_j *
 *           sin(a)) / n_fft, but +0.0 exactly for j == 0 and for the even-n_fft Nyquist bin: irfft ignores those imaginary
 *           parts, and so does this.  lw_istft_basis returns the table, [2 B][win_length].
 *   frame   y_t[k]: acc = +0.0; for l = 0 .. 2 B - 1 ascending acc = fmaf(X[l][t], G[l][k], acc): ONE chain over the source's own
 *           line order, never split.  Dense: a zero weight takes part like any other (an Inf in an ignored imaginary part
 *           gives NaN).
 *   add     in padded coordinates p.  xh[p]: acc = +0.0; for every frame t in [0, T) with 0 <= p - t * hop - o < win_length, in
 *           ASCENDING t, acc = acc + y_t[p - t * hop - o], one rounded f32 add each (the fold starts at +0.0: a zero's sign
 *           cannot reach the result).
 *   env     env[p]: the same fold in double, over the same frames in the same order, of w2[k] = w[k] * w[k] (w in double; the
 *           product one rounding, each add one rounding).  lw_istft_window2 returns w2.
 *   output  sample n of the row is p = n + pad.  out[n] = (float)((double)xh[p] / env[p]) when p < P and env[p] > 1e-11 (the
 *           double literal), else +0.0: one double division, one rounding to f32.  (torch.istft raises where the envelope is
 *           small; here the sample has a defined value.)
 *   length  out_len[i] is the caller's wish, as torch.istft(length=): it may pass the natural length
 *           lw_istft_out_len(is, T) = T == 0 ? 0 : P - 2 * pad, and the samples behind what the frames cover are +0.0.
 *           out_len == NULL: the natural lengths.  Exactly [0, out_len[i]) of every destination row and channel is written.
 *   bits    p, t * hop and every element offset are 64-bit.  Which NaN a NaN is stays outside the contract; all else is a bit.
 *
 * lw_istft_rows: source row i (frames[i] frames) goes to destination row dst_row[i] (NULL: row i).  frames, dst_row and out_len
 * are HOST arrays, copied during the call.  Asynchronous on hip_stream; calls on one object may be queued back to back.
 * Refusals, decided on the host before anything is queued, so a refused call has written nothing:
 *   LW_ERR_NULL_ARG     is NULL, frames NULL with rows, d_dst NULL with samples to write, d_src NULL with frames to read;
 *                       (create) the params NULL
 *   LW_ERR_UNSUPPORTED  (create) a parameter outside lw_spec's limits, an unknown window, center other than 0 or 1,
 *                       hop > win_length, ov > LW_ISTFT_MAX_OVERLAP, reserved != 0;  (rows) an i16 format;
 *                       (set_route, set_tile_frames) a value the object does not have
 *   LW_ERR_DEVICE       (create) no such device, or its LDS per workgroup is below the 80 896 bytes k_istft needs (asked of the
 *                       device, not assumed)
 *   LW_ERR_CAPACITY     frames[i] > frame_capacity, out_len[i] > dst_capacity, dst_row[i] >= n_dst_rows, two source rows for one
 *                       destination row, ch == 0 or > 255, a buffer not addressable in 64 bits of bytes */
typedef struct lw_istft lw_istft;
#define LW_ISTFT_MAX_OVERLAP 16
typedef struct lw_istft_params {
	uint32_t n_fft, win_length, hop;
	int32_t window;    /* LW_SPEC_HANN ... LW_SPEC_BLACKMAN: the analysis window, which is the synthesis window */
	int32_t center;    /* 0 or 1 */
	uint32_t reserved; /* must be 0 */
} lw_istft_params;
lw_istft *lw_istft_create(int device, const lw_istft_params *p, int *err);
void lw_istft_destroy(lw_istft *is);
uint32_t lw_istft_bins(const lw_istft *is);                       /* B; the source has 2 B lines */
uint64_t lw_istft_out_len(const lw_istft *is, uint64_t frames);   /* the natural length of a row of `frames` frames */
size_t lw_istft_basis(const lw_istft *is, float *dst);            /* [2 B][win_length]; returns the count, dst NULL = size query */
size_t lw_istft_window2(const lw_istft *is, double *dst);         /* [win_length] doubles, likewise */
int lw_istft_rows(lw_istft *is, uint32_t ch, const void *d_src, size_t n_src_rows, size_t frame_capacity, const uint64_t *frames,
		const uint32_t *dst_row, const uint64_t *out_len, int fmt, void *d_dst, size_t n_dst_rows, size_t dst_capacity, void *hip_stream);
/* routes: 0 = the frame signals on the matrix cores (v_mfma_f32_32x32x2_f32), 1 = the same kernel body with per-lane fmaf
 * chains; both give the same bits.  lw_istft_last_route: the route of the last queued call, -1 = no call yet. */
int lw_istft_last_route(const lw_istft *is);
int lw_istft_set_route(lw_istft *is, int route);
/* A workgroup owns m * hop consecutive padded samples and recomputes the frames that reach into them, so m never reaches a
 * bit.  lw_istft_tile_frames: the object's m.  lw_istft_set_tile_frames (debug: a test runs two values and demands identical
 * bits): 1 <= m <= the m the object was created with, else LW_ERR_UNSUPPORTED. */
uint32_t lw_istft_tile_frames(const lw_istft *is);
int lw_istft_set_tile_frames(lw_istft *is, uint32_t m);

/* ---- finishing feature rows ------------------------------------------------------------------------------------------------
 * Log compression, dynamic-range clamp, affine map and fill of finished feature rows, on the GPU, as a pass of its own (k_feat):
 * what stands between lw_spec_rows' output and a speech model's input (Whisper: log10, floor 1e-10, top 8, add 4, mul 0.25, the
 * scope a row, filled to 3000 frames).  Source and destination are f32 [row][ch][F][frame_capacity], lw_spec_rows' layout;
 * row i has n_frames[i] frames.  A contract on BITS.  For element x of a line at frame t < n_frames[row]:
 *   1  v = (x > floor) ? x : floor.  A NaN and everything at or below the floor become the floor; v is never NaN.
 *   2  l = LOG(v).  LW_FEAT_LOG_NONE: l = v.  Otherwise v = +inf gives +inf, and any other v (positive and finite, see the
 *      refusals) goes through double arithmetic in which every * + - / is ONE correctly rounded IEEE operation, nothing fused:
 *        d = (double)v (exact, a subnormal f32 included);  d = m * 2^e with m in [0.5, 1) (frexp);
 *        if m < RH = 0x1.6a09e667f3bcdp-1 (the double nearest sqrt(1/2)): m = m * 2, e = e - 1
 *        s = (m - 1) / (m + 1),  z = s * s
 *        p = c9; for k = 8 .. 0: p = p * z + c_k, with c_k = 1.0 / (2 k + 1) the correctly rounded quotient
 *        r = (double)e * LN2 + (s + s) * p,  LN2 = 0x1.62e42fefa39efp-1
 *      LW_FEAT_LOG_LN: r.  LW_FEAT_LOG_LOG10: r * LOG10E, LOG10E = 0x1.bcb7b1526e50ep-2.  LW_FEAT_LOG_DB: (r * LOG10E) * 10.0.
 *      Then ONE rounding to f32.  (The series' truncation error is about 2e-17 relative, so l is the correctly rounded f32
 *      logarithm on all but a vanishing share of inputs, and the same bits on every machine with IEEE doubles.)
 *   3  M = the maximum of l over the scope: LW_FEAT_SCOPE_ROW, all ch * F lines of the row, frames [0, n_frames);
 *      LW_FEAT_SCOPE_CHANNEL, the F lines of the channel.  l is never NaN, and +0.0 counts as greater than -0.0, so the order
 *      cannot matter.  An empty scope (n_frames == 0) has M = l0 = LOG(floor) (LW_FEAT_LOG_NONE: l0 = floor).
 *   4  tt = M - top, one rounded f32 subtraction; top == +inf: tt = -inf whatever M is (no clamp).  y = (l > tt) ? l : tt.
 *   5  z = (y + add) * mul, two rounded f32 operations.  (Whisper's (x + 4) / 4: add = 4, mul = 0.25, exact.)
 * Positions [n_frames, max(n_frames, fill_to[row])) of every line receive what x = floor would give (steps 2 - 5 with the
 * scope's M); they take no part in M.  Nothing else of d_dst is written, and nothing of d_src beyond n_frames of a line is read.
 * d_max, when given, receives M per scope: f32 [n_rows] (row scope) or [n_rows][ch], rows with nothing written included.  Which
 * NaN a NaN result is, is outside the contract (z can be one, inf * 0); every other bit is inside it, the sign of a zero included.
 * d_src == d_dst is allowed (in place); any other overlap is the caller's error.
 *
 * lw_feat_rows: n_frames and fill_to (may be NULL: nothing is filled) are HOST arrays, copied during the call.  Asynchronous on
 * hip_stream; calls on one object may be queued back to back.  Two kernel launches on the stream (the second combines the
 * tiles' maxima and re-reads the l the first one stored in d_dst); one when top == +inf and d_max is NULL.
 * lw_feat_last_launches: the kernels the last accepted call queued, -1 = no call yet.  lw_feat_log: step 2 for one value on the
 * host (NaN for a v that step 1 cannot produce: NaN, or not positive under a log kind).
 * Refusals, decided on the host before anything is queued:
 *   LW_ERR_NULL_ARG     ft or p NULL, n_frames NULL with rows, d_src NULL with frames to read, d_dst NULL with elements to write
 *   LW_ERR_UNSUPPORTED  (create) an unknown log or scope; a log kind with a floor that is not a positive finite f32 (a subnormal
 *                       is fine); floor NaN; top NaN or negative; add or mul NaN
 *   LW_ERR_DEVICE       (create) no such device
 *   LW_ERR_CAPACITY     n_frames[i] or fill_to[i] > frame_capacity, ch == 0 or > 255, F == 0 or > 65535, a buffer that 64 bits of
 *                       bytes cannot address, more than 2^32 - 1 runs of 256 frames in one channel */
typedef struct lw_feat lw_feat;
enum { LW_FEAT_LOG_NONE = 0, LW_FEAT_LOG_LN = 1, LW_FEAT_LOG_LOG10 = 2, LW_FEAT_LOG_DB = 3 };
enum { LW_FEAT_SCOPE_ROW = 0, LW_FEAT_SCOPE_CHANNEL = 1 };
typedef struct {
	int32_t log, scope;
	float floor, top, add, mul;
} lw_feat_params;
lw_feat *lw_feat_create(int device, const lw_feat_params *p, int *err);
void lw_feat_destroy(lw_feat *ft);
float lw_feat_log(const lw_feat *ft, float v);
int lw_feat_rows(lw_feat *ft, uint32_t ch, uint32_t F, const void *d_src, void *d_dst, size_t n_rows, size_t frame_capacity,
		const uint64_t *n_frames, const uint64_t *fill_to, float *d_max, void *hip_stream);
int lw_feat_last_launches(const lw_feat *ft);

/* ---- normalising rows ----------------------------------------------------------------------------------------------------
 * Mean removal and scaling of rows by a statistic of their own, on the GPU, as a pass of its own (k_norm): per-utterance
 * (x - mean) / sqrt(var + 1e-7) for the waveform models (wav2vec 2.0, HuBERT, WavLM), utterance CMVN for the feature models (every
 * mel band over time), peak and RMS level.  Source and destination are f32 [row][ch][F][capacity], lw_spec_rows' and lw_feat_rows'
 * layout; a planar waveform rows buffer [row][ch][capacity] is F = 1.  Row i has n[i] valid elements per line.  A SCOPE is what one
 * statistic is taken over: LW_NORM_SCOPE_ROW, all ch * F lines of a row; LW_NORM_SCOPE_CHANNEL, the F lines of a channel;
 * LW_NORM_SCOPE_LINE, one line.  A scope of L lines has N = L * n elements.  A contract on BITS, and the first in this library whose
 * result depends on the ORDER of a summation -- so the order is part of it.  All arithmetic of steps 1 - 4 is double; every + - * /
 * and sqrt is ONE correctly rounded IEEE operation, nothing fused.
 *   1  Chunk sums.  A line is cut into chunks of 256 consecutive elements counted from the line's element 0 (by index, not by
 *      address); C = ceil(n / 256).  Elements of a chunk at or beyond n are +0.0 and take part like any other.  With elements
 *      4i .. 4i + 3 of the chunk as doubles d0 .. d3 (i = 0 .. 63; the squares are exact in double):
 *        a_i = ((d0 + d1) + d2) + d3,   b_i = ((d0*d0 + d1*d1) + d2*d2) + d3*d3
 *      The 64 values are folded by the adjacent-pair tree t[j] = t[2j] + t[2j + 1], six levels, a and b each.  The chunk's peak is
 *      the largest |x| of its elements below n, compared as the unsigned bit patterns of |x| (a NaN therefore wins, and the order
 *      cannot matter).  A chunk so yields a triple (sum, sum of squares, peak).
 *   2  Scope sums.  The chunk triples of a scope are listed line-major: channel, then feature line, then chunk, all ascending.  A
 *      list of more than one entry is folded 64 entries at a time by the same six-level tree, a short last group padded with +0.0
 *      (sums) or 0 (peak); the resulting list is folded the same way, until one triple (S1, S2, P) is left.  A list of one entry is
 *      that entry.
 *   3  Scalars.  mu = S1 / (double)N;  q = S2 / (double)N;  v = q - mu * mu, and v = 0 if !(v > 0);  m = center ? mu : +0.0;
 *        LW_NORM_SCALE_NONE  g = 1.0                          LW_NORM_SCALE_STD   g = 1.0 / sqrt(v + eps)
 *        LW_NORM_SCALE_RMS   g = target / sqrt(q + eps)       LW_NORM_SCALE_PEAK  g = (P == 0) ? 1.0 : target / (double)P
 *      An empty scope (n == 0) has m = +0.0, g = 1.0.
 *   4  z = (float)(((double)x - m) * g): one subtraction, one multiplication, one rounding to f32.  With center = 0 and no scale
 *      this is a bit copy of every value that is not a NaN.
 * Positions [n, max(n, fill_to[row])) of every line receive +0.0.  Nothing else of d_dst is written, and nothing of d_src at or
 * beyond n of a line is read.  d_stats, when given, receives (m, g) as two doubles per scope in row / channel / line order --
 * [n_rows][2], [n_rows][ch][2] or [n_rows][ch][F][2] -- rows with n == 0 included.  Which NaN a NaN result is, is outside the
 * contract; every other bit is inside it, the sign of a zero included.  d_src == d_dst is allowed (in place); any other overlap is
 * the caller's error.
 * Accuracy: S1 and S2 carry an error of at most about 26 * 2^-53 of the sum of the magnitudes up to 2^18 chunks in a scope (2 + 6
 * additions deep in a chunk, 6 per list level, three levels), six more per further level.  v = q - mu * mu cancels: its relative error is about 2^-50 * (1 + mu^2 / v) -- ample for audio, where a DC offset is a
 * fraction of the deviation, and poor only for an offset thousands of times the deviation (at 512 deviations z is still within
 * one f32 ulp of the exactly centred value; at 10 000 it is not).
 *
 * lw_norm_rows: n and fill_to (may be NULL: nothing is filled) are HOST arrays, copied during the call.  Asynchronous on
 * hip_stream; calls on one object may be queued back to back.  No float atomics: the bits depend neither on the grid nor on the
 * number of launches.  Three kernel launches on the stream (chunk sums into a list the object owns; the fold of each scope's list
 * to (m, g); apply and fill); without center and scale one (apply and fill; the fold before it only when d_stats is given); the sums
 * are left out when no row has an element, the apply pass when nothing is to be written.
 * lw_norm_last_launches: the kernels the last accepted call queued, -1 = no call yet.  lw_norm_scalars: step 3 on the host, from
 * the same source as the kernel's (P is the peak as an f32, N the scope's element count).
 * Refusals, decided on the host before anything is queued:
 *   LW_ERR_NULL_ARG     nm, p, m or g NULL, n NULL with rows, d_src NULL with elements to read, d_dst NULL with elements to write
 *   LW_ERR_UNSUPPORTED  (create) an unknown scale or scope; center not 0 or 1; reserved != 0; eps NaN, negative or infinite; target
 *                       not positive and finite under LW_NORM_SCALE_RMS or LW_NORM_SCALE_PEAK
 *   LW_ERR_DEVICE       (create) no such device
 *   LW_ERR_CAPACITY     n[i] or fill_to[i] > capacity, ch == 0 or > 255, F == 0 or > 65535, a buffer that 64 bits of bytes cannot
 *                       address, more than 2^32 - 1 chunks in one row (its longest possible list) */
typedef struct lw_norm lw_norm;
enum { LW_NORM_SCALE_NONE = 0, LW_NORM_SCALE_STD = 1, LW_NORM_SCALE_RMS = 2, LW_NORM_SCALE_PEAK = 3 };
enum { LW_NORM_SCOPE_ROW = 0, LW_NORM_SCOPE_CHANNEL = 1, LW_NORM_SCOPE_LINE = 2 };
typedef struct {
	int32_t center, scale, scope, reserved;
	double eps, target;
} lw_norm_params;
lw_norm *lw_norm_create(int device, const lw_norm_params *p, int *err);
void lw_norm_destroy(lw_norm *nm);
int lw_norm_rows(lw_norm *nm, uint32_t ch, uint32_t F, const void *d_src, void *d_dst, size_t n_rows, size_t capacity, const uint64_t *n,
		const uint64_t *fill_to, double *d_stats, void *hip_stream);
int lw_norm_scalars(const lw_norm *nm, double S1, double S2, float P, uint64_t N, double *m, double *g);
int lw_norm_last_launches(const lw_norm *nm);

/* ---- cepstra and deltas of feature rows ----------------------------------------------------------------------------------
 * A matrix ACROSS the feature lines of finished feature rows and a regression filter ALONG their frames, on the GPU, as a pass
 * of its own (k_cep): MFCC (a DCT of the log-mel lines, optionally liftered) and the delta / delta-delta features taken of
 * cepstra or of filterbanks (HuBERT's 39-dimensional k-means targets, HTK / Kaldi "fbank + deltas").  Source: f32
 * [row][ch][n_in][frame_capacity], the layout of lw_spec_rows, lw_feat_rows and lw_norm_rows.  Destination: f32
 * [row][ch][n_out * (1 + order)][frame_capacity], the same frame_capacity: lines 0 .. n_out - 1 are the static features, the
 * next n_out their deltas, the next n_out the delta-deltas (HTK / Kaldi order).  Row i has n_frames[i] frames.  An object is made
 * from (n_in, n_out, matrix, order, width): 1 <= n_in <= LW_CEP_MAX_IN, 1 <= n_out <= LW_CEP_MAX_OUT, order 0, 1 or 2, width N
 * in 1 .. LW_CEP_MAX_WIDTH when order > 0 and 0 when order == 0.  A contract on BITS.  For frame t < n_frames[row]:
 *   1  Static line q.  matrix is the caller's n_out x n_in HOST floats, matrix[q * n_in + f], copied at creation.  With x[f][t]
 *      element t of source line f:  acc = +0.0;  for f = 0 .. n_in - 1 ascending: acc = fmaf(x[f][t], matrix[q][f], acc).  The
 *      fold is dense: a weight of 0 takes part like any other.  matrix == NULL is the identity and needs n_out == n_in: the
 *      static lines are then a BIT COPY of the source lines (deltas of filterbanks with no arithmetic on the static part).
 *   2  Delta weights.  D = 2 * (1*1 + 2*2 + .. + N*N) as an integer;  w_n = (float)((double)n / (double)D) for n = 1 .. N: one
 *      double division, one rounding, on the host.  The kernel divides nothing.
 *   3  Delta of a line s.  With c(i) = min(max(i, 0), n_frames - 1) in signed 64-bit integers (the edge frames are replicated):
 *        acc = +0.0;  for n = 1 .. N ascending:  d = s[c(t + n)] - s[c(t - n)] (ONE rounded f32 subtraction);  acc = fmaf(w_n, d, acc)
 *      The delta lines are this of the static lines.  The delta-delta lines are this OF THE DELTA LINES, with the same clamp --
 *      what torchaudio.functional.compute_deltas applied twice gives, and python_speech_features.delta.  (Kaldi's add-deltas
 *      convolves the two windows and clamps once, so it differs within 2 N frames of either end; librosa's Savitzky-Golay deltas
 *      differ at the edges.)
 * No reassociation, no chain split over f or over n, subnormals kept.  The sign of a zero is inside the contract; which NaN a
 * NaN result is, is outside it.  Positions [n_frames, max(n_frames, fill_to[row])) of every destination line receive +0.0.
 * Nothing else of d_dst is written, and nothing of d_src at or beyond n_frames of a line is read.  Any overlap of d_src and d_dst
 * is the caller's error: the shapes differ, so there is no in-place form.
 * Accuracy of a static line against the exact sum: |acc - exact| <= (n_in + 1) * 2^-24 * sum_f |x[f][t]| |matrix[q][f]| (n_in
 * roundings of partial sums that are at most the sum of the magnitudes, and the rounding of the weights).
 *
 * lw_cep_rows: n_frames and fill_to (may be NULL: nothing is filled) are HOST arrays, copied during the call.  Asynchronous on
 * hip_stream; calls on one object may be queued back to back.  ONE kernel launch per 65535 rows on the stream, none when nothing
 * is to be written: the source is read once and every destination line written once.  A workgroup produces lw_cep_tile_frames
 * consecutive frames of a row and channel (256 - 2 * order * width) and recomputes the order * width frames either side of them
 * at their clamped indices; no atomics, and the bits depend neither on the tile nor on the grid.
 * lw_cep_features: n_out * (1 + order).  lw_cep_matrix: the matrix as the kernel reads it, [n_out][n_in] floats into dst; returns
 * their count (dst NULL: the count alone), 0 for the identity.  lw_cep_delta_weights: w_1 .. w_N into dst (may be NULL); returns
 * N.  lw_cep_last_launches: the kernels the last accepted call queued, -1 = no call yet.
 * Refusals, decided on the host before anything is queued:
 *   LW_ERR_NULL_ARG     cp NULL, n_frames NULL with rows, d_src NULL with frames to read, d_dst NULL with elements to write;
 *                       (create) matrix NULL with n_out != n_in
 *   LW_ERR_UNSUPPORTED  (create) n_in or n_out outside its limits, order > 2, width outside 1 .. LW_CEP_MAX_WIDTH under an order,
 *                       width != 0 without one
 *   LW_ERR_DEVICE       (create) no such device, or one whose workgroups have less LDS than the kernel needs (order * 256 *
 *                       min(32, n_out rounded up to 8) floats; the device is asked)
 *   LW_ERR_CAPACITY     n_frames[i] or fill_to[i] > frame_capacity, ch == 0 or > 255, a buffer that 64 bits of bytes cannot address,
 *                       more than 2^24 - 1 tiles in a line (a grid dimension holds fewer than 2^32 lanes, a tile has 256) */
#define LW_CEP_MAX_IN 256
#define LW_CEP_MAX_OUT 256
#define LW_CEP_MAX_WIDTH 16
typedef struct lw_cep lw_cep;
lw_cep *lw_cep_create(int device, uint32_t n_in, uint32_t n_out, const float *matrix, uint32_t order, uint32_t width, int *err);
void lw_cep_destroy(lw_cep *cp);
uint32_t lw_cep_features(const lw_cep *cp);
size_t lw_cep_matrix(const lw_cep *cp, float *dst);
uint32_t lw_cep_delta_weights(const lw_cep *cp, float *dst);
uint32_t lw_cep_tile_frames(const lw_cep *cp);
int lw_cep_rows(lw_cep *cp, uint32_t ch, const void *d_src, void *d_dst, size_t n_rows, size_t frame_capacity, const uint64_t *n_frames,
		const uint64_t *fill_to, void *hip_stream);
int lw_cep_last_launches(const lw_cep *cp);

/* ---- frame-major model input ---------------------------------------------------------------------------------------------
 * The last step between the chain's feature rows and a model that reads [batch][frame][feature] (WeNet, icefall, ESPnet, FunASR,
 * SeamlessM4T, AST, BEATs): transpose, splice or stack-and-skip a context of frames, a global shift and scale per output element,
 * ONE rounding to the model's number format, padding and the padding mask, on the GPU, as a pass of its own (k_pack) that reads
 * the source once and writes the destination once.  Source: f32 [row][ch][F][frame_capacity], the layout of every stage before
 * it; row i has n_frames[i] frames.  An object is made from (F, left, right, stride, edge, dtype, shift, scale, pad); W = left +
 * right + 1, D = W * F.  Destination: [row][ch][out_capacity][D] of dtype (LW_PACK_F32, LW_PACK_BF16, LW_PACK_F16): a frame is D
 * contiguous elements, element j = k * F + f is feature line f of context position k, k = 0 the oldest frame (Kaldi's
 * splice-feats and FunASR's LFR order).  A contract on BITS.
 *   Frames of a row, T = n_frames[row], all in signed 64-bit integers:
 *     LW_PACK_EDGE_REPLICATE  T_out = ceil(T / stride);  context position k of output frame u is source frame
 *                             c(u * stride - left + k), c(i) = min(max(i, 0), T - 1)   (FunASR's apply_lfr(m, n) is left =
 *                             (m - 1) / 2, right = m - 1 - left, stride = n)
 *     LW_PACK_EDGE_VALID      T_out = T < W ? 0 : (T - W) / stride + 1;  source frame u * stride + k, never outside the row
 *                             ("stack m skip n": left = 0, right = m - 1, stride = n)
 *   Value, with x the source element:  v = x;  if shift is given v = v + shift[j], ONE rounded f32 addition;  if scale is given
 *     v = v * scale[j], ONE rounded f32 multiplication;  nothing is fused.  A step whose array is NULL is SKIPPED, not done with 0
 *     or 1 (-0.0 + 0.0 is not a bit copy).  shift and scale are D HOST floats each, copied at creation, indexed by the OUTPUT
 *     element j (a per-line vector is repeated W times by the caller).  With both NULL and LW_PACK_F32 the pass is a bit copy of
 *     every value, NaN payloads included.
 *   Conversion: one rounding of v, in integer arithmetic on its bit pattern u (a = u & 0x7fffffff, s = the sign moved to bit 15):
 *     LW_PACK_BF16  a > 0x7f800000 (a NaN, taken FIRST): a NaN.  Otherwise (u + 0x7fff + ((u >> 16) & 1)) >> 16: round to nearest
 *                   even on bit 16; a finite value may round to infinity.
 *     LW_PACK_F16   a > 0x7f800000: a NaN.  a >= 0x47800000 (65536 and above, infinity): s | 0x7c00.  a >= 0x38800000 (2^-14 and
 *                   above): m = a - 0x38000000;  s | ((m + 0xfff + ((m >> 13) & 1)) >> 13), which carries into the exponent and,
 *                   from 65520 on, into infinity.  a < 0x33000000 (below 2^-25): s.  Otherwise a subnormal: e = a >> 23, sh = 126 - e
 *                   (14 .. 24), M = (a & 0x7fffff) | 0x800000, r = M >> sh, rem = M & ((1 << sh) - 1), half = 1 << (sh - 1);
 *                   r = r + 1 if rem > half or (rem == half and r is odd);  s | r.  IEEE round to nearest even throughout.
 *     A NaN stays a NaN; which NaN is outside the contract.  Every other bit is inside it, the sign of a zero included.
 *   Fill and mask: positions [T_out, max(T_out, fill_to[row])) of every channel receive pad, an f32 parameter converted by the same
 *     rule, without shift or scale.  d_mask, when given, is uint8 [n_rows][out_capacity]: 1 on [0, T_out), 0 on [T_out, fill_end),
 *     written once, not once per channel.  Nothing else of either buffer is written, and nothing of d_src at or beyond n_frames of
 *     a line is read.  Any overlap of source and destination is the caller's error.
 *
 * lw_pack_rows: n_frames and fill_to (may be NULL: nothing is filled; in OUTPUT frames) are HOST arrays, copied during the call.
 * Asynchronous on hip_stream; calls on one object may be queued back to back.  ONE kernel launch per 65535 rows, none when nothing
 * is to be written.  A workgroup takes lw_pack_tile_frames consecutive output frames of a row and channel; the bits depend
 * neither on the tile nor on the grid.  lw_pack_width: D.  lw_pack_frames: T_out of T, on the host.  lw_pack_convert: the
 * conversion of one value on the host, from the same source as the kernel's; the bit pattern in the low 32 or 16 bits.
 * lw_pack_last_launches: the kernels the last accepted call queued, -1 = no call yet.
 * Refusals, decided on the host before anything is queued:
 *   LW_ERR_NULL_ARG     pk or p NULL, n_frames NULL with rows, d_src NULL with frames to read, d_dst NULL with elements to write
 *   LW_ERR_UNSUPPORTED  (create) an unknown edge or dtype, F outside 1 .. 65535, left or right > LW_PACK_MAX_CONTEXT, stride == 0 or
 *                       > LW_PACK_MAX_STRIDE, pad NaN
 *   LW_ERR_DEVICE       (create) no such device, or one whose workgroups have less LDS than the kernel's image (min(F, 32) lines
 *                       of up to 289 floats; the device is asked)
 *   LW_ERR_CAPACITY     n_frames[i] > frame_capacity, lw_pack_frames(n_frames[i]) or fill_to[i] > out_capacity, ch == 0 or > 255, a
 *                       buffer that 64 bits of bytes cannot address, more than 2^24 - 1 tiles in a row (a grid dimension holds
 *                       fewer than 2^32 lanes, a workgroup has 256) */
#define LW_PACK_MAX_CONTEXT 16
#define LW_PACK_MAX_STRIDE 16
typedef struct lw_pack lw_pack;
enum { LW_PACK_F32 = 0, LW_PACK_BF16 = 1, LW_PACK_F16 = 2 };
enum { LW_PACK_EDGE_REPLICATE = 0, LW_PACK_EDGE_VALID = 1 };
typedef struct {
	uint32_t F, left, right, stride;
	int32_t edge, dtype;
	float pad;
	uint32_t reserved; /* 0 */
} lw_pack_params;
lw_pack *lw_pack_create(int device, const lw_pack_params *p, const float *shift, const float *scale, int *err);
void lw_pack_destroy(lw_pack *pk);
uint32_t lw_pack_width(const lw_pack *pk);
uint32_t lw_pack_tile_frames(const lw_pack *pk);
uint64_t lw_pack_frames(const lw_pack *pk, uint64_t T);
uint32_t lw_pack_convert(const lw_pack *pk, float v);
int lw_pack_rows(lw_pack *pk, uint32_t ch, const void *d_src, void *d_dst, size_t n_rows, size_t frame_capacity, size_t out_capacity,
		const uint64_t *n_frames, const uint64_t *fill_to, uint8_t *d_mask, void *hip_stream);
int lw_pack_last_launches(const lw_pack *pk);

/* ---- sliding-window normalisation of feature rows ---------------------------------------------------------------------------
 * Kaldi's apply-cmvn-sliding on the GPU, as a pass of its own (k_slide): every frame of a feature line minus the mean of a window
 * of frames around (center) or before it, optionally divided by the window's deviation -- what the x-vector recipes run with a
 * 300-frame centred window between fbank / mfcc and the model, and what streaming ASR uses in place of utterance CMVN.  Source and
 * destination are f32 [row][ch][F][frame_capacity], the layout of every stage before it; row i has T = n_frames[i] frames.  An
 * object is made from (cmn_window W, min_cmn_window, center, norm_vars): 1 <= min_cmn_window <= W <= LW_SLIDE_MAX_WINDOW, center
 * and norm_vars 0 or 1.  A contract on BITS, applied to every line on its own; the order of the sums is part of it.
 *   1  The window [s, e) of frame t, Kaldi's rule, in signed 64-bit integers:
 *        center:     s = t - W / 2 (integer division), e = s + W;      otherwise:  s = t - W, e = t + 1 (W + 1 frames, as in Kaldi)
 *        if s < 0:  e -= s, then s = 0;      if not center and e > t:  e = max(t + 1, min_cmn_window);
 *        if e > T:  s -= e - T, e = T, and s = 0 if s < 0.
 *      (T, W, min, center) = (10, 4, 2, 1): t = 0, 1, 2, 3, 8, 9 have [0,4) [0,4) [0,4) [1,5) [6,10) [6,10);
 *      (10, 4, 3, 0): t = 0, 1, 2, 3, 5, 9 have [0,3) [0,3) [0,3) [0,4) [1,6) [5,10).  Every window contains t and lies in
 *      [t - W, t + W] and in [0, T); s and e never decrease with t, and s grows by at most one a frame.
 *   2  Block sums.  A line is cut into blocks of 16 frames counted from the line's frame 0 (by index, not by address).  A_b: from
 *      +0.0, add (double)x[16 b + i] for i = 0 .. 15 ascending, one rounded double add each.  Q_b: the same fold of the squares
 *      (exact in double).
 *   3  The window sum.  b0 = ceil(s / 16), b1 = floor(e / 16).  ONE accumulator from +0.0, one rounded double add per term:
 *        b0 >= b1:   the elements s .. e - 1 ascending;
 *        otherwise:  the elements s .. 16 b0 - 1, then A_b0 .. A_(b1 - 1), then the elements 16 b1 .. e - 1.
 *      This is S.  Q is the same fold over the squares and Q_b.  (A 600-frame window takes at most 15 + 37 + 15 adds.)
 *   4  The value.  n = e - s;  mu = S / (double)n.
 *        without norm_vars:  z = (float)((double)x[t] - mu)
 *        norm_vars, n == 1:  z = +0.0
 *        norm_vars, n > 1:   v = Q / (double)n - mu * mu;  v = 1e-10 if !(v > 1e-10);  g = 1.0 / sqrt(v);
 *                            z = (float)(((double)x[t] - mu) * g)
 *      Every + - * / and sqrt is ONE IEEE double operation, nothing fused.
 *   5  Positions [T, max(T, fill_to[row])) of every destination line receive +0.0.  Nothing else of d_dst is written, and nothing of
 *      d_src at or beyond T of a line is read.  Any overlap of d_src and d_dst is the caller's error: neighbours are read, so there
 *      is no in-place form.  The sign of a zero is inside the contract; which NaN a NaN result is, is outside it.
 * Accuracy: an element of the window passes through at most d = 16 + 15 + ((W + 1) / 16 + 1) + 15 additions (16 in its block, then
 * the terms of rule 3), so |S - exact| <= d * 2^-53 * sum |x| over the window (first order), the same for Q over the squares: d = 84
 * at W = 600, 175 at W = 2048.  z without norm_vars is then within half an f32 ulp plus (d + 2) * 2^-53 * (mean |x| + |x[t]|) of the exactly
 * centred value.  v = Q / n - mu * mu cancels as in "normalising rows": its relative error is about d * 2^-52 * (1 + mu^2 / v).
 *
 * lw_slide_rows: n_frames and fill_to (may be NULL: nothing is filled) are HOST arrays, copied during the call.  Asynchronous on
 * hip_stream; calls on one object may be queued back to back.  ONE kernel launch per 65535 rows (the one-launch form: block sums
 * are recomputed by every workgroup over its own span in LDS, nothing goes through scratch), none when nothing is to be written.
 * A workgroup takes lw_slide_tile_frames consecutive frames (1024) of up to 16 lines of a row and channel and stages the frames
 * its windows cover -- at most tile + W + 15 -- as floats, with their block sums as doubles, in at most 64 KiB of LDS (4.125 + 1
 * bytes per staged frame and line; the number of lines is what fits, a multiple of four from four on: the chains of four lines
 * run side by side in a lane).  No atomics, no workgroup waits on another; the bits depend
 * neither on the tile nor on the grid.  lw_slide_set_tile_frames: a test's handle on the seams, a multiple of 16 in 16 .. 4096.
 * lw_slide_window: rule 1 on the host, from the same source as the kernel's.  lw_slide_last_launches: the kernels the last
 * accepted call queued, -1 = no call yet.
 * Refusals, decided on the host before anything is queued:
 *   LW_ERR_NULL_ARG     sl, p, start or end NULL, n_frames NULL with rows, d_src NULL with frames to read, d_dst NULL with elements
 *                       to write
 *   LW_ERR_UNSUPPORTED  (create) min_cmn_window == 0 or > cmn_window, cmn_window > LW_SLIDE_MAX_WINDOW, center or norm_vars not 0 or
 *                       1; (set_tile_frames) a tile that is no multiple of 16 in 16 .. 4096
 *   LW_ERR_DEVICE       (create) no such device, or one whose workgroups have less than 64 KiB of LDS (the device is asked)
 *   LW_ERR_CAPACITY     n_frames[i] or fill_to[i] > frame_capacity, ch == 0 or > 255, F == 0 or > 65535, a buffer that 64 bits of
 *                       bytes cannot address, more than 2^24 - 1 workgroups (tiles * line groups) in a channel; (window) t >= T */
#define LW_SLIDE_MAX_WINDOW 2048
typedef struct lw_slide lw_slide;
typedef struct {
	uint32_t cmn_window, min_cmn_window;
	int32_t center, norm_vars;
} lw_slide_params;
lw_slide *lw_slide_create(int device, const lw_slide_params *p, int *err);
void lw_slide_destroy(lw_slide *sl);
int lw_slide_rows(lw_slide *sl, uint32_t ch, uint32_t F, const void *d_src, void *d_dst, size_t n_rows, size_t frame_capacity,
		const uint64_t *n_frames, const uint64_t *fill_to, void *hip_stream);
int lw_slide_window(const lw_slide *sl, uint64_t t, uint64_t T, uint64_t *start, uint64_t *end);
uint32_t lw_slide_tile_frames(const lw_slide *sl);
int lw_slide_set_tile_frames(lw_slide *sl, uint32_t tile);
int lw_slide_last_launches(const lw_slide *sl);

/* ---- energy voice-activity decisions of feature rows --------------------------------------------------------------------------
 * Kaldi's compute-vad-energy on the GPU, as a pass of its own (k_vad): the per-frame voiced / unvoiced decision that every
 * x-vector, diarization and language-ID recipe takes from the log energy of the RAW features, before apply-cmvn-sliding, and hands
 * to select-voiced-frames.  The source is f32 [row][ch][F][frame_capacity], the layout of every stage before it; the mask is uint8
 * [row][ch][frame_capacity], exactly what lw_select_rows takes.  Row i has T = n_frames[i] frames.  An object is made from Kaldi's
 * options without their vad_ prefix, with Kaldi's defaults: energy_threshold 5.0f, energy_mean_scale 0.5f, frames_context 0,
 * proportion_threshold 0.6f; line (0) is the feature line that holds the log energy; reserved is 0.  The float parameters are f32,
 * as Kaldi's BaseFloat.  A contract on BITS, for every row and channel on its own, with e[t] element t of line `line`:
 *   1  The threshold.  If energy_mean_scale == 0 or T == 0: thr = energy_threshold, and nothing of the line is summed (a NaN in the
 *      line cannot reach thr).  Otherwise S is the sum S1 of steps 1 and 2 of "normalising rows" taken over this one line with n = T:
 *      chunks of 256 frames counted from frame 0, ((d0 + d1) + d2) + d3 per lane, the six-level adjacent-pair tree, the chunk list
 *      folded 64 at a time, all in double.  Then in f32, as Kaldi does after its own double sum:
 *        sf = (float)S;   p = energy_mean_scale * sf;   q = p / (float)T;   thr = energy_threshold + q
 *      where (float)T is the round-to-nearest-even conversion of the uint64.  Each of these is ONE IEEE f32 operation, nothing fused.
 *   2  The raw decision.  d[t] = e[t] > thr, an f32 comparison: a NaN on either side gives 0.
 *   3  The context.  In signed 64-bit integers: lo = max(0, t - frames_context), hi = min(T, t + frames_context + 1), den = hi - lo,
 *      num = the number of d set in [lo, hi).  voiced[t] = (float)num >= (float)den * proportion_threshold, with ONE rounded f32
 *      multiply, as Kaldi's int * BaseFloat does.  The f32 product is part of the contract on purpose:
 *        (den, num) = (5, 3) at 0.6f:   5 * 0.6f rounds to 3.0f, so the frame IS voiced (the exact product is 3.00000012);
 *        (den, num) = (10, 6) at 0.6f:  10 * 0.6f rounds to 6.0f, so the frame IS voiced (the exact product is 6.00000024).
 *      T = 7, frames_context = 2, proportion_threshold 0.6f, d = 1 0 0 1 1 0 1:
 *        t    0      1      2      3      4      5      6
 *        lo   0      0      0      1      2      3      4
 *        hi   3      4      5      6      7      7      7
 *        den  3      4      5      5      5      4      3
 *        num  1      2      3      2      3      3      2
 *        v    0      0      1      0      1      1      1       ((float)den * 0.6f = 1.80000007, 2.4000001, 3.0)
 *   4  The mask.  mask[t] is the byte 1 or 0 for t < T; positions [T, max(T, fill_to[row])) receive 0.  Every such byte is written
 *      exactly once and no other byte of d_mask is written -- a wide store never reaches past the span.  Nothing of d_src at or
 *      beyond T is read, and nothing of any other line.
 *   5  The thresholds.  d_thr, when given, receives thr as one f32 per row and channel, [n_rows][ch], rows with T == 0 included.
 *      Which NaN a NaN thr is, is outside the contract.
 * Against Kaldi: its sum over the line is a sequential double sum, this one a tree.  Both are within a few 2^-53 of the exact sum
 * per addition, which the conversion to f32 nearly always absorbs; where the two thresholds have the same bits, the masks are
 * identical.
 *
 * lw_vad_rows: n_frames and fill_to (may be NULL: nothing is filled) are HOST arrays, copied during the call.  Asynchronous on
 * hip_stream; calls on one object may be queued back to back.  Two forms with the same bits: the contract does not know the grid.
 *   FUSED  ONE kernel launch per 65535 rows, whenever every row's max(T, fill_to) is at most LW_VAD_FUSED_MAX frames (64 chunks, so
 *          the chunk list is ONE tree): a workgroup of 256 lanes takes a tile of lw_vad_tile_frames frames (1024) of a row and
 *          channel, recomputes the line's S itself (at most 64 KiB out of L2) and decides its tile; tile 0 stores d_thr.
 *   SPLIT  THREE launches per 65535 rows for longer rows: the chunk sums into a list the object owns, every row and channel's list
 *          to thr, the decisions.
 * With energy_mean_scale == 0 both are the decide launch alone.  With no byte of the mask to write there is no decide launch; d_thr,
 * when given, is then filled with energy_threshold by a launch of ONE workgroup, which lw_vad_last_launches counts (1; 0 without
 * d_thr or rows).  The raw decisions of a tile and of frames_context frames either side are ballot words in LDS, num is a popcount;
 * mask bytes leave as dwords where the address allows and as bytes at the ragged head and tail of a tile's span.  No atomics, no
 * workgroup waits on another.  A workgroup needs 832 bytes of LDS.
 * lw_vad_threshold: rule 1 behind the sum on the host, from the same source as the kernels'.  lw_vad_voiced: rule 3 on the host, from
 * the same source: 1 or 0, -1 for a NULL object.  lw_vad_set_tile_frames: a test's handle on the seams, a multiple of 256 in 256 ..
 * 2048.  lw_vad_set_route: a test's handle on the two forms; LW_VAD_ROUTE_SPLIT is taken at any length, LW_VAD_ROUTE_FUSED only up to
 * LW_VAD_FUSED_MAX.  lw_vad_last_launches: the kernels the last accepted call queued, -1 = no call yet.
 * Refusals, decided on the host before anything is queued:
 *   LW_ERR_NULL_ARG     v, p or thr NULL, n_frames NULL with rows, d_src NULL with frames to read, d_mask NULL with bytes to write
 *   LW_ERR_UNSUPPORTED  (create) energy_threshold not finite; energy_mean_scale NaN, negative or infinite; frames_context >
 *                       LW_VAD_MAX_CONTEXT; proportion_threshold not strictly inside (0, 1); reserved != 0; (set_tile_frames,
 *                       set_route) a bad value; (rows) LW_VAD_ROUTE_FUSED on a call whose longest max(T, fill_to) exceeds
 *                       LW_VAD_FUSED_MAX
 *   LW_ERR_DEVICE       (create) no such device, or one whose workgroups have less LDS than the kernels need (the device is asked)
 *   LW_ERR_CAPACITY     n_frames[i] or fill_to[i] > frame_capacity, ch == 0 or > 255, F == 0 or > 65535, line >= F, a buffer that 64
 *                       bits of bytes cannot address, more than 2^24 - 1 tiles in a row */
#define LW_VAD_MAX_CONTEXT 256
#define LW_VAD_FUSED_MAX 16384
typedef struct lw_vad lw_vad;
enum { LW_VAD_ROUTE_AUTO = 0, LW_VAD_ROUTE_FUSED = 1, LW_VAD_ROUTE_SPLIT = 2 };
typedef struct {
	float energy_threshold, energy_mean_scale;
	uint32_t frames_context;
	float proportion_threshold;
	uint32_t line, reserved;
} lw_vad_params;
lw_vad *lw_vad_create(int device, const lw_vad_params *p, int *err);
void lw_vad_destroy(lw_vad *v);
int lw_vad_rows(lw_vad *v, uint32_t ch, uint32_t F, const void *d_src, uint8_t *d_mask, float *d_thr, size_t n_rows, size_t frame_capacity,
		const uint64_t *n_frames, const uint64_t *fill_to, void *hip_stream);
int lw_vad_threshold(const lw_vad *v, double S, uint64_t T, float *thr);
int lw_vad_voiced(const lw_vad *v, uint64_t num, uint64_t den);
uint32_t lw_vad_tile_frames(const lw_vad *v);
int lw_vad_set_tile_frames(lw_vad *v, uint32_t tile);
int lw_vad_set_route(lw_vad *v, int route);
int lw_vad_last_launches(const lw_vad *v);

/* ---- frame decisions and frame selection ------------------------------------------------------------------------------------
 * Shortening feature rows by a mask on the GPU, as a pass of its own (k_select): Kaldi's select-voiced-frames for ANY mask -- an
 * energy VAD's, a neural VAD's, a silence trim.  Source and destination are f32 [row][ch][F][frame_capacity], the layout of every
 * stage before it, with the SAME frame_capacity, so no count can overflow a line; the mask is uint8 [row][ch][frame_capacity], one
 * decision per frame of a row and channel (any non-zero byte keeps the frame).  Row i has T = n_frames[i] frames.  For each row
 * and channel:
 *   the kept frames are those t < T with mask[t] != 0, in ascending order: t_0 < .. < t_(K-1);
 *   element j < K of destination line f is a BIT COPY of element t_j of source line f (NaN payloads included);
 *   positions [K, max(T, fill_to[row])) of every destination line receive +0.0.
 * Every position below max(T, fill_to[row]) is therefore written exactly once, and nothing else of d_dst is written.  Nothing of
 * d_src or d_mask at or beyond T is read.  d_counts, when given, receives K as one uint64 per row and channel, [n_rows][ch], rows
 * with T == 0 included.  Any overlap of the buffers is the caller's error.  Integer arithmetic only: there is no order to specify.
 * The channels of a row may end up with different lengths: [B][C][F][cap] viewed as [B * C][1][F][cap] is the same memory, and the
 * counts read as [B * C] are the next pass's n_frames.
 *
 * lw_select_rows: n_frames and fill_to (may be NULL: nothing is filled) are HOST arrays, copied during the call.  Asynchronous on
 * hip_stream; calls on one object may be queued back to back.  TWO kernel launches per 65535 rows: the kept frames of every tile
 * of lw_select_tile_frames frames (1024) of every row and channel are counted into a list the object owns; then every workgroup
 * adds up the list in front of its tile, compacts its tile's kept frames in LDS by an integer prefix sum, copies them for up to 16
 * lines (coalesced writes, a monotone gather of reads) and zeroes its share of the tail.  The count launch is left out when no
 * row has a frame; with nothing to write there is no launch, and d_counts is zeroed by a memset on the stream.  No atomics, no
 * workgroup waits on another.  A workgroup needs 9280 bytes of LDS.  lw_select_set_tile_frames: a test's handle on the seams, a
 * multiple of 256 in 256 .. 2048.  lw_select_last_launches: the kernels the last accepted call queued, -1 = no call yet.
 * Refusals, decided on the host before anything is queued:
 *   LW_ERR_NULL_ARG     se NULL, n_frames NULL with rows, d_src or d_mask NULL with frames to read, d_dst NULL with elements to write
 *   LW_ERR_UNSUPPORTED  (set_tile_frames) a tile that is no multiple of 256 in 256 .. 2048
 *   LW_ERR_DEVICE       (create) no such device, or one whose workgroups have less LDS than the kernel needs (the device is asked)
 *   LW_ERR_CAPACITY     n_frames[i] or fill_to[i] > frame_capacity, ch == 0 or > 255, F == 0 or > 65535, a buffer that 64 bits of
 *                       bytes cannot address, more than 2^24 - 1 workgroups (tiles * groups of 16 lines) in a channel */
typedef struct lw_select lw_select;
lw_select *lw_select_create(int device, int *err);
void lw_select_destroy(lw_select *se);
int lw_select_rows(lw_select *se, uint32_t ch, uint32_t F, const void *d_src, const uint8_t *d_mask, void *d_dst, uint64_t *d_counts,
		size_t n_rows, size_t frame_capacity, const uint64_t *n_frames, const uint64_t *fill_to, void *hip_stream);
uint32_t lw_select_tile_frames(const lw_select *se);
int lw_select_set_tile_frames(lw_select *se, uint32_t tile);
int lw_select_last_launches(const lw_select *se);

/* ---- segments of a frame mask -------------------------------------------------------------------------------------------------
 * Stretches of speech from a frame mask on the GPU, as a pass of its own (k_segment_count, k_segment): the mask is smoothed and
 * turned into (start, end) pairs in the order of pyannote's Binarize -- pad, merge across short gaps, drop short regions; a
 * Kaldi-style hangover is pad_offset alone.  d_mask is uint8 [row][ch][frame_capacity], exactly what lw_vad_rows writes and
 * lw_select_rows reads; any non-zero byte is "set".  Row i has T = n_frames[i] frames; nothing at or beyond T is read.  An object
 * is made from four counts of frames, each at most LW_SEG_MAX_SPAN (10 s at a 10 ms shift).  With m[t] = (mask[t] != 0) on [0, T),
 * for each row and channel, pointwise (nothing outside [0, T) is ever set):
 *   1. pad   P[t] = 1 iff some u in [0, T) has m[u] and t - pad_offset <= u <= t + pad_onset;
 *   2. fill  C[t] = P[t], or there are a < t < b with P[a], P[b] and b - a - 1 < min_off: a gap of fewer than min_off frames
 *            BETWEEN two set frames is filled; a gap that touches either end of the line is not;
 *   3. drop  O[t] = C[t] and the maximal run of C that holds t has at least min_on frames; runs at the line's ends are not exempt;
 *   4. the segments are the maximal runs of O in ascending order, [a_0, b_0) < .. < [a_(K-1), b_(K-1)).
 * With all four counts 0 the segments are the runs of the raw mask.  Worked examples (x = set, . = unset; tests/test_segment_model.py
 * pins them):
 *   min_off = 3:            x..x -> xxxx (a gap of min_off - 1)      x...x -> x...x (a gap of min_off)     x..  -> x.. (an end's gap stays)
 *   min_on = 3:             .xx. -> .... (a run of min_on - 1)       .xxx. -> .xxx.
 *   pad_onset = 2, pad_offset = 1, T = 6:   .....x -> ...xxx   x..... -> xx....   (clamped at 0 and at T)
 *   pad_onset = pad_offset = 1:             .x..x. -> xxxxxx  (the pads meet: one segment)
 *   T = 0: K = 0.  T = 1: x -> one segment [0, 1), unless min_on > 1.  xxxx: [0, T).  ....: K = 0.  x.x.x: K = ceil(T / 2).
 * O[t] depends on m only within H = max(pad_onset, pad_offset) + min_off + min_on <= 3 * LW_SEG_MAX_SPAN frames of t: that bound
 * is what lets a workgroup recompute the rule for its tile from the tile and a halo, and it is the reason for the limit.
 *
 * Outputs, each may be NULL and is then not computed:
 *   d_spans   uint64 [row][ch][seg_capacity][2] receives (a_k, b_k) for k < min(K, seg_capacity); entries at or beyond K are not written;
 *   d_counts  uint64 [row][ch] receives the true K even when K > seg_capacity (how the caller sees the overflow), rows with T == 0 included;
 *   d_smooth  uint8 [row][ch][frame_capacity] receives O[t] as a 0 / 1 byte for t < T and 0 on [T, max(T, fill_to[row])); every byte
 *             of that span is written once, nothing else is: lw_select_rows with a hangover.
 * lw_segment_rows: n_frames and fill_to (may be NULL: nothing is filled) are HOST arrays, copied during the call.  Asynchronous on
 * hip_stream; calls on one object may be queued back to back.  TWO kernel launches per 65535 rows: a workgroup of 256 lanes takes a
 * tile of lw_segment_tile_frames frames (1024), loads it and H + 1 frames either side as ballot words into LDS and recomputes P, C
 * and O there; the first launch counts the segment starts of every tile into a list the object owns, in the second every
 * workgroup adds up the list in front of its tile in 64 bits, ranks its own starts and ends by popcounts (the ends in front of a
 * tile are the starts in front of it, minus one if a run crosses the tile's start) and stores spans, smoothed bytes (four at a 4-byte
 * boundary of the address as one dword, byte by byte at a cut) and, for tile 0, the count.  The count launch is left out when no
 * row has a frame or neither spans nor counts are wanted; with nothing to write there is no launch, and d_counts is zeroed by a
 * memset on the stream.  No atomics, no workgroup waits on another.  A workgroup needs 6176 bytes of LDS.
 * lw_segment_set_tile_frames: a test's handle on the seams, a multiple of 256 in 256 .. 2048 (at 256 the halo covers twelve tiles
 * either side).  lw_segment_last_launches: the kernels the last accepted call queued, -1 = no call yet.
 * Refusals, decided on the host before anything is queued:
 *   LW_ERR_NULL_ARG     sg or p NULL, n_frames NULL with rows, d_mask NULL with frames to read
 *   LW_ERR_UNSUPPORTED  (create) a count above LW_SEG_MAX_SPAN, reserved != 0; (set_tile_frames) a tile that is no multiple of 256 in
 *                       256 .. 2048
 *   LW_ERR_DEVICE       (create) no such device, or one whose workgroups have less LDS than the kernel needs (the device is asked)
 *   LW_ERR_CAPACITY     n_frames[i] or fill_to[i] > frame_capacity, ch == 0 or > 255, seg_capacity == 0 with d_spans given, a buffer
 *                       that 64 bits of bytes cannot address, more than 2^24 - 1 workgroups (tiles) in a channel */
#define LW_SEG_MAX_SPAN 1024
typedef struct lw_segment lw_segment;
typedef struct {
	uint32_t pad_onset;  /* frames a segment starts earlier */
	uint32_t pad_offset; /* frames a segment ends later: the hangover */
	uint32_t min_off;    /* gaps of fewer frames between two set frames are filled */
	uint32_t min_on;     /* runs of fewer frames are dropped */
	uint32_t reserved;   /* 0 */
} lw_segment_params;
lw_segment *lw_segment_create(int device, const lw_segment_params *p, int *err);
void lw_segment_destroy(lw_segment *sg);
int lw_segment_rows(lw_segment *sg, uint32_t ch, const uint8_t *d_mask, uint64_t *d_spans, uint64_t *d_counts, uint8_t *d_smooth, size_t n_rows,
		size_t frame_capacity, size_t seg_capacity, const uint64_t *n_frames, const uint64_t *fill_to, void *hip_stream);
uint32_t lw_segment_tile_frames(const lw_segment *sg);
int lw_segment_set_tile_frames(lw_segment *sg, uint32_t tile);
int lw_segment_last_launches(const lw_segment *sg);

/* ---- cutting rows into segment rows -------------------------------------------------------------------------------------------
 * One output row per segment on the GPU, as a pass of its own (k_cut).  Source and destination are [row][ch][F][capacity] and
 * [n_out][ch][F][out_capacity], elements of elem_bytes in {2, 4}: i16 PCM, f32 PCM or features; a waveform is F = 1.  jobs is a HOST
 * array of n_out triples (row, start, end) in uint64, copied during the call, as are n_frames (one per source row, for the check)
 * and fill_to (one per job; may be NULL: nothing is filled).  For job i with len = end - start, every channel c and line f:
 *   dst[i][c][f][j] is a BIT COPY of src[row][c][f][start + j] for j < len (NaN payloads are kept);
 *   positions [len, max(len, fill_to[i])) receive zero bits;
 * nothing else of d_dst is written, nothing of d_src outside [start, end) of the job's lines is read.  Jobs may overlap in the
 * source and may name a row any number of times; overlap of the buffers is the caller's error.  Both buffers are aligned to
 * elem_bytes.  Asynchronous on hip_stream; calls on one object may be queued back to back.  ONE kernel launch per 65535 jobs: a
 * workgroup takes 16384 destination bytes of one line; the destination leaves in aligned 16-byte stores wherever the line's
 * address allows, the source is read by 16-byte loads at the alignment its start gives it; all addresses in 64 bits.
 * lw_cut_last_launches: the kernels the last accepted call queued, -1 = no call yet.
 * Refusals, decided on the host before anything is queued:
 *   LW_ERR_NULL_ARG     c NULL, n_frames NULL with rows, jobs NULL with jobs, d_src NULL with elements to read, d_dst NULL with
 *                       elements to write
 *   LW_ERR_UNSUPPORTED  elem_bytes not 2 or 4
 *   LW_ERR_DEVICE       (create) no such device
 *   LW_ERR_CAPACITY     row >= n_rows, start > end, end > n_frames[row], n_frames[row] > capacity, len or fill_to[i] > out_capacity,
 *                       ch == 0 or > 255, F == 0 or > 65535, a buffer that 64 bits of bytes cannot address, more than 2^24 - 1
 *                       workgroups (tiles * F) in a channel */
typedef struct lw_cut lw_cut;
lw_cut *lw_cut_create(int device, int *err);
void lw_cut_destroy(lw_cut *c);
int lw_cut_rows(lw_cut *c, uint32_t ch, uint32_t F, uint32_t elem_bytes, const void *d_src, size_t n_rows, size_t capacity, const uint64_t *n_frames,
		const uint64_t *jobs, size_t n_out, void *d_dst, size_t out_capacity, const uint64_t *fill_to, void *hip_stream);
int lw_cut_last_launches(const lw_cut *c);

/* ---- masking feature rows -----------------------------------------------------------------------------------------------------
 * SpecAugment (Park et al. 2019) without its time warp, on the GPU, as a pass of its own (k_specaug): a few time masks and a few
 * frequency masks per utterance, the step every training recipe puts between the normalised features and the model.  Source and
 * destination are f32 [row][ch][F][frame_capacity], the layout of every stage before it; a planar waveform is F = 1, so time
 * masks on waveforms are the same call.  Row i has T = n_frames[i] frames and an id ids[i]; ids is a HOST uint64 array, NULL means
 * id = the row's index.  The library draws its random numbers from a counter-based generator, Philox4x32-10 (Salmon et al., SC'11;
 * lewton_amd/csrc/lw_rng.hpp, plain integer arithmetic, no state): an utterance's masks are a pure function of (seed, id) -- the same
 * in any batch, at any row position, on any grid, and reproducible from a log line that holds the two numbers.
 * A GROUP g is channel c when per_channel is set, else 0: then all channels of a row share their masks.  Mask k of kind d (0 = a
 * time mask over n = T, 1 = a frequency mask over n = F) of group g, all in unsigned 64-bit integers:
 *   x     = philox(counter = (id & 0xffffffff, id >> 32, k | g << 16, d), key = (seed & 0xffffffff, seed >> 32))
 *   W     = min(max_d, n);  for d == 0 and ratio_den != 0:  W = min(W, (n / ratio_den) * ratio_num + ((n % ratio_den) * ratio_num) / ratio_den)
 *   lo    = min(min_d, W)
 *   w     = lo + ((uint64)x[0] * (W - lo + 1) >> 32)
 *   start = the high 64 bits of the 128-bit product ((uint64)x[1] << 32 | x[2]) * (n - w + 1);   end = start + w      (x[3] is not used)
 * Philox: multipliers 0xD2511F53 (on counter word 0) and 0xCD9E8D57 (on word 2), ten rounds, 0x9E3779B9 / 0xBB67AE85 added to the
 * key words before every round but the first; one round maps (c0, c1, c2, c3) to (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^
 * k1, lo(M0 c0)).  Both draws are multiply-high without rejection: biased by at most (W + 1) / 2^32 and (n + 1) / 2^64.
 * Known answers, seed 2024, k = 0, g = 0, widths 0 .. 50:  id 0, T = 3000: [797, 827);  id 1, T = 3000: [1300, 1317);  id 0, a
 * frequency mask of 0 .. 10 over F = 80: [40, 40), an empty mask;  id 7, T = 100, ratio 1/5: [78, 84);  id 7, T = 3, min 5: [0, 3);
 * T = 0: [0, 0);  id 0, T = 2^32 + 2^20 + 5: [1153752137, 1153752167);  id 6099, k = 18, the same T, widths 0 .. 65535:
 * [4294953827, 4294968123), a mask that straddles frame 2^32.
 * The width is drawn first and the start over what it leaves, so a mask lies WHOLLY inside the row: torchaudio's form (mask_along_axis),
 * not WeNet's, which draws the start over the whole row and cuts the mask at the row's end.  ratio_num / ratio_den is torchaudio's p
 * and the upper end of ESPnet's time_mask_width_ratio_range: no time mask is wider than that share of the row's own length.
 * Element (c, f, t) with t < T is MASKED when some time mask of its group has start <= t < end or some frequency mask has start <=
 * f < end; masks may overlap and may be empty.  dst = masked ? fill : src, both sides BIT COPIES: fill's own bits, NaN payloads
 * and -0.0 included.  Positions [T, max(T, fill_to[row])) of every line receive +0.0.  Nothing else of d_dst is written; nothing
 * of d_src at or beyond T is read.  d_src == d_dst is allowed (any other overlap is the caller's error): then only the masked
 * elements and the fill span are written, and nothing is read.  d_spans, when given, receives (start, end) as int64 pairs
 * [n_rows][G][num_t + num_f][2], time masks first, G = ch with per_channel, else 1; rows with T == 0 are included.
 *
 * lw_specaug_rows: n_frames, fill_to (may be NULL: nothing is filled) and ids are HOST arrays, copied during the call.
 * Asynchronous on hip_stream; calls on one object may be queued back to back.  ONE kernel launch per 65535 rows: a workgroup of 256
 * lanes takes a tile of lw_specaug_tile_frames frames (2048) of one line; its first num_t + num_f lanes each draw one mask of the
 * group into LDS (no list travels between launches: the masks are drawn again wherever they are needed), then the tile streams
 * through in groups of four frames, 16-byte loads and stores where the line's address allows and dwords at the ragged head and
 * tail; a group that is all fill is not loaded.  In place a workgroup whose tile meets no mask and no fill span returns without
 * touching memory.  There is no launch without rows or when nothing can be written: out of place no row has a position below
 * max(T, fill_to); in place no masks are configured or no row has a frame, and no row has a fill span; in both cases no d_spans.
 * No atomics, no workgroup waits on another.  A workgroup needs 1024 bytes of LDS.
 * lw_specaug_plan: the rule on the host, from the same source as the kernel's: spans receives the num_t + num_f pairs of one
 * group of an utterance of T frames and F bins.  lw_specaug_set_tile_frames: a test's handle on the seams, a multiple of 256 in
 * 256 .. 2048.  lw_specaug_last_launches: the kernels the last accepted call queued, -1 = no call yet.
 * Refusals, decided on the host before anything is queued:
 *   LW_ERR_NULL_ARG     sa, p or spans NULL, n_frames NULL with rows, d_src NULL with frames to read, d_dst NULL with elements to write
 *   LW_ERR_UNSUPPORTED  (create) min_t > max_t or min_f > max_f; num_t or num_f > LW_SPECAUG_MAX_MASKS; max_t or max_f >
 *                       LW_SPECAUG_MAX_WIDTH; ratio_num > ratio_den; ratio_den > 65535; per_channel not 0 or 1; reserved != 0;
 *                       (set_tile_frames) a tile that is no multiple of 256 in 256 .. 2048
 *   LW_ERR_DEVICE       (create) no such device
 *   LW_ERR_CAPACITY     n_frames[i] or fill_to[i] > frame_capacity, ch == 0 or > 255, F == 0 or > 65535, a buffer that 64 bits of
 *                       bytes cannot address, more than 2^24 - 1 workgroups (tiles * F) in a channel; (plan) group or F > 65535,
 *                       T > 2^63 - 1 (its spans are int64) */
#define LW_SPECAUG_MAX_MASKS 32    /* per kind */
#define LW_SPECAUG_MAX_WIDTH 65535 /* frames or bins of one mask */
typedef struct lw_specaug lw_specaug;
typedef struct {
	uint64_t seed;
	uint32_t num_t, min_t, max_t; /* time masks: how many, and the least and the largest width in frames */
	uint32_t ratio_num, ratio_den; /* ... none wider than ratio_num / ratio_den of the row's frames; ratio_den 0: no such limit */
	uint32_t num_f, min_f, max_f; /* frequency masks, in bins */
	uint32_t per_channel;         /* 1: every channel draws masks of its own */
	float fill;                   /* what a masked element receives, bit for bit */
	uint32_t reserved;            /* 0 */
} lw_specaug_params;
lw_specaug *lw_specaug_create(int device, const lw_specaug_params *p, int *err);
void lw_specaug_destroy(lw_specaug *sa);
int lw_specaug_rows(lw_specaug *sa, uint32_t ch, uint32_t F, const void *d_src, void *d_dst, size_t n_rows, size_t frame_capacity,
		const uint64_t *n_frames, const uint64_t *fill_to, const uint64_t *ids, int64_t *d_spans, void *hip_stream);
int lw_specaug_plan(const lw_specaug *sa, uint64_t id, uint32_t group, uint64_t T, uint32_t F, int64_t *spans);
uint32_t lw_specaug_tile_frames(const lw_specaug *sa);
int lw_specaug_set_tile_frames(lw_specaug *sa, uint32_t tile);
int lw_specaug_last_launches(const lw_specaug *sa);

/* ---- staging ring (BASELINE north_star: "pinned hipMemcpyAsync staging ring so entropy decode of packet N+1 overlaps
 * GPU synthesis of packet N") ------------------------------------------------------------------------------------------
 * A ring of `slots` staging slots on the decoder's device; a slot = one batch object (pinned records + device mirror), a device
 * PCM buffer, a pinned host PCM buffer, a HIP stream.  Slots are used first-in first-out:
 *   lw_ring_stage    host entropy stage of `n` packets into the next free slot (what lw_batch_entropy does);
 *                    LW_ERR_CAPACITY when every slot is in flight (collect + release first) or n > max_packets
 *   lw_ring_launch   queues, for the oldest staged slot and without waiting: H2D of its records, the synthesis kernels
 *                    (ordered behind the previous launch's kernels: consecutive batches may carry the same streams'
 *                    window state) and D2H of the PCM into the slot's pinned buffer
 *   lw_ring_submit   = stage + launch: returns while the GPU works, so the next submit's entropy decode overlaps it
 *   lw_ring_collect  waits for the oldest launched slot; results / PCM stay valid until lw_ring_release.  LW_ERR_DEVICE with
 *                    the slot collected all the same (release it as usual): lw_batch_device_status of that batch
 *   lw_ring_release  frees that slot
 *   lw_ring_drain    waits for everything in flight and frees all slots (their results are dropped)
 * stage may run on another thread than launch / collect / release (one thread each).  Every PreviousWindowRight sees its
 * packets in submission order.  The reference has no counterpart (it decodes one packet per call, audio.rs:919); callers
 * that want its call-by-call semantics use lw_read_audio_packet or the Ogg stream layer below, which runs on this ring. */
typedef struct lw_ring lw_ring;
lw_ring *lw_ring_create(lw_decoder *d, size_t slots, size_t max_packets, int fmt, int *err);
void lw_ring_destroy(lw_ring *r);
int lw_ring_stage(lw_ring *r, const lw_packet *pkts, size_t n, int n_threads);
int lw_ring_launch(lw_ring *r);
int lw_ring_submit(lw_ring *r, const lw_packet *pkts, size_t n, int n_threads);
int lw_ring_collect(lw_ring *r, const lw_packet_result **results, size_t *n, const void **pcm, size_t *pcm_elems);
int lw_ring_release(lw_ring *r);
int lw_ring_drain(lw_ring *r);
size_t lw_ring_slots(const lw_ring *r);
size_t lw_ring_in_flight(lw_ring *r); /* slots staged, launched or collected and not yet released */
size_t lw_ring_last_staged_elems(lw_ring *r); /* elements the batch staged last will produce (known after lw_ring_stage) */
int lw_ring_set_entropy_on_device(lw_ring *r, int on); /* lw_batch_set_entropy_on_device for every slot (ring must be idle) */
const char *lw_ring_last_kernels(const lw_ring *r);
/* measurement hook, process-wide, read by lw_ring_create: -1 (default) = by the ring's decoder -- a tenant's ring
 * (lw_decoder_set_cu_share) runs its launches' kernels one launch after the other, and its PCM copies are issued by one copier
 * thread per device once their kernels have finished (a copy queued behind its kernels blocks the copy engine for the other
 * tenants' ready copies); else bit 0 = kernels in launch order per ring, bit 1 = copies by the device's copier */
void lw_debug_ring_policy(int bits);
/* The host half of a PreviousWindowRight (whether a right part is stored, its length, which of the two device buffers
 * holds it).  lw_batch_entropy / lw_ring_stage advance it when they plan a batch; a caller that drops a staged batch (or
 * one launched batch: a launch writes the OTHER device buffer) restores the state it saved before staging. */
typedef struct {
	uint8_t present, parity;
	uint32_t len;
} lw_pwr_state;
void lw_pwr_get_state(const lw_pwr *p, lw_pwr_state *out);
void lw_pwr_set_state(lw_pwr *p, const lw_pwr_state *in);
int lw_decoder_device(const lw_decoder *d);
/* Several decoders on ONE GPU (tenants; nothing in the reference corresponds: lewton decodes one stream on one thread).
 * lw_decoder_set_shared_device(d, 1): other decoders' rings run on d's GPU as well.  The rings created for d AFTERWARDS then hand
 * their PCM copies to one copier thread per device, which issues each copy once its kernels have finished -- a copy queued
 * behind its kernels blocks the copy engine for every other ring's ready copies (measured: two rings on one GPU 8.6-9.0 M
 * packets/s, with the copier 11.1-12.4 M, the rate of one ring) -- and run their launches' kernels in launch order.
 * lw_sharder_create does this by itself when devices[] names a device several times.
 * lw_decoder_set_cu_share: in addition, decoder `part` of `parts` launches on the slice [32 part / parts, 32 (part + 1) / parts)
 * of the 32 CUs of EVERY XCD only (a HIP queue has to keep CUs on all eight; tenants share the L2s, never a CU): the rings
 * created AFTERWARDS launch on CU-masked HIP streams and its batches are planned for that many CUs; parts = 1 gives the device
 * back.  The wave-pipeline kernels take whole compute units, so without a share a 15 us launch next to another tenant's
 * long-running kernel waits for CUs to drain (130-700 us measured; 28 us flat on a half-device share).  Throughput is the
 * same either way (the PCIe link is the bound), so the sharder leaves it off.  Batches launched on a caller's own stream
 * (lw_batch_synth) are planned for the share but run wherever that stream runs.  LW_ERR_UNSUPPORTED: parts > 32.
 * LW_ERR_UNSUPPORTED also: a device that is not the one the mask layout was measured on (gfx950, eight XCDs of equally many CUs).
 * The two kinds of tenant stream never meet in one process.  With the HIP runtime this was measured on (ROCm 7.2) a process that
 * had BOTH copied on the copier's own stream (the ring of a flagged decoder without a share) AND run CU-masked streams was seen
 * not to exit, one run in three.  The library therefore keeps a latch per device and process:
 *   - once a ring has made the copier's own stream on a device, lw_decoder_set_cu_share(parts > 1) on that device and
 *     lw_ring_create for a decoder that already has a share return LW_ERR_UNSUPPORTED;
 *   - once a CU-masked stream exists on a device, the copier of later rings issues their copies on the slots' own streams
 *     instead of a stream of its own (the same results; 9-10 instead of 11-12 M packets/s for two tenants).
 * A deployment picks one of the two modes per process: CU shares for tenants, or none. */
int lw_decoder_set_shared_device(lw_decoder *d, int on);
int lw_decoder_set_cu_share(lw_decoder *d, unsigned part, unsigned parts);
int lw_decoder_cu_count(const lw_decoder *d); /* compute units this decoder's launches are planned for */
int lw_decoder_device_cu_count(const lw_decoder *d); /* compute units of its device */
size_t lw_decoder_max_block_elems(const lw_decoder *d); /* channels * (3 n1 - n0) / 4: the largest block a packet yields */

/* ---- independent streams sharded over the GPUs of a node, one process (BASELINE configs[4]) ----------------
 * Streams never exchange data (audio.rs:919 touches only its own pwr): shard g owns the streams with stream_id mod G == g.
 * A shard = one lw_decoder on devices[g] (tables + the state pool of its streams in that GPU's HBM), one batch with pinned
 * staging, one HIP stream, one worker thread.  devices[] may name a device several times (logical shards).
 * A shard runs on a staging ring of its own (lw_ring_*: pinned records and pinned PCM per slot).
 * lw_sharder_submit takes packets of any streams (those of one stream in stream order), has every shard run the host
 * entropy stage of its packets and queue H2D, kernels and D2H on the shard's own thread and device, all shards at once,
 * and returns when every shard has launched -- while the GPUs work (no collective, nothing crosses xGMI).  The packet
 * bytes are consumed when it returns.  *out_elems = elements the call will produce.  Up to 3 calls may be in flight, so
 * the host stage of call k+1 overlaps the GPU work of call k on every device.
 * lw_sharder_collect waits for the OLDEST call: out = host memory for cap_elems elements (NULL: drop the samples); results[i] (status, n_samples,
 * out_offset = element offset of packet i's block in out) come back in the order of that call's pkts; blocks are laid out
 * shard by shard.  LW_ERR_CAPACITY: more than max_packets_per_shard packets for one shard, three calls already in flight
 * (submit), nothing in flight or out too small (collect).
 * Which returns of lw_sharder_collect consume the call: LW_ERR_CAPACITY and LW_ERR_NULL_ARG come from the argument checks and
 * consume NOTHING (call again); every other return -- LW_OK, or the error of a shard (LW_ERR_DEVICE) -- has taken the call out
 * of the queue and freed its slots; the packets of a shard that failed carry LW_ERR_DEVICE in results[].  A shard whose ring
 * saw a device error is started over (drained): EVERY part that was in flight on that shard at that moment -- of older calls and
 * of newer ones already submitted (up to two) -- reports LW_ERR_DEVICE when it is collected; calls submitted after the drain run
 * normally.  The dropped batches had already advanced the host halves of their streams' window states, so the drain resets the
 * PreviousWindowRight of every stream opened on that shard (lw_sharder_stream_reset): the first packet of each of them after the
 * failure yields 0 samples (audio.rs:1140-1152), never samples overlapped with a stale right part.
 * A submit that fails AFTER some shards have launched (a device error on one shard) still queues the call, so that the
 * slots those shards hold can be freed: collect it (its packets on the failed shard come back with LW_ERR_DEVICE).
 * lw_sharder_decode = submit + collect on an empty pipeline.
 * Logical shards (a device named several times) are tenants of that GPU (lw_decoder_set_shared_device): their PCM copies go
 * through the device's copier thread, ready copies only, one at a time.
 * The process-per-GPU form of the same rule is lewton_amd/shard.py + bench.py under torch.distributed.run. */
typedef struct lw_sharder lw_sharder;
typedef struct lw_shard_stream lw_shard_stream; /* one logical stream: its PreviousWindowRight lives on the owning shard */
typedef struct {
	lw_shard_stream *stream;
	const uint8_t *data;
	size_t len;
} lw_shard_packet;
lw_sharder *lw_sharder_create(const lw_ident *id, const lw_setup *setup, const int *devices, size_t n_shards,
		size_t max_packets_per_shard, int fmt, int *err);
void lw_sharder_destroy(lw_sharder *sh); /* close the streams first */
size_t lw_sharder_shards(const lw_sharder *sh);
int lw_sharder_shard_cus(const lw_sharder *sh, size_t shard); /* compute units shard's launches run on (its lw_decoder_cu_count) */
/* measurement hook, process-wide, read by lw_sharder_create: 1 = logical shards of one device also get a CU share each
 * (lw_decoder_set_cu_share); 0 (default) = they share all its CUs */
void lw_debug_sharder_share_cus(int on);
int lw_sharder_set_entropy_on_device(lw_sharder *sh, int on); /* every shard's entropy stage on its own GPU (k_entropy) */
size_t lw_sharder_shard_of(const lw_sharder *sh, uint64_t stream_id);
int lw_sharder_device_of(const lw_sharder *sh, size_t shard);
lw_shard_stream *lw_sharder_stream_open(lw_sharder *sh, uint64_t stream_id);
void lw_sharder_stream_close(lw_shard_stream *st);
void lw_sharder_stream_reset(lw_shard_stream *st); /* `pwr = PreviousWindowRight::new()` */
int lw_sharder_decode(lw_sharder *sh, const lw_shard_packet *pkts, size_t n, int n_threads_per_shard, void *out,
		size_t cap_elems, lw_packet_result *results);
int lw_sharder_submit(lw_sharder *sh, const lw_shard_packet *pkts, size_t n, int n_threads_per_shard, size_t *out_elems);
int lw_sharder_collect(lw_sharder *sh, void *out, size_t cap_elems, lw_packet_result *results, size_t n_results);
size_t lw_sharder_in_flight(lw_sharder *sh); /* calls submitted and not yet collected */
/* Zero-copy form of collect: the oldest call's PCM stays where the GPUs' copy engines put it, in the shards' pinned ring
 * buffers -- pcm[g] / elems[g] for shard g (arrays of lw_sharder_shards() entries); results[i].out_offset is relative to
 * the block of the shard that owns packet i (lw_sharder_shard_of).  Valid until lw_sharder_release, which frees the slots.
 * Both run on the caller's thread (no hand-over to the shards' workers) and leave the caller's current HIP device as they found
 * it.  After ANY return of lw_sharder_collect_pinned other
 * than LW_ERR_CAPACITY / LW_ERR_NULL_ARG the call is held by the caller: lw_sharder_release takes it out of the queue. */
int lw_sharder_collect_pinned(lw_sharder *sh, lw_packet_result *results, size_t n_results, const void **pcm, size_t *elems);
int lw_sharder_release(lw_sharder *sh);

/* ---- Ogg container either side of the path ---------------------------- */
/* lewton reads Ogg through the external crate `ogg` 0.8.0 (Cargo.lock; `PacketReader`, `Packet`) and wraps it
 * in src/inside_ogg.rs.  The functions below replace both: a page/packet demultiplexer after RFC 3533 with the
 * packet attributes lewton's call sites use, and `OggStreamReader` with the device decode behind it. */
enum {
	LW_OGG_EOF = 48,                     /* Ok(None): clean end of the physical stream */
	/* ogg::OggReadError */
	LW_OGG_NO_CAPTURE_PATTERN = 49,      /* NoCapturePatternFound */
	LW_OGG_INVALID_STREAM_STRUCT_VER = 50, /* InvalidStreamStructVer(u8) */
	LW_OGG_HASH_MISMATCH = 51,           /* HashMismatch(u32, u32) */
	LW_OGG_READ_ERROR = 52,              /* ReadError(io::Error), incl. UnexpectedEof inside a page / read_packet_expected */
	LW_OGG_INVALID_DATA = 53             /* InvalidData */
};

typedef struct lw_ogg_reader lw_ogg_reader; /* ogg::PacketReader<T: Read + Seek> */
typedef struct lw_ogg_stream lw_ogg_stream; /* OggStreamReader<T>, src/inside_ogg.rs:66-77 */

typedef struct {                 /* the `T: Read + Seek` of the reference as C callbacks */
	int64_t (*read)(void *user, uint8_t *dst, size_t n);       /* bytes read (0 = end), < 0 = error */
	int64_t (*seek)(void *user, int64_t offset, int whence);   /* whence 0/1/2 = SEEK_SET/CUR/END; new position or < 0 */
	void *user;
} lw_ogg_io;

typedef struct {                 /* ogg::Packet */
	const uint8_t *data;         /* owned by the reader, valid until its next call */
	size_t len;
	uint32_t stream_serial;      /* Packet::stream_serial() */
	uint64_t absgp_page;         /* Packet::absgp_page(): granule position of the page the packet ended on */
	uint8_t first_in_stream;     /* Packet::first_in_stream(): first packet of a page with the begin-of-stream flag */
	uint8_t last_in_stream;      /* Packet::last_in_stream(): last packet of a page with the end-of-stream flag */
	uint8_t first_in_page;       /* Packet::first_in_page() */
	uint8_t last_in_page;        /* Packet::last_in_page() */
} lw_ogg_packet;

/* PacketReader::new(rdr).  open_memory borrows `data` unless copy != 0. */
lw_ogg_reader *lw_ogg_reader_open_memory(const uint8_t *data, size_t len, int copy);
lw_ogg_reader *lw_ogg_reader_open_file(const char *path, int *err);
lw_ogg_reader *lw_ogg_reader_open_io(const lw_ogg_io *io);
void lw_ogg_reader_close(lw_ogg_reader *r);
/* PacketReader::read_packet: LW_OK + *out, LW_OGG_EOF, or an OggReadError code.  Streams may be multiplexed. */
int lw_ogg_read_packet(lw_ogg_reader *r, lw_ogg_packet *out);
/* PacketReader::read_packet_expected: end of stream is LW_OGG_READ_ERROR (UnexpectedEof) */
int lw_ogg_read_packet_expected(lw_ogg_reader *r, lw_ogg_packet *out);
/* PacketReader::delete_unread_packets (inside_ogg.rs:47) */
void lw_ogg_delete_unread_packets(lw_ogg_reader *r);
/* PacketReader::seek_absgp(stream_serial, absgp) with page granularity (inside_ogg.rs:307-313): reading resumes behind
 * the LAST page of the stream (any stream when has_serial == 0) that completes a packet and whose granule position
 * is <= absgp -- at the start of the physical stream if there is none -- so the position reached is <= absgp.
 * Bisection over the byte range, then a linear scan of the last interval. */
int lw_ogg_seek_absgp(lw_ogg_reader *r, int has_serial, uint32_t serial, uint64_t absgp);
/* CRC of RFC 3533 (polynomial 0x04c11db7, initial 0, no reflection) -- exposed for muxers and tests */
uint32_t lw_ogg_crc32(const uint8_t *data, size_t len, uint32_t crc);

/* OggStreamReader::from_ogg_reader (inside_ogg.rs:100-113) = read_headers (:30-49) + an empty PreviousWindowRight.
 * Takes ownership of `r` (also on failure).  The device context is created on `device` at the first decode, so
 * opening and header access work without a GPU.  *err: HeaderReadError / OggReadError code. */
lw_ogg_stream *lw_ogg_stream_open(lw_ogg_reader *r, int device, int *err);
void lw_ogg_stream_close(lw_ogg_stream *s);
/* pub fields ident_hdr / comment_hdr / setup_hdr (:72-74); owned by the stream, replaced at a chain boundary */
const lw_ident *lw_ogg_stream_ident(const lw_ogg_stream *s);
const lw_comment *lw_ogg_stream_comment(const lw_ogg_stream *s);
const lw_setup *lw_ogg_stream_setup(const lw_ogg_stream *s);
uint32_t lw_ogg_stream_serial(const lw_ogg_stream *s);                  /* stream_serial(), :288-290 */
uint32_t lw_ogg_stream_link_index(const lw_ogg_stream *s);              /* chain boundaries crossed so far (0 = first link) */
int lw_ogg_stream_last_absgp(const lw_ogg_stream *s, uint64_t *absgp); /* get_last_absgp(), :296-298: 1 = Some */
/* read_dec_packet_generic<S> (:195-206; read_dec_packet :167, read_dec_packet_itl :183): decodes the next audio
 * packet of the logical stream (chained streams re-initialise the context and prime it with their first audio
 * packet, :120-151), truncates the last packet of the stream to the final granule position (:219-227) and tracks
 * cur_absgp.  out: host memory for cap_elems elements, filled planar [ch][*n_samples] packed or interleaved.  LW_OK,
 * LW_OGG_EOF (Ok(None)), or a VorbisError: AudioReadError (BadAudio), HeaderReadError (BadHeader), OggReadError
 * (OggError) code.  LW_ERR_CAPACITY: cap_elems < channels << blocksize_1 of the CURRENT logical stream (it may just have
 * changed at a chain boundary: re-read lw_ogg_stream_ident); the packet is kept for the next call. */
int lw_ogg_stream_read_dec_packet(lw_ogg_stream *s, int fmt, void *out, size_t cap_elems, size_t *n_samples);
/* Look-ahead queue (the batched form of the call above): reads up to max_packets audio
 * packets of the current logical stream, decodes them with ONE batch (host entropy threads + one set of kernel
 * launches) and applies the same truncation / granule bookkeeping packet by packet.  out receives the packets'
 * blocks back to back; n_samples[i] / status[i] per packet (a packet that fails to decode has its AudioReadError in
 * status[i] and no samples).  Stops early at the end of the stream and in front of a chain boundary.
 * Returns LW_OK (also with *n_packets == 0 in front of a chain boundary: call lw_ogg_stream_read_dec_packet),
 * LW_OGG_EOF when no packet is left, or an error.
 * THREADING AND READ-AHEAD CONTRACT.  From the first call on the stream runs two library threads (a demultiplexer and an
 * entropy-staging thread) that keep reading the source through the reader's lw_ogg_io callbacks BETWEEN calls and after
 * a call has returned, holding up to about 5 x max_packets packets ahead of what the caller has been handed.  Hence:
 * (1) the io callbacks are invoked on library threads, never concurrently with each other, but concurrently with the
 * caller's own code -- they must not share unsynchronised state with it; (2) the position of the underlying source
 * between calls is unspecified (ahead of the last delivered packet); (3) every other entry point of the stream
 * (read_dec_packet, skip_samples_linear, seek_absgp_pg, into_inner, set_entropy_on_device, close) first stops both
 * threads and rolls the stream back to exactly what the caller has been handed, so the sequence of packets, errors
 * and samples is the one the packet-by-packet calls produce; (4) a device failure on the staging thread is reported
 * by the next call on the caller's thread, with its text republished through lw_last_device_error(). */
int lw_ogg_stream_read_dec_packets(lw_ogg_stream *s, int fmt, size_t max_packets, int n_threads, void *out,
		size_t cap_elems, uint32_t *n_samples, int32_t *status, size_t *n_packets);
/* Read-ahead behind the packet-by-packet call: with max_packets > 0, lw_ogg_stream_read_dec_packet hands out, one per call, the
 * packets of batches of up to max_packets that the look-ahead pipeline above decodes (n_threads host entropy threads; the entropy
 * stage on the device if set) -- the reference's own loop `while let Some(p) = rdr.read_dec_packet()? { .. }` (examples/perf.rs:35-44)
 * at the batched rate instead of one synchronous GPU round trip per packet, with no change to the loop.  What the caller observes is
 * the packet-by-packet sequence, call for call: samples, AudioReadError codes at the packets they belong to, get_last_absgp() as of
 * the packet just handed out, the last packet's truncation, LW_OGG_EOF, chain boundaries (crossed by the call itself).  Every other
 * entry point first returns the packets not yet handed out and re-makes the PreviousWindowRight as of the last one that was (one
 * synchronous decode of that packet: a decoded packet's right half depends on nothing before it, audio.rs:1125-1138).
 * A served batch's samples stay in the staging ring's pinned memory and are copied once, into the caller's buffer, at the call.
 * The threading and read-ahead contract above applies from the first call on.  0 turns it off (the default); more than 65 536
 * packets: LW_ERR_CAPACITY. */
int lw_ogg_stream_set_read_ahead(lw_ogg_stream *s, size_t max_packets, int n_threads);
/* Look-ahead batches with the entropy stage on the device (lw_ring_set_entropy_on_device) whenever the current logical
 * stream is eligible; other streams (and the packet-by-packet call) keep the host stage.  Results are identical. */
int lw_ogg_stream_set_entropy_on_device(lw_ogg_stream *s, int on);
/* skip_samples_linear<S> (:244-283): *got_packet = 0 is (None, left); otherwise the decoded packet that contains the
 * target is in out and *left samples of it remain to be skipped.  LW_ERR_CAPACITY as above: call again with
 * to_skip = *left and a buffer for the current logical stream. */
int lw_ogg_stream_skip_samples_linear(lw_ogg_stream *s, size_t to_skip, int fmt, void *out, size_t cap_elems,
		size_t *n_samples, size_t *left, int *got_packet);
/* seek_absgp_pg (:307-313) */
int lw_ogg_stream_seek_absgp_pg(lw_ogg_stream *s, uint64_t absgp);
/* into_inner (:111-113): gives the reader back and destroys the stream object */
lw_ogg_reader *lw_ogg_stream_into_inner(lw_ogg_stream *s);

/* Test hook for the host Huffman decoder (spec 3.2.1 codeword assignment; src/huffman_tree.rs:183-221):
 * returns 0 valid, 1 overspecified, 2 underpopulated, 3 invalid single entry; when valid and bits != NULL
 * decodes up to max_syms symbols. */
int lw_huffman_check(const uint8_t *lengths, size_t n_entries, const uint8_t *bits, size_t bits_len,
		uint32_t *syms, size_t max_syms, size_t *n_syms);

/* Test hook: run the device IMDCT (src/imdct.rs:291) of block size blocksize_0 (blockflag 0) or blocksize_1
 * (blockflag 1) on `spectrum` (n/2 floats) and return the n time-domain values.  Implemented as a packet
 * record with a unit floor (inverse-dB index 255 = 1.0) through the generic kernels. */
int lw_debug_imdct(lw_decoder *d, int blockflag, const float *spectrum, float *out);

/* Test hook (host only): the LDS table image of the specialised long-block kernel and its 16 section
 * offsets (order of struct LwFastImage in csrc/lw_fast.hpp).  Returns the image size in bytes, 0 if the
 * stream shape is not covered by that kernel; copies min(size, cap) bytes. */
size_t lw_debug_fast_image(const lw_ident *id, const lw_setup *s, uint8_t *dst, size_t cap, uint32_t *offsets16);
/* The same for the block kernel k_short<L> (L = lanes per block = block size / 32; section offsets: LwBlkLayout<L> in
 * csrc/lw_fast.hpp) and its unit list (8 bytes per unit: channel a, channel b or -1, coupled, floor slot a / b, post count
 * a / b, 0).  blockflag 0: the short blocks; 1: the long blocks of a stream k_long does not cover.  *n_units: in = room in
 * units8, out = units of the stream.  0 if those blocks are not covered. */
size_t lw_debug_short_image(const lw_ident *id, const lw_setup *s, int blockflag, uint8_t *dst, size_t cap, uint8_t *units8,
		size_t *n_units, uint32_t *lanes);

/* Census hook (host only, no GPU needed): which synthesis kernels the blocks of this stream shape are routed to, and the reason
 * where a faster one does not apply, as one line of text: "long=<kernel> | short=<kernel> | transitions=<how long blocks with a short
 * slope are done> | entropy=<device | host (why)>".  Returns the length of the whole text; copies at most cap - 1 characters. */
size_t lw_debug_plan_census(const lw_ident *id, const lw_setup *s, char *dst, size_t cap);

/* Library/version introspection */
const char *lw_version(void);
/* Host threads the entropy stage uses when a call passes n_threads <= 0: the CPUs this process may run on (hardware
 * threads, cut to the affinity mask and to the container's CFS quota, cgroup cpu.max); LW_HOST_THREADS overrides. */
int lw_default_host_threads(void);

#ifdef __cplusplus
}
#endif
#endif
