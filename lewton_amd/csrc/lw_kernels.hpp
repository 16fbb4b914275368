// Device-side tables and kernel launchers of the audio-packet synthesis path (gfx950).
#pragma once

#include "lw_records.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>
#include <type_traits>

// hipFuncSetAttribute is per DEVICE, and launchers are entered from several host threads (one decoder per GPU in one
// process; the sharder's workers; the Ogg staging thread next to the caller): `run(set)` calls
// `set` exactly once per (kernel family, current device) -- under the mutex, so that a second thread on the same device
// cannot launch before the attributes are in place -- and marks the device done only when it succeeded.
struct LwPerDeviceOnce {
	std::mutex mu;
	uint64_t done[4] = {0, 0, 0, 0}; // one bit per device ordinal
	template <class Set> hipError_t run(Set &&set)
	{
		int dev = 0;
		if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 256)
			return set(); // unknown ordinal: set the attributes every time (cheap, idempotent)
		std::lock_guard<std::mutex> g(mu);
		if (done[dev >> 6] & (1ull << (dev & 63)))
			return hipSuccess;
		const hipError_t e = set();
		if (e == hipSuccess)
			done[dev >> 6] |= 1ull << (dev & 63); // (a failure leaves the bit clear: the next launch tries again)
		return e;
	}
};

// Kernel launch that RETURNS the launch status (hipLaunchKernelGGL drops it; hipGetLastError would also pick up an earlier
// hipErrorNotReady of a polled event): the arguments are passed by address, in the kernel's parameter order -- and hipLaunchKernel
// reads sizeof(parameter) bytes behind each address, so every argument must BE the parameter's type (a bool or a size_t handed in
// for an int parameter would be read as garbage without a diagnostic): checked against the kernel's signature at compile time.
template <class... P, class... A>
static inline hipError_t lw_launch_k(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t st, A &...a)
{
	static_assert(sizeof...(P) == sizeof...(A), "lw_launch_k: one argument per kernel parameter");
	static_assert((std::is_same<typename std::remove_cv<A>::type, typename std::remove_cv<P>::type>::value && ...),
			"lw_launch_k: every argument must have exactly its kernel parameter's type");
	void *args[] = {(void *)&a...};
	return hipLaunchKernel((const void *)kernel, grid, block, args, lds, st);
}

// CachedBlocksizeDerived (header_cached.rs:19-110) in HBM; computed on the host, never on the device.
struct LwDevBs {
	const float *A, *B, *C, *window;
	const uint32_t *bitrev;
	uint32_t bs, n;
};

#define LW_XSTRIDE 66 // u16 entries per floor in floor_x (LW_MAX_POSTS + 1)

struct LwDevTables {
	LwDevBs bs[2];
	const float *inv_db;          // FLOOR1_INVERSE_DB_TABLE, audio.rs:437-501
	const uint16_t *floor_x;      // [n_floors][LW_XSTRIDE] ascending x of each floor-1 config (header.rs:887-889)
	const uint8_t *floor_F;       // [n_floors] post count
	const uint8_t *mode_floor;    // [n_modes][ch] floor index of each channel (mapping_mux -> submap floor)
	const uint16_t *couple_off;   // [n_modes + 1] offsets (in steps) into `couple`
	const uint8_t *couple;        // (magnitude, angle) channel pairs in header order (audio.rs:990-1002 walks them reversed)
	const uint8_t *sid;           // fast path: [n_floors][2][n_max/2] static interval index per bin (may be null)
	const int8_t *mode_partner;   // [n_modes][ch] the other channel of the ONE coupling step this channel is in, or -1
	const uint8_t *mode_role;     // [n_modes][ch] 1 = magnitude, 2 = angle of that step
	uint32_t pair_coupling;       // 1: in every mode a channel takes part in at most one coupling step (the two tables are valid)
	uint32_t ch, fstride, n_modes, n_floors;
	uint32_t state_stride;        // floats per (slot, parity): ch * (n1 / 2)
	uint32_t state_chan_stride;   // n1 / 2
};

// generic kernels: blocks up to 2^LW_SMALL_BS points are transformed by ONE wave each (four per workgroup), larger ones by
// a 256-thread workgroup (host: lw_runtime.cpp builds one task list per class)
#define LW_SMALL_BS 9

// Kernel-internal sample formats (the `fmt` argument of the launchers; the host maps the public LW_FMT_* onto them,
// lw_kernel_fmt in lw_internal.hpp).  The launchers take 0, 1, 2 and 4 (lw_with_out_fmt); 3 and 5 are the stereo unit forms,
// the interleaved formats of a 2-channel stream whose channels form ONE unit (a coupled pair), that only k_long's launcher chooses.
enum LwOutFmt {
	LW_OUT_I16_PLANAR = 0,
	LW_OUT_I16_INTERLEAVED = 1,
	LW_OUT_F32_PLANAR = 2,
	LW_OUT_I16_ITL_STEREO = 3,
	LW_OUT_F32_INTERLEAVED = 4,
	LW_OUT_F32_ITL_STEREO = 5
};

// f32 samples (no conversion), and the generic interleaved stores (element i of channel c at i * ch + c)
__host__ __device__ constexpr bool lw_out_f32(int f)
{
	return f == LW_OUT_F32_PLANAR || f == LW_OUT_F32_INTERLEAVED || f == LW_OUT_F32_ITL_STEREO;
}
__host__ __device__ constexpr bool lw_out_itl(int f)
{
	return f == LW_OUT_I16_INTERLEAVED || f == LW_OUT_F32_INTERLEAVED;
}
// the generic format of a stereo unit form (the kernel variants without one: PRE, SPLIT, EDGE)
__host__ __device__ constexpr int lw_out_unit_free(int f)
{
	return f == LW_OUT_I16_ITL_STEREO ? LW_OUT_I16_INTERLEAVED : f == LW_OUT_F32_ITL_STEREO ? LW_OUT_F32_INTERLEAVED : f;
}

// The one place where a launcher's runtime `fmt` becomes a template argument: fn(std::integral_constant<int, FMT>{}) for the four
// tags a launcher takes, hipErrorInvalidValue for any other value.
template <class Fn>
static inline hipError_t lw_with_out_fmt(int fmt, Fn &&fn)
{
	switch (fmt) {
	case LW_OUT_I16_PLANAR:
		return fn(std::integral_constant<int, LW_OUT_I16_PLANAR>{});
	case LW_OUT_I16_INTERLEAVED:
		return fn(std::integral_constant<int, LW_OUT_I16_INTERLEAVED>{});
	case LW_OUT_F32_INTERLEAVED:
		return fn(std::integral_constant<int, LW_OUT_F32_INTERLEAVED>{});
	case LW_OUT_F32_PLANAR:
		return fn(std::integral_constant<int, LW_OUT_F32_PLANAR>{});
	}
	return hipErrorInvalidValue;
}

struct LwBatchDev {
	const LwPacketRec *recs;
	const uint16_t *floors;
	const float *residue;
	const float *fcurve; // explicit floor curves (floor 0), layout of residue; nullptr when the setup has none
	float *decoupled; // scratch [same layout as residue]
	float *td;        // scratch: per packet [ch][n] time-domain blocks at float offset 2 * res_off
	float *state;     // state pool [slots][2][ch][n1/2]
	uint32_t n_packets;
	// packets the generic kernels work on, by block-size class; nullptr = every packet (filters inside the kernels)
	const uint32_t *gen_small, *gen_large;
	uint32_t n_gen_small, n_gen_large;
	const uint32_t *gen_ola; // packets of k_ola_generic: the two lists above plus the LW_RF_TDONLY packets
	uint32_t n_gen_ola;
	const LwOlaDesc *ola;    // one descriptor per entry of gen_ola (null: k_ola_generic reads the records)
	const LwGenTask *gen_tasks; // [n_gen_small * ch] tasks of k_imdct_generic<64> (null: it reads lists and records)
};

// Generic path (any block size 64..8192, any window shape, any channel count / coupling list), two phases so
// that the specialised kernel can run in between (it reads td blocks of generic predecessors and writes td
// right halves for generic successors).
// (the launchers that opt a kernel into a large dynamic LDS segment return the result of that call)
hipError_t lw_launch_generic_imdct(const LwDevTables &T, const LwBatchDev &B, float *tap_spec, hipStream_t st, uint32_t max_n,
		bool any_coupling, bool include_fast);
// Canonicalising pre-pass of the specialised kernels (k_prep, lw_kernels.hip; LwPrepPlan in lw_fast.hpp): for the n_list packets of
// d_list, B.decoupled = residues after every coupling step (x floor curve for the channels d_action marks), d_floors_out (may be
// null) = their floor records with the unit floor for those channels.
hipError_t lw_launch_prep(const LwDevTables &T, const LwBatchDev &B, const uint32_t *d_list, uint32_t n_list, const uint8_t *d_action,
		uint16_t *d_floors_out, hipStream_t st);
// entropy stage on the device (lw_kernels_entropy.hip): floor records and residue vectors of n packets from their raw bytes
struct LwEntTables;
struct LwEntPacket;
hipError_t lw_launch_entropy(const LwEntTables &T, const LwEntPacket *d_pk, const LwPacketRec *d_recs, const uint32_t *d_pool,
		uint16_t *d_floor, float *d_res, uint32_t n, hipStream_t st);
void lw_launch_generic_ola(const LwDevTables &T, const LwBatchDev &B, void *out, int fmt, hipStream_t st, bool include_fast);

// Stream-major rows (k_rows, lw_kernels_rows.hip): a segmented copy of a batch's packet-major PCM (elements of elem_size = 2 or 4
// bytes at d_src) into a rows buffer at d_dst.  A piece = `count` consecutive elements from element src_elem of the source to
// element dst_elem of the destination (64-bit: a rows buffer may hold more than 2^32 elements); the host cuts segments into pieces
// of at most LW_ROWS_PIECE elements (lw_rows.cpp), one wave moves one piece.  Nothing outside the pieces' destinations is written.
struct LwRowSeg {
	uint32_t src_elem;
	uint32_t count;
	uint64_t dst_elem;
};
static_assert(sizeof(LwRowSeg) == 16, "LwRowSeg is read as one 16-byte descriptor");
#define LW_ROWS_PIECE 2048u
hipError_t lw_launch_rows(const void *d_src, void *d_dst, const LwRowSeg *d_segs, uint32_t n_segs, int elem_size, hipStream_t st);

// Stream-major rows through a channel matrix (k_rows_mix, lw_kernels_rows_mix.hip).  A piece = `count` sample positions of ONE
// packet, all channels: input channel c of position p is element src_elem + c * src_stride + p of the source (planar;
// src_stride = the packet's n_samples) or src_elem + p * in_ch + c (interleaved; src_stride = 1), output channel o of position p
// is element dst_elem + o * row_capacity + p (planar) or dst_elem + p * out_ch + o (interleaved) of the destination, 64-bit.
// The host cuts a packet's kept range into pieces of at most LW_ROWS_MIX_PIECE positions (lw_rows_mix.cpp), one wave takes one
// piece.  d_coef: out_ch * in_ch floats in device memory, coef[o * in_ch + c]; the folding rule is the one of
// include/lewton_amd.h (lw_rows_synth_mix).  Nothing outside the pieces' destinations is written.
struct LwRowMixPiece {
	uint32_t src_elem;
	uint32_t src_stride;
	uint32_t count;
	uint32_t pad_;
	uint64_t dst_elem;
};
static_assert(sizeof(LwRowMixPiece) == 24, "LwRowMixPiece is read as six dwords");
#define LW_ROWS_MIX_PIECE 512u
#define LW_ROWS_MIX_OUT 8u // == LW_ROWS_MIX_MAX_OUT of the public header
hipError_t lw_launch_rows_mix(const void *d_src, void *d_dst, const LwRowMixPiece *d_pieces, uint32_t n_pieces, const float *d_coef,
		uint32_t in_ch, uint32_t out_ch, uint64_t row_capacity, int elem_size, bool interleaved, hipStream_t st);

// Specialised long-block path (lw_kernels_long.hip): optional halo pre-pass + main pass.
struct LwFastLaunch;
hipError_t lw_launch_long(const LwDevTables &T, const LwBatchDev &B, const LwFastLaunch &L, void *out, int fmt, hipStream_t st);
// The same design for blocksize_1 = 10 (k_long10, lw_long10.inc): L.d_image = the block kernel's image for 32 lanes per block
// (LwBlkLayout<32>), the work list and the halo pre-pass as for k_long with 512-value residue vectors.
hipError_t lw_launch_long10(const LwDevTables &T, const LwBatchDev &B, const LwFastLaunch &L, void *out, int fmt, hipStream_t st);
// ... and for blocksize_1 = 12 (k_long12, lw_long12.inc): one wave per channel (L.units = the split units), L.d_image = LwL12Layout
hipError_t lw_launch_long12(const LwDevTables &T, const LwBatchDev &B, const LwFastLaunch &L, void *out, int fmt, hipStream_t st);
// k_mix10: k_long10<EDGE> and k_short<8 / 16> in one launch (arguments as lw_launch_mix)
struct LwShortLaunch;
bool lw_mix10_applicable(const LwFastLaunch &LL, const LwShortLaunch &LS, int n_cus);
hipError_t lw_launch_mix10(const LwDevTables &T, const LwBatchDev &B, const LwFastLaunch &LL, const LwShortLaunch &LS, uint32_t *d_flags,
		uint32_t *d_err, uint32_t spin, bool drop_flags, void *out, int fmt, hipStream_t st);
// Short blocks of such streams (k_short, same translation unit); runs after lw_launch_long (it reads the edge buffer).
struct LwShortLaunch;
hipError_t lw_launch_short(const LwDevTables &T, const LwBatchDev &B, const LwShortLaunch &L, void *out, int fmt, hipStream_t st);
// Long blocks of 4096 / 8192 points (k_big, lw_kernels_big.hip): the same slot descriptors, L.lanes = 128 / 256
hipError_t lw_launch_big(const LwDevTables &T, const LwBatchDev &B, const LwShortLaunch &L, void *out, int fmt, hipStream_t st);
// Both in ONE launch (k_mix, same translation unit) where lw_mix_applicable says so; d_flags: [packets][2][ch] dwords, zero.
bool lw_mix_applicable(const LwFastLaunch &LL, const LwShortLaunch &LS, int n_cus);
// d_err: the batch's device error word (device-visible host memory): a short block's wave that does not see its edge flags within
// `spin` polls (0 = the default, about a second) raises it and stores nothing.  drop_flags: test hook, no producer signals.
hipError_t lw_launch_mix(const LwDevTables &T, const LwBatchDev &B, const LwFastLaunch &LL, const LwShortLaunch &LS, uint32_t *d_flags,
		uint32_t *d_err, uint32_t spin, bool drop_flags, void *out, int fmt, hipStream_t st);
